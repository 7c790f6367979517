"""The f64 restatement of the many-sequence entries of csrc/dtw.hip (include/rbvae_hip.h, "Many sequences aligned") that the
GPU tests compare bit for bit, built on the unchanged tests/_dtw_ref.py for every single table: the stack and pair layout, the
launch-by-launch fill of a batch with each pair's own frontiers, path_ranges, the barycenter update and the whole DBA loop, the
distance matrix, the medoid, vote_labels, and the one list of cases that test_dtw_many_cpu.py and test_dtw_many_gpu.py share.

No DTW library is installed here (tslearn, dtw-python and dtaidistance are absent), so there is no fixture; the restatement is
tied down by test_dtw_many_cpu.py: the batched fill against _dtw_ref's plain loop, the range form of the update against a
cell-by-cell accumulation, fixed points, the descent of the objective and planted data.

defect= names the ways such code goes wrong; test_dtw_many_cpu.py shows that each changes a result on the GPU test's cases:
  pair_row_offset          a pair reads its Y rows from the previous sequence's offset
  shared_frontier          all pairs of a batch use one frow / fcol / corner
  launches_of_first_pair   the diagonal count comes from pair 0, not from the largest pair
  range_off_by_one         hi is one too small
  update_sum_f32           the update's sum is kept in f32
  update_divides_by_S      the update divides by S, not by cnt_i
  stale_paths_returned     the returned paths belong to the previous template
  medoid_tie_high          a medoid tie goes to the highest index
  vote_counts_cells        vote_labels counts cells, not one vote per source
"""
import functools
import math

import numpy as np

import _dtw_ref as R

INF = math.inf
DEFECTS = ("pair_row_offset", "shared_frontier", "launches_of_first_pair", "range_off_by_one", "update_sum_f32",
           "update_divides_by_S", "stale_paths_returned", "medoid_tie_high", "vote_counts_cells")


# ---- stacks and pairs -------------------------------------------------------------------------------------------------------------

def row_offsets(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))])


def split(X, lengths):
    o = row_offsets(lengths)
    return [X[o[s]:o[s + 1]] for s in range(len(lengths))]


def all_pairs(S):
    return [(a, b) for a in range(S) for b in range(a + 1, S)]


def layout(len_x, len_y, pairs, tile):
    """rbvae_dtw_pairs_sizes: {"dirs", "last", "ws", "path": int64 [P + 1]}: bytes, doubles, bytes, rows"""
    TI, TJ = tile
    off = {k: [0] for k in ("dirs", "last", "ws", "path")}
    for a, b in pairs:
        n, m = int(len_x[a]), int(len_y[b])
        off["dirs"].append(off["dirs"][-1] + ((n * ((m + 3) // 4) + 15) // 16) * 16)
        off["last"].append(off["last"][-1] + m)
        off["ws"].append(off["ws"][-1] + 8 * (n + m + -(-n // TI) * -(-m // TJ)))
        off["path"].append(off["path"][-1] + n + m - 1)
    return {k: np.array(v, dtype=np.int64) for k, v in off.items()}


def launch_numbers(len_x, len_y, pairs, tile):
    """what rbvae_dtw_pairs_plan returns: (tile anti-diagonals of the largest pair, most tiles of one pair on a diagonal)"""
    TI, TJ = tile
    t = [(-(-int(len_x[a]) // TI), -(-int(len_y[b]) // TJ)) for a, b in pairs]
    return max(i + j - 1 for i, j in t), max(min(i, j) for i, j in t)


def pair_rows(X, len_x, Y, len_y, a, b, defect=None):
    ox, oy = row_offsets(len_x), row_offsets(len_y)
    y0 = oy[b - 1] if defect == "pair_row_offset" and b > 0 else oy[b]
    return X[ox[a]:ox[a] + len_x[a]], Y[y0:y0 + len_y[b]]


def fill_batch(costs, tile, defect=None):
    """The batched fill as the device runs it: one launch per tile anti-diagonal for all pairs, every tile reading the frontier
    row, the frontier column and the corner that earlier launches left, each pair with its own.  Within a launch the pairs are
    taken in order (on the device they run together: with shared frontiers the result is a race, and this is one outcome of it).
    -> per pair {"D", "dirs"}; cells that no launch reached keep NaN and direction 255"""
    TI, TJ = tile
    shapes = [c.shape for c in costs]
    tiles = [(-(-n // TI), -(-m // TJ)) for n, m in shapes]
    n_diag = max(i + j - 1 for i, j in tiles)
    if defect == "launches_of_first_pair":
        n_diag = tiles[0][0] + tiles[0][1] - 1
    own = defect != "shared_frontier"
    N1, M1 = max(n for n, _ in shapes), max(m for _, m in shapes)
    front = [([INF] * (m if own else M1), [INF] * (n if own else N1), {}) for n, m in shapes]
    if not own:
        front = [front[0]] * len(costs)
    out = [{"D": np.full(s, np.nan), "dirs": np.full(s, 255, dtype=np.uint8)} for s in shapes]
    for d in range(n_diag):
        for p, c in enumerate(costs):
            (n, m), (nTi, nTj) = shapes[p], tiles[p]
            frow, fcol, corner = front[p]
            for ti in range(max(0, d - (nTj - 1)), min(d, nTi - 1) + 1):
                tj = d - ti
                i0, j0 = ti * TI, tj * TJ
                nr, nc = min(TI, n - i0), min(TJ, m - j0)
                top = [frow[j0 + k] if i0 else INF for k in range(nc)]
                left = [fcol[i0 + k] if j0 else INF for k in range(nr)]
                cor = corner[(ti - 1, tj - 1)] if i0 and j0 else INF
                Dt = [[0.0] * nc for _ in range(nr)]
                for r in range(nr):
                    for k in range(nc):
                        if i0 + r == 0 and j0 + k == 0:
                            Dt[r][k], out[p]["dirs"][0, 0] = float(c[0, 0]), 3
                            continue
                        dg = Dt[r - 1][k - 1] if r and k else (cor if not r and not k else (top[k - 1] if not r else left[r - 1]))
                        up = Dt[r - 1][k] if r else top[k]
                        lf = Dt[r][k - 1] if k else left[r]
                        q = 0 if dg <= up and dg <= lf else (1 if up <= lf else 2)
                        Dt[r][k] = float(c[i0 + r, j0 + k]) + (dg, up, lf)[q]
                        out[p]["dirs"][i0 + r, j0 + k] = q
                out[p]["D"][i0:i0 + nr, j0:j0 + nc] = Dt
                frow[j0:j0 + nc] = Dt[nr - 1]
                for r in range(nr):
                    fcol[i0 + r] = Dt[r][nc - 1]
                if nr == TI and nc == TJ:
                    corner[(ti, tj)] = Dt[nr - 1][nc - 1]
    return out


def align_pairs(X, len_x, Y, len_y, pairs, metric, tile, defect=None):
    """every pair's R.dtw result ("packed", "last_row", "path", "cost", "start", "end", "D", "dirs"), the batch defects
    included; a defect that leaves a table unfinished gives path None"""
    rows = [pair_rows(X, len_x, Y, len_y, a, b, defect) for a, b in pairs]
    if defect not in ("shared_frontier", "launches_of_first_pair"):
        return [R.dtw(x, y, metric, tile=tile) for x, y in rows]
    got = fill_batch([R.cost_matrix(x, y, metric) for x, y in rows], tile, defect)
    out = []
    for g in got:
        done = not np.any(g["dirs"] == 255)
        path = R.trace(g["dirs"], g["dirs"].shape[1] - 1) if done else None
        out.append({"D": g["D"], "dirs": g["dirs"], "packed": R.pack_dirs(g["dirs"] & 3), "last_row": g["D"][-1].copy(),
                    "path": path, "cost": float(g["D"][-1, -1]), "start": 0, "end": g["D"].shape[1] - 1})
    return out


# ---- ranges and the update ----------------------------------------------------------------------------------------------------------

def path_ranges(path, n, defect=None):
    """lo, hi int32 [n]: the first and the last j aligned with row i of an ascending path"""
    lo, hi = np.full(n, -1, dtype=np.int32), np.full(n, -1, dtype=np.int32)
    for k, (i, j) in enumerate(path.tolist()):
        if k == 0 or path[k - 1, 0] != i:
            lo[i] = j
        if k == len(path) - 1 or path[k + 1, 0] != i:
            hi[i] = j - 1 if defect == "range_off_by_one" else j
    return lo, hi


def update(seqs, ranges, T, defect=None):
    """rbvae_dtw_barycenter_update: for every template row the f64 sum of the aligned rows, s ascending, j ascending, every
    addition rounded once (numpy adds the L coordinates side by side, each in its own order), one division by the count, one
    rounding to f32 -> (T' f32 [T, L], count int32 [T])"""
    Ld = seqs[0].shape[1]
    acc_t = np.float32 if defect == "update_sum_f32" else np.float64
    out, count = np.zeros((T, Ld), dtype=np.float32), np.zeros(T, dtype=np.int32)
    for i in range(T):
        acc, cnt = np.zeros(Ld, dtype=acc_t), 0
        for y, (lo, hi) in zip(seqs, ranges):
            for j in range(int(lo[i]), int(hi[i]) + 1):
                acc = acc + y[j].astype(acc_t)
            cnt += max(int(hi[i]) - int(lo[i]) + 1, 0)
        div = len(seqs) if defect == "update_divides_by_S" else cnt
        with np.errstate(invalid="ignore", divide="ignore"):   # a defect's empty range: the device's 0 / 0 as well
            out[i] = (acc.astype(np.float64) / np.float64(div)).astype(np.float32)
        count[i] = cnt
    return out, count


def update_by_cells(seqs, paths, T):
    """the same mean accumulated cell by cell along the paths (a path is ascending, so a row's cells come in j order)"""
    Ld = seqs[0].shape[1]
    acc, cnt = np.zeros((T, Ld), dtype=np.float64), np.zeros(T, dtype=np.int64)
    for y, p in zip(seqs, paths):
        for i, j in p.tolist():
            acc[i] = acc[i] + y[j].astype(np.float64)
            cnt[i] += 1
    return (acc / cnt[:, None].astype(np.float64)).astype(np.float32), cnt.astype(np.int32)


def objective(tmpl, seqs, paths):
    """sum over all path cells of |t_i - y_j|^2 in exact-as-possible arithmetic (math.fsum of f64 products)"""
    terms = []
    t64 = tmpl.astype(np.float64)
    for y, p in zip(seqs, paths):
        df = t64[p[:, 0]] - y.astype(np.float64)[p[:, 1]]
        terms += (df * df).reshape(-1).tolist()
    return math.fsum(terms)


# ---- the matrix, the medoid, the votes ----------------------------------------------------------------------------------------------

def distance_matrix(seqs, metric, tile):
    """-> {"cost", "path_len", "normalized", "results": {(a, b): R.dtw result, a < b}}"""
    S = len(seqs)
    cost, plen, results = np.zeros((S, S)), np.diag(np.array([len(s) for s in seqs], dtype=np.int64)), {}
    for a, b in all_pairs(S):
        r = R.dtw(seqs[a], seqs[b], metric, tile=tile)
        cost[a, b] = cost[b, a] = r["cost"]
        plen[a, b] = plen[b, a] = len(r["path"])
        results[(a, b)] = r
    return {"cost": cost, "path_len": plen, "normalized": cost / plen, "results": results}


def medoid(cost, defect=None):
    S = len(cost)
    total = [0.0] * S
    for a in range(S):
        for b in range(S):
            total[a] = total[a] + float(cost[a, b])
    best = min(total)
    hits = [a for a in range(S) if total[a] == best]
    total = np.array(total)
    return {"index": hits[-1] if defect == "medoid_tie_high" else hits[0], "total": total,
            "mean_to_others": total / (S - 1) if S > 1 else np.zeros(S)}


def transfer_counts(path, labels_a, M, K):
    """votes [M, K]: the path cells of every row of Y by the label of their row of X"""
    v = np.zeros((M, K), dtype=np.int64)
    for i, j in np.asarray(path).tolist():
        v[j, labels_a[i]] += 1
    return v


def transfer(path, labels_a, M, K):
    v = transfer_counts(path, labels_a, M, K)
    out = v.argmax(axis=1).astype(np.int64)
    out[v.sum(axis=1) == 0] = -1
    return out


def vote(paths, labels, M, K, defect=None):
    """every source's transfer is one vote per row; the most frequent label, the smallest on a tie, -1 where nobody votes.
    paths[s] has the source's rows first.  vote_counts_cells pools the path cells of all sources instead."""
    v = np.zeros((M, K), dtype=np.int64)
    for p, la in zip(paths, labels):
        if defect == "vote_counts_cells":
            v += transfer_counts(p, la, M, K)
        else:
            t = transfer(p, la, M, K)
            ok = t >= 0
            v[np.nonzero(ok)[0], t[ok]] += 1
    out = v.argmax(axis=1).astype(np.int64)
    out[v.sum(axis=1) == 0] = -1
    return out


def vote_vectors(vectors):
    """vote_labels on label vectors, one loop per row"""
    vectors = [np.asarray(v) for v in vectors]
    out = []
    for j in range(len(vectors[0])):
        seen = [int(v[j]) for v in vectors if v[j] >= 0]
        out.append(min(set(seen), key=lambda k: (-seen.count(k), k)) if seen else -1)
    return np.array(out, dtype=np.int64)


# ---- DBA ------------------------------------------------------------------------------------------------------------------------------

def barycenter(seqs, init, max_iter, tol, tile, defect=None):
    """the loop of the header and of alignment.dtw_barycenter; init: "medoid", an index or an array [T, L]
    -> {"template", "inertia": the history, "n_iter", "reason", "paths", "costs", "count"}"""
    if isinstance(init, str):
        init = medoid(distance_matrix(seqs, "sqeuclidean", tile)["cost"])["index"]
    tmpl = np.array(seqs[init] if isinstance(init, (int, np.integer)) else init, dtype=np.float32)
    T = len(tmpl)

    def align(t):
        res = [R.dtw(t, y, "sqeuclidean", tile=tile) for y in seqs]
        total = 0.0
        for r in res:
            total = total + r["cost"]
        return total, res

    history, aligned, best, it = [], [], None, 0
    while True:
        inertia, res = align(tmpl)
        history.append(inertia)
        aligned.append(res)
        returned = it
        if it >= 1 and inertia > best[0]:
            reason, (_, tmpl, res, returned) = "increased", best
            break
        best = (inertia, tmpl, res, it)
        if it >= 1 and history[it - 1] - inertia <= tol * history[it - 1]:
            reason = "converged"
            break
        if it == max_iter:
            reason = "max_iter"
            break
        ranges = [path_ranges(r["path"], T, defect) for r in res]
        tmpl, _ = update(seqs, ranges, T, defect)
        it += 1
    if defect == "stale_paths_returned" and returned >= 1:
        res = aligned[returned - 1]
    ranges = [path_ranges(r["path"], T) for r in res]
    count = np.sum([hi - lo + 1 for lo, hi in ranges], axis=0).astype(np.int32)
    return {"template": tmpl, "inertia": history, "n_iter": it, "reason": reason, "paths": [r["path"] for r in res],
            "costs": [r["cost"] for r in res], "count": count}


# ---- the cases the CPU and the GPU tests share ----------------------------------------------------------------------------------------------

INPUTS = R.INPUTS                                           # (kind, L): soft 1 / 50 / 128, repeat 50, code 32 / 50 / 128
SECOND_BATCH = [(5, 0), (0, 5), (3, 3), (2, 4), (2, 4)]


def stack_lengths(TI):
    return (1, 2, TI - 1, TI, TI + 1, 2 * TI + 2)


@functools.lru_cache(maxsize=None)
def make_stack(kind, L, lengths, seed=0):
    """one stack of sequences of the given lengths, made as R.make makes its rows -> X f32 [sum, L], read-only"""
    n = int(sum(lengths))
    X, _ = R.make(kind, n, 1, L, seed=seed + 11)
    return X


@functools.lru_cache(maxsize=None)
def stack_reference(kind, L, metric, TI, TJ, second):
    lengths = stack_lengths(TI)
    X = make_stack(kind, L, lengths)
    pairs = SECOND_BATCH if second else all_pairs(len(lengths))
    return align_pairs(X, lengths, X, lengths, pairs, metric, (TI, TJ))


@functools.lru_cache(maxsize=None)
def planted(S, n, L, seed, noise=0.05, states=5):
    """a base chain of n rows that dwells in `states` planted states, and S copies sampled from it at varying speeds (every
    base row at least once, some repeated) with noise added -> (base f32 [n, L], [copies], [the base row of every copy row],
    the base's states int64 [n])"""
    r = np.random.RandomState(seed)
    centres = r.randn(states, L)
    state = (np.arange(n) * states) // n
    base = (centres[state] + 0.15 * np.cumsum(r.randn(n, L), axis=0) / np.sqrt(n)).astype(np.float32)
    copies, picks = [], []
    for _ in range(S):
        rep = 1 + (r.rand(n) < 0.15) + (r.rand(n) < 0.05)
        pick = np.repeat(np.arange(n), rep)
        y = base[pick] + (noise * r.randn(len(pick), L) if noise else 0.0)
        copies.append(y.astype(np.float32))
        picks.append(pick)
    base.setflags(write=False)
    return base, copies, picks, state.astype(np.int64)


DBA_CASE = dict(S=4, n=150, L=3, seed=3, max_iter=5, tol=1e-6)      # copies of about 150 to 200 rows: three tiles a side
DBA_RUNS = (("medoid", 5), (0, 5), ("tensor", 5), (0, 2))           # (init, max_iter)


@functools.lru_cache(maxsize=None)
def dba_reference(init, TI, TJ, max_iter=None):
    """init: "medoid", an index, or "tensor" (the base chain itself); max_iter 5 reaches a fixed point, where the last two
    templates have the same paths, so DBA_RUNS also stops one at 2, where the paths still move"""
    c = DBA_CASE
    base, copies, _, _ = planted(c["S"], c["n"], c["L"], c["seed"])
    start = base if init == "tensor" else init
    return barycenter(copies, start, c["max_iter"] if max_iter is None else max_iter, c["tol"], (TI, TJ))


def update_cases(TI):
    """(name, template length, the sequences' lengths, L)"""
    return [("three", TI + 1, (TI - 3, TI + 9, 2 * TI + 1), 1), ("three", TI + 1, (TI - 3, TI + 9, 2 * TI + 1), 50),
            ("one_row_sequence", 7, (1, 9), 3), ("one_row_template", 1, (5, 1, TI + 2), 3)]


@functools.lru_cache(maxsize=None)
def update_case(T, lengths, L, TI, TJ):
    """-> (template, [sequences], [R.dtw results], [(lo, hi)], (T', count))"""
    r = np.random.RandomState(T + 7 * L + sum(lengths))
    tmpl = r.randn(T, L).astype(np.float32)
    seqs = [r.randn(m, L).astype(np.float32) for m in lengths]
    res = [R.dtw(tmpl, y, "sqeuclidean", tile=(TI, TJ)) for y in seqs]
    ranges = [path_ranges(x["path"], T) for x in res]
    return tmpl, seqs, res, ranges, update(seqs, ranges, T)


@functools.lru_cache(maxsize=None)
def videos_case():
    """three tiny planted "videos" as latents: (latents [F_v, 6], states, frame indices, flags) per video"""
    base, copies, picks, state = planted(3, 24, 6, seed=9, noise=0.02, states=3)
    out = []
    for v, (y, pick) in enumerate(zip(copies, picks)):
        st = state[pick]
        frames = list(range(100 * (v + 1), 100 * (v + 1) + len(y)))
        flags = [frames[int(np.nonzero(st == k)[0][0])] for k in (1, 2)]
        out.append((y, st, frames, flags))
    return out


# a tie between rows 0 and 2 (totals 5, 6, 5, 9), and three sources of which one alone has many path cells on row 0
MEDOID_TIE = np.array([[0.0, 2.0, 1.0, 2.0], [2.0, 0.0, 1.0, 3.0], [1.0, 1.0, 0.0, 3.0], [2.0, 3.0, 3.0, 0.0]])
VOTE_CASE = {"M": 2, "K": 2, "labels": [np.array([1, 1, 1, 0]), np.array([0, 0]), np.array([0, 1])],
             "paths": [np.array([[0, 0], [1, 0], [2, 0], [3, 1]]), np.array([[0, 0], [1, 1]]), np.array([[0, 0], [1, 1]])]}
