"""The f64 restatement of csrc/dtw.hip (include/rbvae_hip.h has the definition) that the GPU tests compare bit for bit, the
brute-force enumeration of all warping paths that proves it on tiny inputs, and the one list of inputs and shapes that
test_dtw_cpu.py and test_dtw_gpu.py share.

The cell cost repeats the device's operations: f32 widened to f64, subtract, square, add with l ascending (numpy rounds every
one and fuses none); np.sqrt for "euclidean"; the popcount of the XOR of the rows packed as rbvae_bern_pack packs them for
"hamming".  The table is a plain loop over the cells, visited tile by tile in the library's tile order (any order that respects
the dependencies gives the same table; the tiles matter only to the defect "stale_corner"), one Python float addition per cell.

defect= names the ways such a kernel goes wrong; test_dtw_cpu.py shows that each changes the result on the GPU test's inputs:
  tie_up_first               up (i - 1, j) preferred to the diagonal on a tie
  stale_corner               the first cell of a tile takes D[i0 - 1][j0 - 1] from the frontier row after the tile to the left has
                             overwritten it with its own last row
  band_off_by_one            |i - j| < w for <= w
  subseq_row0_accumulates    row 0 accumulates along j in subsequence mode
  end_last_min               the highest j among the smallest D[N - 1][j] in subsequence mode
"""
import functools
import itertools
import math

import numpy as np

INF = math.inf
DEFECTS = ("tie_up_first", "stale_corner", "band_off_by_one", "subseq_row0_accumulates", "end_last_min")
METRICS = ("sqeuclidean", "euclidean", "hamming")


def pack(codes):
    """rbvae_bern_pack: bit l of a row is codes[i, l] > 0.5, in word l // 32 at position l % 32 -> uint32 [N, 4]"""
    N, L = codes.shape
    bits = np.zeros((N, 4), dtype=np.uint32)
    for l in range(L):
        bits[:, l // 32] |= (codes[:, l] > 0.5).astype(np.uint32) << np.uint32(l % 32)
    return bits


def cost_matrix(X, Y, metric):
    """d(i, j) f64 [N, M] by the device's operation sequence"""
    if metric == "hamming":
        x = pack(X)[:, None, :] ^ pack(Y)[None, :, :]
        return np.unpackbits(np.ascontiguousarray(x).view(np.uint8), axis=-1).sum(axis=-1).astype(np.float64)
    X64, Y64 = X.astype(np.float64), Y.astype(np.float64)
    s = np.zeros((X.shape[0], Y.shape[0]), dtype=np.float64)
    for l in range(X.shape[1]):
        df = X64[:, l][:, None] - Y64[:, l][None, :]
        s = s + df * df
    return np.sqrt(s) if metric == "euclidean" else s


def pack_dirs(dirs):
    """[N, M] directions -> uint8 [N, ceil(M / 4)], cell j in bits 2 (j mod 4); the bits from M on are 3"""
    N, M = dirs.shape
    W = (M + 3) // 4
    full = np.full((N, 4 * W), 3, dtype=np.uint8)
    full[:, :M] = dirs
    full = full.reshape(N, W, 4)
    return (full[:, :, 0] | (full[:, :, 1] << 2) | (full[:, :, 2] << 4) | (full[:, :, 3] << 6)).astype(np.uint8)


def unpack_dirs(packed, M):
    p = np.asarray(packed, dtype=np.uint8)
    return np.stack([(p >> (2 * q)) & 3 for q in range(4)], axis=-1).reshape(p.shape[0], -1)[:, :M]


def trace(dirs, end_j):
    """the walk from (N - 1, end_j) along dirs to the cell with direction 3 -> int64 [len, 2] ascending"""
    i, j = dirs.shape[0] - 1, end_j
    path = []
    while True:
        path.append((i, j))
        d = int(dirs[i, j])
        if d == 3:
            break
        i -= d != 2
        j -= d != 1
        assert i >= 0 and j >= 0 and len(path) < dirs.shape[0] + dirs.shape[1]
    return np.array(path[::-1], dtype=np.int64)


def dtw_from_cost(d, window=None, subsequence=False, tile=(64, 64), defect=None):
    assert defect is None or defect in DEFECTS
    N, M = d.shape
    TI, TJ = tile
    c = d.tolist()
    D = [[INF] * M for _ in range(N)]
    dirs = np.full((N, M), 3, dtype=np.uint8)
    up_first = defect == "tie_up_first"
    row0_start = subsequence and defect != "subseq_row0_accumulates"
    for i0 in range(0, N, TI):
        for j0 in range(0, M, TJ):
            for i in range(i0, min(i0 + TI, N)):
                Di, Dp, ci = D[i], D[i - 1] if i else None, c[i]
                for j in range(j0, min(j0 + TJ, M)):
                    if window is not None and (abs(i - j) >= window if defect == "band_off_by_one" else abs(i - j) > window):
                        continue                            # +inf, direction 3
                    if i == 0 and (j == 0 or row0_start):
                        Di[j] = ci[j]
                        continue
                    dg = Dp[j - 1] if i and j else INF
                    if defect == "stale_corner" and i == i0 and j == j0 and i and j:
                        dg = D[min(i0 + TI, N) - 1][j0 - 1]
                    up = Dp[j] if i else INF
                    lf = Di[j - 1] if j else INF
                    if up_first:
                        k = 1 if up <= dg and up <= lf else (0 if dg <= lf else 2)
                    else:
                        k = 0 if dg <= up and dg <= lf else (1 if up <= lf else 2)
                    Di[j] = ci[j] + (dg, up, lf)[k]
                    dirs[i, j] = k
    D = np.array(D, dtype=np.float64)
    last = D[N - 1]
    if subsequence:
        m = last.min()
        hits = np.nonzero(last == m)[0]
        end = int(hits[-1] if defect == "end_last_min" else hits[0])
    else:
        end = M - 1
    path = trace(dirs, end)
    return {"D": D, "dirs": dirs, "packed": pack_dirs(dirs), "last_row": last.copy(), "path": path, "cost": float(last[end]),
            "start": int(path[0, 1]), "end": end}


def dtw(X, Y, metric="sqeuclidean", window=None, subsequence=False, tile=(64, 64), defect=None):
    return dtw_from_cost(cost_matrix(X, Y, metric), window, subsequence, tile, defect)


def brute(d, window=None, subsequence=False):
    """the smallest sum of d along any warping path (steps (1, 1), (1, 0), (0, 1); from (0, 0) to (N - 1, M - 1), or from any
    (0, j) to any (N - 1, j') in subsequence mode; inside the band), the costs added in path order from the start"""
    N, M = d.shape
    best = [INF]

    def ok(i, j):
        return i < N and j < M and (window is None or abs(i - j) <= window)

    def go(i, j, s):
        if i == N - 1 and (subsequence or j == M - 1):
            best[0] = min(best[0], s)
            if not subsequence:
                return
        for di, dj in ((1, 1), (1, 0), (0, 1)):
            if ok(i + di, j + dj):
                go(i + di, j + dj, float(d[i + di, j + dj]) + s)

    for j in (range(M) if subsequence else (0,)):
        go(0, j, float(d[0, j]))
    return best[0]


# ---- the inputs and shapes the CPU and the GPU tests share ----------------------------------------------------------------------

INPUTS = (("soft", 1), ("soft", 50), ("soft", 128), ("repeat", 50), ("code", 32), ("code", 50), ("code", 128))


def metrics_of(kind):
    return ("hamming",) if kind == "code" else ("sqeuclidean", "euclidean")


@functools.lru_cache(maxsize=None)
def make(kind, N, M, L, seed=0):
    """soft: random f32 rows; repeat: rows drawn from five random rows, so distances tie exactly; code: four random prototypes
    with a few flipped bits, so ties are everywhere -> (X [N, L], Y [M, L]) f32, read-only"""
    r = np.random.RandomState(1000 * seed + 7 * N + 3 * M + L + {"soft": 0, "repeat": 1, "code": 2}[kind] * 100003)
    if kind == "soft":
        X, Y = r.randn(N, L), r.randn(M, L)
    elif kind == "repeat":
        base = r.randn(5, L)
        X, Y = base[r.randint(5, size=N)], base[r.randint(5, size=M)]
    else:
        proto = r.rand(4, L) < 0.5
        X = proto[np.sort(r.randint(4, size=N))] ^ (r.rand(N, L) < 0.04)
        Y = proto[np.sort(r.randint(4, size=M))] ^ (r.rand(M, L) < 0.04)
    X, Y = X.astype(np.float32), Y.astype(np.float32)
    X.setflags(write=False)
    Y.setflags(write=False)
    return X, Y


def small_shapes(TI, TJ):
    return [(1, 1), (1, 7), (7, 1), (2, 2), (TI - 1, TJ + 1), (TI, TJ), (TI + 1, TJ - 1)]


def multi_tile_shapes(TI, TJ):
    return [(2 * TI + 5, 3 * TJ + 3), (3 * TI + 1, TJ + 2), (5, 3 * TJ + 1), (3 * TI + 1, 5)]


def global_cases(TI, TJ):
    """(kind, L, N, M)"""
    return [(k, L, N, M) for (N, M) in small_shapes(TI, TJ) + multi_tile_shapes(TI, TJ) for (k, L) in INPUTS]


def tiles_outside(N, M, w, TI, TJ):
    """the number of tiles with no cell inside the band"""
    n = 0
    for i0, j0 in itertools.product(range(0, N, TI), range(0, M, TJ)):
        i1, j1 = min(i0 + TI, N) - 1, min(j0 + TJ, M) - 1
        n += i0 - j1 > w or j0 - i1 > w
    return n


def band_windows(N, M, TI, TJ):
    """|N - M|, one more, a tile edge, one more, and the widest band that still leaves a whole tile outside (where one does);
    a w below |N - M| stays in the list: it is refused, and the tests say so"""
    g = abs(N - M)
    ws = [g, g + 1, TJ, TJ + 1]
    out = [w for w in range(g, max(N, M)) if tiles_outside(N, M, w, TI, TJ)]
    return sorted(set(ws + out[-1:]))


BAND_INPUTS = (("soft", 50, "sqeuclidean"), ("repeat", 50, "euclidean"), ("code", 50, "hamming"))


def band_cases(TI, TJ):
    """(kind, L, metric, N, M, w)"""
    return [(k, L, m, N, M, w) for (N, M) in multi_tile_shapes(TI, TJ) for w in band_windows(N, M, TI, TJ)
            for (k, L, m) in BAND_INPUTS]


@functools.lru_cache(maxsize=None)
def subsequence_case(kind, L, TI, TJ, noise):
    """a clip of TI + 3 rows cut from a Y of 3 TJ + 1 rows at row TJ - 2 (across a tile edge), exact or noisy
    -> (X, Y, position)"""
    n, M = TI + 3, 3 * TJ + 1
    pos = TJ - 2
    r = np.random.RandomState(L + 17 * noise)
    if kind == "code":
        Y = (r.rand(M, L) < 0.5)
        X = Y[pos:pos + n].copy()
        if noise:
            X ^= r.rand(n, L) < 0.05
    else:
        Y = r.randn(M, L)
        X = Y[pos:pos + n].copy()
        if noise:
            X = X + 0.1 * r.randn(n, L)
    return X.astype(np.float32), Y.astype(np.float32), pos


@functools.lru_cache(maxsize=None)
def twice_case(L, TI, TJ):
    """codes: the clip stands twice in Y, so two ends cost 0 -> (X, Y, the two positions)"""
    n, M = TI + 3, 3 * TJ + 1
    r = np.random.RandomState(L + 5)
    Y = r.rand(M, L) < 0.5
    a, b = 3, M - n - 2
    Y[b:b + n] = Y[a:a + n]
    return Y[a:a + n].astype(np.float32), Y.astype(np.float32), (a, b)


def subsequence_cases(TI, TJ):
    """(name, metric, X, Y)"""
    out = []
    for kind, L, metric in (("code", 50, "hamming"), ("soft", 50, "sqeuclidean"), ("soft", 128, "euclidean")):
        for noise in (0, 1):
            X, Y, _ = subsequence_case(kind, L, TI, TJ, noise)
            out.append((f"{kind}{L}-{'noisy' if noise else 'exact'}", metric, X, Y))
    X, Y, _ = twice_case(50, TI, TJ)
    out.append(("twice", "hamming", X, Y))
    return out
