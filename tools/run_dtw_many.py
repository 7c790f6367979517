"""Many recordings aligned (alignment.py, the batched entries of csrc/dtw.hip): the device time of the batched all-pairs fill and
trace against a loop of the single-pair entries over the same pairs on the same device in the same session, the launches of
either, one DBA iteration split into fill, trace, ranges and update, the wall time of dtw_distance_matrix and dtw_barycenter,
the medoid and the outlier scores, and the accuracy of the states carried to a held-out recording three ways.

    python tools/run_dtw_many.py [S N L] [--out FILE]

Default size: 8 3000 50.  One chain over min(17, L) states is planted as run_dbscan.py plants it; the S recordings are S samplings
of its rows at different, varying speeds as run_dtw.py makes its two, of 0.85 N to 1.15 N rows, each with its own noise of 0.02.
Device times are device events around the calls, after a warm-up; the batched form and the loop are timed in turn, five times
each, and the fastest of each is reported with the slowest beside it.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import sfv_amd as sfv  # noqa: E402
from run_dbscan import planted  # noqa: E402
from run_dtw import sampling  # noqa: E402


def recordings(S, N, Ld, K, seed=3):
    lengths = [int(round(N * f)) for f in np.linspace(0.85, 1.15, S)] if S > 1 else [N]
    T = int(1.25 * max(lengths))
    X, _, s, _ = planted(T, Ld, K)
    r = np.random.RandomState(seed)
    rows = [sampling(r, n, T) for n in lengths]
    return [(X[i] + 0.02 * r.randn(len(i), Ld)).astype(np.float32) for i in rows], [s[i] for i in rows], lengths


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def in_turn(fns, repeat=5):
    """every fn warmed up once, then timed in turn `repeat` times -> [(fastest, slowest) ms]"""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    t = [[timed(fn) for fn in fns] for _ in range(repeat)]
    return [(min(r[k] for r in t), max(r[k] for r in t)) for k in range(len(fns))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shape", nargs="*", type=int, default=[8, 3000, 50], help="S N L")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    S, N, Ld = a.shape
    K = min(17, Ld)
    out = open(a.out, "a") if a.out else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()

    seqs, states, lengths = recordings(S, N, Ld, K)
    X = torch.from_numpy(np.concatenate(seqs)).cuda()
    rows = np.concatenate([[0], np.cumsum(lengths)])
    call, query = sfv._lib.call, sfv._lib.query
    TI, TJ = query("rbvae_dtw_tile_rows"), query("rbvae_dtw_tile_cols")
    lx = np.ascontiguousarray(lengths, dtype=np.int32)
    pairs = [(p, b) for p in range(S) for b in range(p + 1, S)]
    P = len(pairs)
    tiles = [(-(-lengths[p] // TI), -(-lengths[b] // TJ)) for p, b in pairs]
    cells = sum(lengths[p] * lengths[b] for p, b in pairs)
    batch = sfv.alignment._PairBatch(lx, lx, pairs, X.device)
    say(f"{S} recordings of {min(lengths)} .. {max(lengths)} rows x {Ld}: samplings at varying speeds of one planted chain over {K} "
        f"states; {P} pairs a < b, {cells / 1e6:.1f} M cells; device buffers of the batch: dirs {batch.dirs_bytes / 1e6:.2f} MB, "
        f"workspace {batch.ws_bytes / 1e6:.2f} MB, paths {batch.path_rows * 8 / 1e6:.2f} MB")
    say(f"launches: batched fill {batch.n_diag} (one per tile anti-diagonal of the largest pair, grid up to {batch.max_tiles} x {P}) "
        f"+ 1 trace; the loop {sum(i + j - 1 for i, j in tiles)} fills + {P} traces; on the longest diagonal "
        f"{sum(min(i, j) for i, j in tiles)} of the {batch.max_tiles * P} workgroups have a tile")

    single = []
    for p, b in pairs:
        n, m = lengths[p], lengths[b]
        single.append((X[rows[p]:rows[p + 1]], n, X[rows[b]:rows[b + 1]], m,
                       torch.empty(query("rbvae_dtw_dirs_bytes", n, m), dtype=torch.uint8, device="cuda"),
                       torch.empty(m, dtype=torch.float64, device="cuda"),
                       torch.empty(query("rbvae_dtw_ws_bytes", n, m) // 8, dtype=torch.float64, device="cuda"),
                       torch.empty((n + m - 1, 2), dtype=torch.int32, device="cuda"),
                       torch.empty(3, dtype=torch.int32, device="cuda"), torch.empty(1, dtype=torch.float64, device="cuda")))

    def fill_batched():
        call("rbvae_dtw_pairs_fill", X, X.shape[0], X, X.shape[0], Ld, 0, batch.plan, P, batch.n_diag, batch.max_tiles, batch.dirs,
             batch.dirs_bytes, batch.last_row, batch.last_n, batch.ws, batch.ws_bytes)

    def trace_batched():
        call("rbvae_dtw_pairs_trace", batch.dirs, batch.dirs_bytes, batch.last_row, batch.last_n, batch.plan, P, batch.path,
             batch.path_rows, batch.state, batch.cost)

    def fill_loop():
        for x, n, y, m, dirs, last, ws, _, _, _ in single:
            call("rbvae_dtw_fill", x, n, y, m, Ld, 0, -1, 0, dirs, last, None, ws)

    def trace_loop():
        for _, n, _, m, dirs, last, _, path, state, cost in single:
            call("rbvae_dtw_trace", dirs, last, n, m, 0, path, state, cost)

    (fb, fb1), (fl, fl1), (tb, tb1), (tl, tl1) = in_turn([fill_batched, fill_loop, trace_batched, trace_loop])
    same = all(torch.equal(batch.cost[k], s[9][0]) and torch.equal(batch.state[k], s[8]) for k, s in enumerate(single))
    say("all pairs, sqeuclidean                       device time, fastest (slowest) of 5, timed in turn")
    say(f"  rbvae_dtw_pairs_fill, one batch             {fb:9.3f} ms ({fb1:.3f})   {fb / batch.n_diag * 1e3:7.2f} us a launch, "
        f"{cells / fb / 1e6:.2f} G cells/s")
    say(f"  rbvae_dtw_fill, a loop over the same pairs  {fl:9.3f} ms ({fl1:.3f})   loop / batch = {fl / fb:.2f}")
    say(f"  rbvae_dtw_pairs_trace, one workgroup a pair {tb:9.3f} ms ({tb1:.3f})")
    say(f"  rbvae_dtw_trace, a loop                     {tl:9.3f} ms ({tl1:.3f})   loop / batch = {tl / tb:.2f}")
    say(f"  fill + trace: batch {fb + tb:.3f} ms, loop {fl + tl:.3f} ms, loop / batch = {(fl + tl) / (fb + tb):.2f}; "
        f"every pair's cost and state equal in both: {same}")

    for name, fn in (("dtw_distance_matrix", lambda: sfv.dtw_distance_matrix(X, lengths)),):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        matrix = fn()
        torch.cuda.synchronize()
        say(f"{name} (wall; checks, plan, buffers and the paths' way to the host included): {time.perf_counter() - t0:.4f} s")
    med = sfv.dtw_medoid(matrix["cost"])
    say(f"medoid: recording {med['index']}; mean cost to the others " + " ".join(f"{v:.4g}" for v in med["mean_to_others"]))

    # one DBA iteration on the medoid as the template, all S recordings on the column side
    k = med["index"]
    tmpl = X[rows[k]:rows[k + 1]].clone()
    T = tmpl.shape[0]
    lt = np.array([T], dtype=np.int32)
    tb_ = sfv.alignment._PairBatch(lt, lx, [(0, s) for s in range(S)], X.device)
    lo = torch.empty((S, T), dtype=torch.int32, device="cuda")
    hi = torch.empty((S, T), dtype=torch.int32, device="cuda")
    new, count = torch.empty_like(tmpl), torch.empty(T, dtype=torch.int32, device="cuda")

    def dba_fill():
        call("rbvae_dtw_pairs_fill", tmpl, T, X, X.shape[0], Ld, 0, tb_.plan, S, tb_.n_diag, tb_.max_tiles, tb_.dirs, tb_.dirs_bytes,
             tb_.last_row, tb_.last_n, tb_.ws, tb_.ws_bytes)

    def dba_trace():
        call("rbvae_dtw_pairs_trace", tb_.dirs, tb_.dirs_bytes, tb_.last_row, tb_.last_n, tb_.plan, S, tb_.path, tb_.path_rows,
             tb_.state, tb_.cost)

    def dba_ranges():
        for s in range(S):
            tb_.ranges(s, lo[s], hi[s])

    def dba_update():
        call("rbvae_dtw_barycenter_update", X, X.shape[0], Ld, tb_.plan, S, lo, hi, T, new, count)

    t = in_turn([dba_fill, dba_trace, dba_ranges, dba_update])
    say(f"one DBA iteration, template of {T} rows against {S} recordings: fill {t[0][0]:.3f} ms ({tb_.n_diag} launches), trace "
        f"{t[1][0]:.3f} ms, ranges {t[2][0]:.3f} ms ({S} launches), update {t[3][0]:.3f} ms; longest run of one template row "
        f"{int((hi - lo + 1).max())} rows, {int(count.sum())} rows added in all")
    sfv.dtw_barycenter(X, lengths, init=k, max_iter=1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    bary = sfv.dtw_barycenter(X, lengths, init=k, max_iter=10)
    torch.cuda.synchronize()
    say(f"dtw_barycenter(init = the medoid, max_iter = 10) (wall): {time.perf_counter() - t0:.4f} s; {bary.n_iter} updates, "
        f"{bary.reason}; inertia " + " ".join(f"{v:.6g}" for v in bary.inertia))

    # the last recording held out: the barycenter of the others, then its states three ways
    if S >= 3:
        h = S - 1
        fitted = list(range(S - 1))
        part = sfv.dtw_barycenter(X[:rows[h]], lengths[:h], init="medoid", max_iter=10)
        paths = dict(zip(fitted, (r.path for r in part.results)))
        paths[h] = sfv.dtw_pairs(part.template, [part.template.shape[0]], [(0, 0)], Y=X[rows[h]:], lengths_y=[lengths[h]])[0].path
        got = sfv.alignment.transfer_three_ways(matrix, states, paths, fitted, h)
        acc = {w: float((got[w] == states[h]).mean()) for w in ("nearest", "vote", "barycenter")}
        say(f"recording {h} held out: its states from the nearest recording ({got['source']}) alone {acc['nearest']:.4f}, by the vote "
            f"of the other {S - 1} {acc['vote']:.4f}, through the barycenter of the others ({part.n_iter} updates, {part.reason}) "
            f"{acc['barycenter']:.4f}")
    if out:
        out.close()


if __name__ == "__main__":
    main()
