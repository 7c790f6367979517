"""HDBSCAN* of a synthetic sequence of latents (density.py, csrc/hdbscan.hip): the device time of the core distances, of every
Boruvka round's search launch and of the rest of the round, the number of rounds, the host tree, the wall time of a whole fit, and
rbvae_dbscan_adj on the same data in the same run, whose arithmetic the search repeats -- the ratio of the two is reported.
scikit-learn's HDBSCAN is timed on the host only when it imports (and not with --no-host); no time from any other run is quoted.

    python tools/run_hdbscan.py [N L] [--no-host] [--out FILE]

Default size: 12298 x 50, run_dbscan.py's planted chain over min(17, L) states; min_samples = min_cluster_size = 5.  A search is
the fastest of three runs after a warm-up (it only writes the slices' minima, so it repeats); a round changes the state, so each
round is timed once, in a second pass over the whole tree after a first that warms up.
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
from run_scores import device_ms  # noqa: E402


def once_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shape", nargs="*", type=int, default=[12298, 50], help="N L")
    ap.add_argument("--no-host", action="store_true", help="skip scikit-learn on the host")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    N, Ld = a.shape
    K, M = min(17, Ld), 5
    out = open(a.out, "w") if a.out else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()

    Xh, _, states, tr = planted(N, Ld, K)
    X = torch.from_numpy(Xh).cuda()
    call, query = sfv._lib.call, sfv._lib.query
    say(f"{N} x {Ld} latents along a planted chain over {K} states, {int(tr.sum())} transition rows; min_samples = "
        f"min_cluster_size = {M}; no N x N storage: the workspace is {query('rbvae_mst_ws_bytes', N) / 1e6:.2f} MB")
    say("launch                                          device time")
    W = query("rbvae_dbscan_words", N)
    adj = torch.empty((N, W), dtype=torch.int64, device="cuda")
    cnt = torch.empty(N, dtype=torch.int32, device="cuda")
    t_adj = device_ms(lambda: call("rbvae_dbscan_adj", X, N, Ld, 0.64, adj, cnt))
    say(f"  rbvae_dbscan_adj (+ row counts), the yardstick  {t_adj:9.3f} ms")
    t_core = device_ms(lambda: sfv.core_distances(X, M))
    say(f"  core distances (rbvae_knn, k = {M - 1})              {t_core:9.3f} ms")
    c2 = sfv.density._core2(X, N, M)
    comp = torch.empty(N, dtype=torch.int32, device="cuda")
    edges = torch.empty((N - 1, 2), dtype=torch.int32, device="cuda")
    w2 = torch.empty(N - 1, dtype=torch.float64, device="cuda")
    state = torch.empty(4, dtype=torch.int32, device="cuda")
    ws = torch.empty(query("rbvae_mst_ws_bytes", N) // 8, dtype=torch.int64, device="cuda")
    args = (X, c2, N, Ld, comp, edges, w2, state, ws)
    for passes in range(2):
        call("rbvae_mst_start", N, comp, state, ws)
        rows = []
        while not int(state[0]):
            n_comp = int(state[2])
            t_s = device_ms(lambda: call("rbvae_mst_search", *args))
            t_r = once_ms(lambda: call("rbvae_mst_round", *args))
            rows.append((n_comp, t_s, t_r))
    for r, (n_comp, t_s, t_r) in enumerate(rows):
        say(f"  round {r + 1:2d}: {n_comp:6d} components   search {t_s:9.3f} ms   the whole round {t_r:9.3f} ms   "
            f"(rest {t_r - t_s:7.3f} ms)   search / rbvae_dbscan_adj = {t_s / t_adj:.2f}")
    t_search, t_rounds = sum(r[1] for r in rows), sum(r[2] for r in rows)
    say(f"  {len(rows)} rounds: searches {t_search:.3f} ms, rounds {t_rounds:.3f} ms; mean search / rbvae_dbscan_adj = "
        f"{t_search / len(rows) / t_adj:.2f}")

    sfv.hdbscan(X, M)                                       # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    mst = sfv.mutual_reachability_mst(X, M)
    torch.cuda.synchronize()
    t_mst = time.perf_counter() - t0
    host = (mst.edges.cpu().numpy(), mst.d.cpu().numpy())
    t0 = time.perf_counter()
    sfv.density._host_tree(host[0], host[1], N, M, "eom")
    t_tree = time.perf_counter() - t0
    t0 = time.perf_counter()
    fit = sfv.hdbscan(X, M)
    torch.cuda.synchronize()
    t_fit = time.perf_counter() - t0
    lab, p = fit.labels.cpu().numpy(), fit.probabilities.cpu().numpy()
    keep = lab >= 0
    ari = sfv.clustering_agreement(states[keep], lab[keep].astype(np.int64), K, max(fit.n_clusters, 1))["ari"] if keep.any() else float("nan")
    say(f"tree on the device, sorted (wall): {t_mst:.4f} s, {mst.n_rounds} rounds; host tree (rbvae_hdbscan_tree, wall): {t_tree:.4f} s")
    say(f"whole fit (wall): {t_fit:.4f} s, {fit.n_clusters} clusters, {fit.n_noise} noise rows ({int((~keep & tr).sum())} of them among "
        f"the {int(tr.sum())} transition rows); mean membership strength {p[tr].mean():.3f} on the transition rows, "
        f"{p[~tr].mean():.3f} elsewhere; ARI of the non-noise rows against the states {ari:.4f}")
    t0 = time.perf_counter()
    sweep = sfv.hdbscan_sweep(X, (5, 10, 20, 40), M)
    torch.cuda.synchronize()
    say(f"hdbscan_sweep over min_cluster_size (5, 10, 20, 40), one tree (wall): {time.perf_counter() - t0:.4f} s; clusters "
        f"{[s_.n_clusters for s_ in sweep]}, noise {[s_.n_noise for s_ in sweep]}")
    try:
        if a.no_host:
            raise ImportError
        from sklearn.cluster import HDBSCAN
    except ImportError:
        say("sklearn.cluster.HDBSCAN on the host: not measured" + ("" if a.no_host else " (scikit-learn does not import)"))
    else:
        t0 = time.perf_counter()
        sk = HDBSCAN(min_cluster_size=M, min_samples=M, algorithm="brute", copy=True).fit(Xh.astype(np.float64))
        t_sk = time.perf_counter() - t0
        n_sk = int(sk.labels_.max()) + 1
        say(f"sklearn.cluster.HDBSCAN(algorithm='brute') on the host (wall): {t_sk:.3f} s, {n_sk} clusters, "
            f"{int((sk.labels_ < 0).sum())} noise rows; host / device = {t_sk / t_fit:.1f}")
    if out:
        out.close()


if __name__ == "__main__":
    main()
