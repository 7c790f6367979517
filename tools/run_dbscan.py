"""Density clustering of a synthetic sequence of latents and of hard codes (density.py, csrc/dbscan.hip): the device time of every
entry (device events, the fastest of three runs after a warm-up), the pairs per second of both graph kernels, the rounds, the wall
time of whole fits, and the wall time of sklearn.cluster.DBSCAN on the same matrices on the host when scikit-learn imports.

    python tools/run_dbscan.py [N L] [--no-host] [--out FILE]

Default size: 12298 x 50.  The latents are a planted chain over min(17, L) states (centres 4 e_k, rows 0.05 N(0, I) around them)
that dwells about 60 rows in a state and crosses to another over 4 evenly spaced transition rows on a bent path; eps = 0.8,
min_samples = 5.  The codes are the same chain over random prototypes, every bit flipped with probability 0.02, a transition row
taking each bit from either side; 4 bits, min_samples = 5.
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
from run_scores import device_ms  # noqa: E402


def planted(N, Ld, K, seed=1, spread=0.05, bridge=4, dwell=60, flip=0.02):
    r = np.random.RandomState(seed)
    centres = 4.0 * np.eye(K, Ld)
    proto = r.rand(K, Ld) < 0.5
    X, C = np.zeros((N, Ld)), np.zeros((N, Ld), dtype=bool)
    s, tr = np.zeros(N, dtype=np.int64), np.zeros(N, dtype=bool)
    t, k = 0, 0
    while t < N:
        n = min(N - t, dwell + int(r.randint(-dwell // 4, dwell // 4 + 1)))
        X[t:t + n] = centres[k] + spread * r.randn(n, Ld)
        C[t:t + n] = proto[k]
        s[t:t + n] = k
        t += n
        nxt = (k + 1 + int(r.randint(K - 1))) % K
        m = min(N - t, bridge)
        bend = r.randn(Ld)
        for b in range(m):
            a = (b + 1.0) / (bridge + 1.0)
            X[t + b] = (1 - a) * centres[k] + a * centres[nxt] + 4.0 * a * (1 - a) * bend + spread * r.randn(Ld)
            C[t + b] = np.where(r.rand(Ld) < a, proto[nxt], proto[k])
            s[t + b] = k if a < 0.5 else nxt
            tr[t + b] = True
        t += m
        k = nxt
    C ^= r.rand(N, Ld) < flip
    return X.astype(np.float32), C.astype(np.float32), s, tr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shape", nargs="*", type=int, default=[12298, 50], help="N L")
    ap.add_argument("--no-host", action="store_true", help="skip scikit-learn on the host")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    N, Ld = a.shape
    K = min(17, Ld)
    EPS, BITS, MS = 0.8, 4, 5
    out = open(a.out, "w") if a.out else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()

    Xh, Ch, states, tr = planted(N, Ld, K)
    X, C = torch.from_numpy(Xh).cuda(), torch.from_numpy(Ch).cuda()
    call, query = sfv._lib.call, sfv._lib.query
    W = query("rbvae_dbscan_words", N)
    say(f"{N} x {Ld} latents and hard codes along a planted chain over {K} states, {int(tr.sum())} transition rows; the graph is "
        f"{N} x {W} words = {N * W * 8 / 1e6:.2f} MB; eps {EPS} / {BITS} bits, min_samples {MS}")
    adj = torch.empty((N, W), dtype=torch.int64, device="cuda")
    cnt = torch.empty(N, dtype=torch.int32, device="cuda")
    bits = sfv.pack_codes(C)
    mask = torch.empty(W, dtype=torch.int64, device="cuda")
    f = [torch.empty(N, dtype=torch.int32, device="cuda") for _ in range(3)]
    labels, nc = torch.empty(N, dtype=torch.int32, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda")
    ws = torch.empty(query("rbvae_dbscan_ws_bytes", N) // 8, dtype=torch.int64, device="cuda")
    state = torch.zeros(4, dtype=torch.int32, device="cuda")
    pairs = float(N) * N

    say("launch                                          device time")
    t_h = device_ms(lambda: call("rbvae_dbscan_adj_bits", bits, N, Ld, BITS, adj, cnt))
    say(f"  graph, Hamming (+ row counts)               {t_h:9.3f} ms   {pairs / (t_h * 1e-3) / 1e9:8.2f} G pairs / s")
    t_e = device_ms(lambda: call("rbvae_dbscan_adj", X, N, Ld, EPS * EPS, adj, cnt))
    say(f"  graph, Euclidean (+ row counts)             {t_e:9.3f} ms   {pairs / (t_e * 1e-3) / 1e9:8.2f} G pairs / s, "
        f"{pairs * Ld / (t_e * 1e-3) / 1e12:.3f} T coordinate steps / s (three f64 operations each)")
    t_c = device_ms(lambda: call("rbvae_dbscan_core", cnt, N, MS, mask, f[0]))
    say(f"  core rows                                   {t_c:9.3f} ms")

    def first_round():
        state.zero_()
        call("rbvae_dbscan_round", adj, mask, N, f[0], f[1], state)

    t_r = device_ms(first_round)
    say(f"  the first round (three launches, state reset){t_r:8.3f} ms   {int(cnt.long().sum())} set bits in the graph")
    fit = sfv.dbscan(None, EPS, MS, graph=(adj, cnt))
    state.zero_()
    src = f[0].clone()
    for it in range(fit.n_rounds):                          # the fixed point, for the labels' timing
        call("rbvae_dbscan_round", adj, mask, N, src if it == 0 else f[1 + (it - 1) % 2], f[1 + it % 2], state)
    t_l = device_ms(lambda: call("rbvae_dbscan_labels", adj, mask, f[1], N, labels, nc, ws))
    say(f"  labels (two launches)                       {t_l:9.3f} ms")

    for name, M, eps, metric in (("Euclidean", X, EPS, "euclidean"), ("Hamming", C, BITS, "hamming")):
        sfv.dbscan(M, eps, MS, metric=metric)               # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fit = sfv.dbscan(M, eps, MS, metric=metric)
        torch.cuda.synchronize()
        t_fit = time.perf_counter() - t0
        lab = fit.labels.cpu().numpy()
        noise = lab < 0
        keep = ~noise
        agree = sfv.clustering_agreement(states[keep], lab[keep].astype(np.int64), K, max(fit.n_clusters, 1))["ari"] if keep.any() else float("nan")
        say(f"whole fit, {name} (wall): {t_fit:.4f} s, {fit.n_rounds} rounds, {fit.n_clusters} clusters, {fit.n_noise} noise rows "
            f"({int((noise & tr).sum())} of them among the {int(tr.sum())} transition rows), {int(fit.core.sum())} core rows; ARI of the "
            f"non-noise rows against the states {agree:.4f}")
        t0 = time.perf_counter()
        sweep = sfv.dbscan_sweep(M, eps, (3, 5, 9, 17), metric=metric)
        torch.cuda.synchronize()
        say(f"  dbscan_sweep over min_samples (3, 5, 9, 17), one graph (wall): {time.perf_counter() - t0:.4f} s; clusters "
            f"{[s_.n_clusters for s_ in sweep]}, noise {[s_.n_noise for s_ in sweep]}")
        if a.no_host:
            continue
        try:
            from sklearn.cluster import DBSCAN
        except ImportError:
            say("  scikit-learn does not import: no host time")
            continue
        Mh = M.cpu().numpy().astype(np.float64)
        t0 = time.perf_counter()
        sk = DBSCAN(eps=eps if metric == "euclidean" else (eps + 0.5) / Ld, min_samples=MS, metric=metric).fit(Mh)
        t_sk = time.perf_counter() - t0
        same = np.array_equal(sk.labels_, lab) and np.array_equal(sk.core_sample_indices_, np.flatnonzero(fit.core.cpu().numpy()))
        say(f"  sklearn.cluster.DBSCAN on the host (wall): {t_sk:.3f} s; labels and core rows {'equal' if same else 'DIFFER from'} "
            f"the device's on every row; host / device = {t_sk / t_fit:.1f}")
    if N <= sfv.density.MAX_KNN_ROWS:
        t0 = time.perf_counter()
        eps = sfv.suggest_eps(X, MS)
        torch.cuda.synchronize()
        say(f"suggest_eps(k = {MS}) = {eps:.4f} (wall {time.perf_counter() - t0:.4f} s, the kNN graph included)")
    if out:
        out.close()


if __name__ == "__main__":
    main()
