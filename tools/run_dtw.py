"""Dynamic time warping of two synthetic sequences of latents (alignment.py, csrc/dtw.hip): the device time of the fill on soft
latents and on packed codes, of the trace and of whole calls, the number of launches, rbvae_dbscan_adj at the same N in the same
run as the all-pairs yardstick, the wall time of a numpy implementation vectorised over anti-diagonals on the host, and the
accuracy of the labels carried from one sequence to the other.

    python tools/run_dtw.py [N M L] [--no-host] [--out FILE]

Default size: 12298 x 9000 x 50.  One chain over min(17, L) states is planted as run_dbscan.py plants it, 1.25 max(N, M) rows
long; A and B are two samplings of its rows at different, varying speeds (the increments of a smooth positive random speed,
scaled to run from the first row to the last; a row may repeat), each with its own noise of 0.02 on the latents and its own
flips of 1 % of the code bits.  The cost phase and the chain of the fill run in one kernel and cannot be timed apart; the fill of
the packed codes runs the same launches and the same chain with almost no cost work, so the two fills are reported side by side
and their difference is what the f64 costs add.  Device times are device events, the fastest of three runs after a warm-up.
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


def sampling(r, n, T):
    """n ascending rows of 0 .. T - 1 at a varying speed: the running sum of a smooth positive random speed"""
    knots = np.exp(0.8 * r.randn(12))
    speed = np.interp(np.linspace(0, 11, n), np.arange(12), knots)
    pos = np.cumsum(speed)
    pos = (pos - pos[0]) / max(pos[-1] - pos[0], 1e-12) * (T - 1)
    return np.floor(pos).astype(np.int64)


def two_samplings(N, M, Ld, K, seed=3):
    T = int(1.25 * max(N, M))
    X, C, s, _ = planted(T, Ld, K)
    r = np.random.RandomState(seed)
    ia, ib = sampling(r, N, T), sampling(r, M, T)
    A = (X[ia] + 0.02 * r.randn(N, Ld)).astype(np.float32)
    B = (X[ib] + 0.02 * r.randn(M, Ld)).astype(np.float32)
    CA = ((C[ia] > 0.5) ^ (r.rand(N, Ld) < 0.01)).astype(np.float32)
    CB = ((C[ib] > 0.5) ^ (r.rand(M, Ld) < 0.01)).astype(np.float32)
    return A, B, CA, CB, s[ia], s[ib]


def host_dtw_cost(A, B):
    """D[N - 1][M - 1] on the host, numpy vectorised over the anti-diagonals (f64 costs by the expanded square, so the value
    differs from the device's in rounding)"""
    A, B = A.astype(np.float64), B.astype(np.float64)
    N, M = len(A), len(B)
    C = (A * A).sum(1)[:, None] + (B * B).sum(1)[None, :] - 2.0 * (A @ B.T)
    np.maximum(C, 0.0, out=C)
    p2 = np.full(N, np.inf)                                 # diagonal k - 2, indexed by i
    p1 = np.full(N, np.inf)                                 # diagonal k - 1
    p1[0] = C[0, 0]
    for k in range(1, N + M - 1):
        lo, hi = max(0, k - (M - 1)), min(k, N - 1)
        i = np.arange(lo, hi + 1)
        cur = np.full(N, np.inf)
        up = np.full(hi - lo + 1, np.inf)
        dg = np.full(hi - lo + 1, np.inf)
        up[i > 0] = p1[i[i > 0] - 1]                        # (i - 1, j) lies on diagonal k - 1
        dg[i > 0] = p2[i[i > 0] - 1]                        # (i - 1, j - 1) on diagonal k - 2 (+inf where j = 0: never written)
        dg[k - i == 0] = np.inf
        lf = np.where(k - i > 0, p1[i], np.inf)             # (i, j - 1) on diagonal k - 1
        cur[i] = C[i, k - i] + np.minimum(np.minimum(dg, up), lf)
        p2, p1 = p1, cur
    return float(p1[N - 1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shape", nargs="*", type=int, default=[12298, 9000, 50], help="N M L")
    ap.add_argument("--no-host", action="store_true", help="skip the numpy implementation on the host")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    N, M, Ld = a.shape
    K = min(17, Ld)
    out = open(a.out, "w") if a.out else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()

    A, B, CA, CB, sa, sb = two_samplings(N, M, Ld, K)
    Ad, Bd, CAd, CBd = (torch.from_numpy(t).cuda() for t in (A, B, CA, CB))
    call, query = sfv._lib.call, sfv._lib.query
    TI, TJ = query("rbvae_dtw_tile_rows"), query("rbvae_dtw_tile_cols")
    nti, ntj = -(-N // TI), -(-M // TJ)
    launches = nti + ntj - 1
    say(f"{N} x {M} x {Ld}: two samplings at varying speeds of one planted chain over {K} states; {N * M / 1e6:.1f} M cells in "
        f"{nti} x {ntj} tiles of {TI} x {TJ}, {launches} launches a fill (one per anti-diagonal of tiles); no N x M doubles: "
        f"dirs {query('rbvae_dtw_dirs_bytes', N, M) / 1e6:.2f} MB, workspace {query('rbvae_dtw_ws_bytes', N, M) / 1e6:.2f} MB")
    say("launch                                               device time")
    W = query("rbvae_dbscan_words", N)
    adj = torch.empty((N, W), dtype=torch.int64, device="cuda")
    cnt = torch.empty(N, dtype=torch.int32, device="cuda")
    t_adj = device_ms(lambda: call("rbvae_dbscan_adj", Ad, N, Ld, 0.64, adj, cnt))
    say(f"  rbvae_dbscan_adj (+ row counts), N x N, the yardstick  {t_adj:9.3f} ms   ({N * N / t_adj / 1e6:.1f} G pairs/s)")
    del adj
    dirs = torch.empty((N, (M + 3) // 4), dtype=torch.uint8, device="cuda")
    last = torch.empty(M, dtype=torch.float64, device="cuda")
    ws = torch.empty(query("rbvae_dtw_ws_bytes", N, M) // 8, dtype=torch.float64, device="cuda")
    path = torch.empty((N + M - 1, 2), dtype=torch.int32, device="cuda")
    state = torch.empty(3, dtype=torch.int32, device="cuda")
    cost = torch.empty(1, dtype=torch.float64, device="cuda")
    ba, bb = sfv.pack_codes(CAd), sfv.pack_codes(CBd)
    t_bits = device_ms(lambda: call("rbvae_dtw_fill_bits", ba, N, bb, M, Ld, -1, 0, dirs, last, None, ws))
    t_tr_bits = device_ms(lambda: call("rbvae_dtw_trace", dirs, last, N, M, 0, path, state, cost))
    len_bits = int(state[0])
    t_soft = device_ms(lambda: call("rbvae_dtw_fill", Ad, N, Bd, M, Ld, 0, -1, 0, dirs, last, None, ws))
    t_root = device_ms(lambda: call("rbvae_dtw_fill", Ad, N, Bd, M, Ld, 1, -1, 0, dirs, last, None, ws))
    call("rbvae_dtw_fill", Ad, N, Bd, M, Ld, 0, -1, 0, dirs, last, None, ws)
    t_tr = device_ms(lambda: call("rbvae_dtw_trace", dirs, last, N, M, 0, path, state, cost))
    len_soft = int(state[0])
    say(f"  rbvae_dtw_fill_bits (hamming: the chain, hardly a cost)  {t_bits:9.3f} ms   {t_bits / launches * 1e3:7.2f} us a launch")
    say(f"  rbvae_dtw_fill (sqeuclidean)                             {t_soft:9.3f} ms   {t_soft / launches * 1e3:7.2f} us a launch, "
        f"{N * M / t_soft / 1e6:.2f} G cells/s; fill / rbvae_dbscan_adj at N x N = {t_soft / t_adj:.1f}")
    say(f"    minus the fill of the codes: what the f64 costs add     {t_soft - t_bits:9.3f} ms")
    say(f"  rbvae_dtw_fill (euclidean: a square root per cell)       {t_root:9.3f} ms")
    say(f"  rbvae_dtw_trace (one workgroup, one lane walks)         {t_tr:9.3f} ms on the latents' path of {len_soft} cells, "
        f"{t_tr_bits:.3f} ms on the codes' of {len_bits}")
    w = max(abs(N - M), max(N, M) // 10)
    t_band = device_ms(lambda: call("rbvae_dtw_fill", Ad, N, Bd, M, Ld, 0, w, 0, dirs, last, None, ws))
    say(f"  rbvae_dtw_fill inside a band of {w:5d} (prefill included) {t_band:9.3f} ms")
    n_clip = min(N, 600)
    clip = Ad[N // 3:N // 3 + n_clip].contiguous()
    t_sub = device_ms(lambda: call("rbvae_dtw_fill", clip, n_clip, Bd, M, Ld, 0, -1, 1, dirs, last, None, ws))
    say(f"  rbvae_dtw_fill, subsequence: a clip of {n_clip} rows of A in B   {t_sub:9.3f} ms")

    results = {}
    for name, x, y, metric in (("latents, sqeuclidean", Ad, Bd, "sqeuclidean"), ("codes, hamming", CAd, CBd, "hamming")):
        sfv.dtw(x, y, metric=metric)                        # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = sfv.dtw(x, y, metric=metric)
        torch.cuda.synchronize()
        t_call = time.perf_counter() - t0
        got = sfv.transfer_labels(res.path, sa, M)
        results[name] = res
        say(f"dtw({name}) (wall, checks, packing and the path's way to the host included): {t_call:.4f} s; cost {res.cost:.6g}, "
            f"path of {res.path_len} cells, normalised cost {res.normalized_cost:.4g}; A's states carried to B: accuracy "
            f"{float((got == sb).mean()):.4f}")
    if a.no_host:
        say("numpy over anti-diagonals on the host: not measured")
    else:
        t0 = time.perf_counter()
        c = host_dtw_cost(A, B)
        t_host = time.perf_counter() - t0
        dev = results["latents, sqeuclidean"].cost
        say(f"numpy over anti-diagonals on the host, the cost only (wall): {t_host:.3f} s; its cost {c:.6g} against the device's "
            f"{dev:.6g} (relative difference {abs(c - dev) / max(abs(dev), 1e-300):.2e}: the host expands the square); host / device "
            f"fill = {t_host * 1e3 / t_soft:.0f}")
    if out:
        out.close()


if __name__ == "__main__":
    main()
