"""State boundaries (the exact K-segment dynamic programme over the rows in time order) of synthetic soft latents: the
device time of the prefix launches, of one layer and of the trace (device events, the fastest of three runs after a
warm-up), the wall time of a whole table, the agreement of the recovered boundaries and segment labels with the planted
states, and -- with --host -- the numpy f64 restatement of one layer on the host.

    python tools/run_segments.py [N L K] [--host] [--out FILE]

Default size: 12298 x 50 in 17 states, K = 17.  run_scores.soft_latents sorts its labels, so the rows are in state order:
the planted states are 17 contiguous runs.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import sfv_amd as sfv  # noqa: E402
from run_scores import device_ms, soft_latents  # noqa: E402


def host_layer(P, Q, prev, m, rows=256):
    """The layer's definition in numpy f64, in blocks of `rows` ends: out[t] = min over s <= t - m with prev[s] finite of
    prev[s] + (Q[t] - Q[s]) - sum_l (P[t]_l - P[s]_l)^2 / (t - s), ties to the lower s; (+inf, -1) without a candidate"""
    N1, L = P.shape
    out, arg = np.full(N1, np.inf), np.full(N1, -1, dtype=np.int32)
    fin = np.isfinite(prev)
    pf = np.where(fin, prev, 0.0)
    for t0 in range(0, N1, rows):
        t = np.arange(t0, min(N1, t0 + rows))
        C = max(int(t[-1]) - m + 1, 1)
        s = np.arange(C)
        valid = (s[None, :] <= t[:, None] - m) & fin[None, :C]
        d2 = np.zeros((len(t), C))
        for l in range(L):
            df = P[t, l][:, None] - P[None, :C, l]
            d2 += df * df
        n = np.where(valid, t[:, None] - s[None, :], 1).astype(np.float64)
        cand = np.where(valid, pf[None, :C] + ((Q[t][:, None] - Q[None, :C]) - d2 / n), np.inf)
        a = np.argmin(cand, axis=1)
        some = valid.any(axis=1)
        out[t] = np.where(some, cand[np.arange(len(t)), a], np.inf)
        arg[t] = np.where(some, a, -1)
    return out, arg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shape", nargs="*", type=int, default=[12298, 50, 17], help="N L K")
    ap.add_argument("--host", action="store_true", help="also time the numpy f64 restatement of one layer")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    N, Ld, K = a.shape
    out = open(a.out, "w") if a.out else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()

    Xh, lab = soft_latents(N, Ld, K)
    X = torch.from_numpy(Xh).cuda()
    call, query = sfv._lib.call, sfv._lib.query
    true = np.nonzero(lab[1:] != lab[:-1])[0] + 1
    say(f"{N} x {Ld} soft latents in {len(true) + 1} contiguous states of {np.bincount(lab).min()}..{np.bincount(lab).max()} "
        f"rows, K = {K}")

    P = torch.empty((N + 1, Ld), dtype=torch.float64, device="cuda")
    Q = torch.empty(N + 1, dtype=torch.float64, device="cuda")
    ws = torch.empty(query("rbvae_segment_ws_bytes", N, Ld) // 8, dtype=torch.float64, device="cuda")
    t_pre = device_ms(lambda: call("rbvae_segment_prefix", X, N, Ld, P, Q))
    tab = sfv.segment_table(X, K)                           # also the warm-up of the whole table
    prev = tab.cost[min(1, K - 1)].contiguous()             # D_2: finite from t = 2 on, so the whole triangle is visited
    lo, la = torch.empty(N + 1, dtype=torch.float64, device="cuda"), torch.empty(N + 1, dtype=torch.int32, device="cuda")
    t_lay = device_ms(lambda: call("rbvae_segment_layer", P, Q, N, Ld, prev, 1, lo, la, ws))
    first = torch.full((N + 1,), float("inf"), dtype=torch.float64, device="cuda")
    first[0] = 0.0
    t_first = device_ms(lambda: call("rbvae_segment_layer", P, Q, N, Ld, first, 1, lo, la, ws))
    cuts = torch.empty((K, K), dtype=torch.int32, device="cuda")
    t_tr = device_ms(lambda: call("rbvae_segment_trace", tab.arg, N, K, tab.cost, cuts))
    pairs = N * (N + 1) / 2.0 * Ld
    say(f"  prefix (three launches)                 {t_pre:9.3f} ms")
    say(f"  one layer from D_2 (two launches)       {t_lay:9.3f} ms   {pairs / (t_lay * 1e-3) / 1e9:8.2f} G coordinate pairs/s "
        f"({pairs / 1e9:.2f} G pairs, {query('rbvae_segment_ws_bytes', N, Ld) / 1e6:.1f} MB workspace)")
    say(f"  the first layer (one finite start)      {t_first:9.3f} ms")
    say(f"  trace (K = {K})                          {t_tr:9.3f} ms")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tab = sfv.segment_table(X, K)
    torch.cuda.synchronize()
    t_tab = time.perf_counter() - t0
    say(f"whole table of {K} layers (wall, prefix, trace and the copies of cuts and costs included): {t_tab * 1e3:.3f} ms")

    seg = sfv.segment(X, n_segments=len(true) + 1, max_segments=max(K, len(true) + 1))
    b0, b2 = sfv.boundary_agreement(seg.boundaries, true, 0), sfv.boundary_agreement(seg.boundaries, true, 2)
    agree = sfv.clustering_agreement(lab, seg.labels, K, seg.n_segments)
    km = sfv.kmeans(X, K)
    X64 = Xh.astype(np.float64)
    planted = sum(float(((X64[lab == k] - X64[lab == k].mean(axis=0)) ** 2).sum()) for k in np.unique(lab))
    agree_k = sfv.clustering_agreement(lab, km.labels, K, K)
    say(f"{seg.n_segments} segments against the planted states: boundary F1 {b0['f1']:.4f} at tolerance 0 ({b0['n_matched']} of "
        f"{len(true)} matched), {b2['f1']:.4f} at tolerance 2 ({b2['n_matched']} matched, mean |offset| {b2['mean_abs_offset']:.3f}); "
        f"segment labels ARI {agree['ari']:.4f}, NMI {agree['nmi']:.4f}; k-means (K = {K}, no time order) ARI {agree_k['ari']:.4f}; "
        f"cost {seg.cost:.4f}, of the planted segmentation {planted:.4f}")

    if a.host:
        Ph, Qh, prev_h = P.cpu().numpy(), Q.cpu().numpy(), prev.cpu().numpy()
        t0 = time.perf_counter()
        ho, ha = host_layer(Ph, Qh, prev_h, 1)
        t_host = time.perf_counter() - t0
        call("rbvae_segment_layer", P, Q, N, Ld, prev, 1, lo, la, ws)
        same_o = int((ho.view(np.int64) == lo.cpu().numpy().view(np.int64)).sum())
        same_a = int((ha == la.cpu().numpy()).sum())
        say(f"numpy f64 restatement of that layer on the host ({os.environ.get('OMP_NUM_THREADS', '?')} threads): {t_host:.3f} s, "
            f"{t_host * K:.1f} s for {K} layers; {same_o} of {N + 1} costs bit-equal to the device's, {same_a} argmins equal")
    if out:
        out.close()


if __name__ == "__main__":
    main()
