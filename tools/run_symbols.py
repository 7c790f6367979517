"""Unsupervised symbols (k-means of the soft latents, code symbols, agreement scores, cluster indices) of synthetic soft
latents: the device time of the k-means++ trials, assign, update and decision launches (device events, the fastest of
three runs after a warm-up), the wall time of a whole fit and of the scores, and -- with --host -- scikit-learn's KMeans
from the same initial centres.

    python tools/run_symbols.py [N L K] [--host] [--launches-only] [--out FILE]

Default size: 12298 x 50 in 17 states, K = 17.  --launches-only times the four launches from K spread rows as centres
and leaves out the seeding, the fit and the scores (for sizes at which the host's share of the seeding takes long).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shape", nargs="*", type=int, default=[12298, 50, 17], help="N L K")
    ap.add_argument("--host", action="store_true", help="also run scikit-learn's KMeans from the same initial centres")
    ap.add_argument("--launches-only", action="store_true", help="only the device times of the launches")
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
    say(f"{N} x {Ld} soft latents in {K} states of {np.bincount(lab).min()}..{np.bincount(lab).max()} rows, K = {K}")

    t0 = time.perf_counter()
    idx = np.arange(K, dtype=np.int64) * (N // K) if a.launches_only else sfv.kmeans_plusplus(X, K, 42)
    torch.cuda.synchronize()
    t_pp = time.perf_counter() - t0
    C0 = Xh[idx].astype(np.float64)
    C = torch.from_numpy(C0).cuda()
    T = 2 + int(np.log(K))
    ws = torch.empty(query("rbvae_kmeans_ws_bytes", N, Ld, K) // 8, dtype=torch.float64, device="cuda")
    cand = torch.from_numpy(idx[:T].astype(np.int32)).cuda()
    closest = torch.full((N,), float("inf"), dtype=torch.float64, device="cuda")
    mins, pot = torch.empty((T, N), dtype=torch.float64, device="cuda"), torch.empty(T, dtype=torch.float64, device="cuda")
    label, prev = (torch.full((N,), -1, dtype=torch.int32, device="cuda") for _ in range(2))
    d2 = torch.empty(N, dtype=torch.float64, device="cuda")
    count = torch.empty(K, dtype=torch.int32, device="cuda")
    shift2, within, spread = (torch.empty(K, dtype=torch.float64, device="cuda") for _ in range(3))
    state = torch.zeros(4, dtype=torch.int32, device="cuda")
    scratch = C.clone()

    t_tr = device_ms(lambda: call("rbvae_kmeans_pp_trials", X, N, Ld, cand, T, closest, mins, pot, ws))
    t_as = device_ms(lambda: call("rbvae_kmeans_assign", X, N, Ld, C, K, prev, None, label, d2, None))
    t_up = device_ms(lambda: call("rbvae_kmeans_update", X, N, Ld, label, d2, K, scratch, count, shift2, within, spread, ws, None))
    # a decision that decides: state is reset to {0, 0, 0, changed = 1} before every launch, and with tol = 0 and no
    # max_iter in reach no rule fires, so the kernel adds shift2 and goes through all three; the reset copy is timed alone
    undecided = torch.tensor([0, 0, 0, 1], dtype=torch.int32, device="cuda")

    shift2.fill_(1.0)

    def decide():
        state.copy_(undecided)
        call("rbvae_kmeans_decide", shift2, K, 0.0, 1 << 30, state)

    t_re = device_ms(lambda: state.copy_(undecided))
    t_de = device_ms(decide)
    assert state.cpu().tolist() == [0, 1, 0, 0], state.cpu().tolist()
    say(f"  k-means++ trials (T = {T}, two launches)  {t_tr:9.3f} ms   {float(N) * T * Ld / (t_tr * 1e-3) / 1e9:8.2f} G coordinate pairs/s")
    say(f"  assign                                  {t_as:9.3f} ms   {float(N) * K * Ld / (t_as * 1e-3) / 1e9:8.2f} G coordinate pairs/s")
    say(f"  update (two launches)                   {t_up:9.3f} ms   {float(N) * Ld * 4 / (t_up * 1e-3) / 1e9:8.2f} GB/s of X")
    say(f"  decision, after a reset of the state    {t_de:9.3f} ms   the reset copy alone {t_re:.3f} ms")
    if a.launches_only:
        if out:
            out.close()
        return
    say(f"  k-means++ seeding, whole (wall, {K} centres, host draws and copies included)  {t_pp:.3f} s")

    sfv.kmeans(X, K, init=C0, max_iter=2)                   # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fit = sfv.kmeans(X, K, init=C0)
    torch.cuda.synchronize()
    t_fit = time.perf_counter() - t0
    say(f"whole fit from those centres (wall): {t_fit:.3f} s, {fit.n_iter} iterations ({fit.converged}), "
        f"{t_fit / fit.n_iter * 1e3:.3f} ms per iteration, inertia {fit.inertia:.4f}, {fit.n_empty} empty clusters")

    t0 = time.perf_counter()
    agree = sfv.clustering_agreement(lab, fit.labels, K, K)
    sym, uniq, _ = sfv.code_symbols((X > 0.5).float().contiguous())
    agree_s = sfv.clustering_agreement(lab, sym, K, int(uniq.shape[0]))
    db, ch = sfv.davies_bouldin(X, fit.labels), sfv.calinski_harabasz(X, fit.labels)
    db_s, ch_s = sfv.davies_bouldin(X, lab), sfv.calinski_harabasz(X, lab)
    torch.cuda.synchronize()
    say(f"scores (wall {time.perf_counter() - t0:.3f} s for all of them): k-means against the states ARI {agree['ari']:.4f}, NMI "
        f"{agree['nmi']:.4f}, V {agree['v_measure']:.4f}, FMI {agree['fowlkes_mallows']:.4f}; {uniq.shape[0]} code symbols: ARI "
        f"{agree_s['ari']:.4f}, NMI {agree_s['nmi']:.4f}; Davies-Bouldin {db:.4f} (states {db_s:.4f}), Calinski-Harabasz "
        f"{ch:.4f} (states {ch_s:.4f})")

    if a.host:
        try:
            from sklearn.cluster import KMeans
            from sklearn.metrics import adjusted_rand_score
        except ImportError:
            say("scikit-learn does not import here: no host run")
        else:
            threads = os.environ.get("OMP_NUM_THREADS", "?")
            X64 = Xh.astype(np.float64)
            t0 = time.perf_counter()
            km = KMeans(K, init=C0.copy(), n_init=1, algorithm="lloyd", tol=1e-4).fit(X64)
            t_host = time.perf_counter() - t0
            same = int((km.labels_ == fit.labels.cpu().numpy()).sum())
            say(f"scikit-learn on the host ({threads} threads): KMeans {t_host:.3f} s, {km.n_iter_} iterations, inertia "
                f"{km.inertia_:.4f} (device / host - 1 = {fit.inertia / km.inertia_ - 1:.2e}), {same} of {N} labels equal, ARI "
                f"of the two labellings {adjusted_rand_score(km.labels_, fit.labels.cpu().numpy()):.6f}, centres within "
                f"{np.abs(km.cluster_centers_ - fit.centers.cpu().numpy()).max():.2e}")
    if out:
        out.close()


if __name__ == "__main__":
    main()
