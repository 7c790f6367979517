"""Gaussian mixture of synthetic soft latents (mixture.py, csrc/gmm.hip): the device time of the E-step, M-step and decision
launches (device events, the fastest of three runs after a warm-up), the wall time of a whole fit from given labels and
of gmm_select over K = 2..32, and -- with --host -- scikit-learn's GaussianMixture from the same start.

    python tools/run_mixture.py [N L K] [--host] [--launches-only] [--out FILE]

Default size: 12298 x 50 in 17 states, K = 17.  The start is the states' own labelling with every tenth row moved to the
next state, so neither side spends its time in k-means and both make the same iterations.
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
    ap.add_argument("--host", action="store_true", help="also run scikit-learn's GaussianMixture from the same start")
    ap.add_argument("--launches-only", action="store_true", help="only the device times of the launches")
    ap.add_argument("--select-to", type=int, default=32, help="gmm_select runs K = 2..this")
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
    start = lab.copy()
    start[::10] = (start[::10] + 1) % K
    X = torch.from_numpy(Xh).cuda()
    call, query = sfv._lib.call, sfv._lib.query
    say(f"{N} x {Ld} soft latents in {K} states of {np.bincount(lab).min()}..{np.bincount(lab).max()} rows, K = {K}")

    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device="cuda")     # noqa: E731
    resp = torch.zeros((K, N), dtype=torch.float64, device="cuda")
    resp.scatter_(0, torch.from_numpy(start).cuda().view(1, N), 1.0)
    weights, logc, means, covars, prec = f64(K), f64(K), f64(K, Ld), f64(K, Ld), f64(K, Ld)
    ws, lognorm, lb, hist = f64(query("rbvae_gmm_ws_bytes", N, Ld, K) // 8), f64(N), f64(1), f64(4)
    label = torch.empty(N, dtype=torch.int32, device="cuda")
    state = torch.zeros(4, dtype=torch.int32, device="cuda")
    call("rbvae_gmm_mstep", X, N, Ld, resp, K, 1e-6, weights, means, covars, prec, logc, ws, None)
    scratch = resp.clone()
    t_e = device_ms(lambda: call("rbvae_gmm_estep", X, N, Ld, means, prec, logc, K, scratch, lognorm, None, None))
    t_s = device_ms(lambda: call("rbvae_gmm_estep", X, N, Ld, means, prec, logc, K, None, lognorm, label, None))
    w2, c2, m2, v2, p2 = f64(K), f64(K), f64(K, Ld), f64(K, Ld), f64(K, Ld)
    t_m = device_ms(lambda: call("rbvae_gmm_mstep", X, N, Ld, scratch, K, 1e-6, w2, m2, v2, p2, c2, ws, None))
    undecided = torch.zeros(4, dtype=torch.int32, device="cuda")

    def decide():                                           # tol = 0 and max_iter out of reach: no rule fires
        state.copy_(undecided)
        call("rbvae_gmm_decide", lognorm, N, 0.0, 4, lb, hist, state)

    t_re = device_ms(lambda: state.copy_(undecided))
    t_d = device_ms(decide)
    say(f"  E-step with responsibilities            {t_e:9.3f} ms   {float(N) * K * Ld / (t_e * 1e-3) / 1e9:8.2f} G coordinate pairs/s")
    say(f"  E-step, scoring only (two sweeps)       {t_s:9.3f} ms   {2 * float(N) * K * Ld / (t_s * 1e-3) / 1e9:8.2f} G coordinate pairs/s")
    say(f"  M-step (three launches)                 {t_m:9.3f} ms   {2 * float(N) * K * Ld / (t_m * 1e-3) / 1e9:8.2f} G products/s")
    say(f"  decision, after a reset of the state    {t_d:9.3f} ms   the reset copy alone {t_re:.3f} ms")
    say(f"  an iteration's five launches            {t_e + t_m + t_d - t_re:9.3f} ms of device time")
    if a.launches_only:
        if out:
            out.close()
        return

    sfv.gmm(X, K, init=start, max_iter=2)                   # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fit = sfv.gmm(X, K, init=start)
    torch.cuda.synchronize()
    t_fit = time.perf_counter() - t0
    score = sfv.gmm_score(fit, X)
    say(f"whole fit from the perturbed states (wall): {t_fit:.4f} s, {fit.n_iter} iterations (converged {fit.converged}), "
        f"{t_fit / fit.n_iter * 1e3:.3f} ms per iteration, lower bound {fit.lower_bound:.6f}, score {score:.6f}, BIC "
        f"{sfv.gmm_bic(fit, X):.1f}, AIC {sfv.gmm_aic(fit, X):.1f}")
    agree = sfv.clustering_agreement(lab, fit.labels, K, K)
    proba = sfv.gmm_predict_proba(fit, X)
    say(f"  against the states: ARI {agree['ari']:.4f}, NMI {agree['nmi']:.4f}; mean largest responsibility "
        f"{float(proba.max(dim=1).values.mean()):.4f}")

    ks = list(range(2, min(a.select_to, N) + 1))
    t0 = time.perf_counter()
    table, best, _ = sfv.gmm_select(X, ks)
    torch.cuda.synchronize()
    t_sel = time.perf_counter() - t0
    by_aic = ks[sfv.mixture.choose(table, "aic")]
    say(f"gmm_select over K = {ks[0]}..{ks[-1]} (wall, k-means starts included): {t_sel:.3f} s, "
        f"{sum(r['n_iter'] for r in table)} EM iterations in all; BIC chooses {best}, AIC {by_aic}")

    if a.host:
        try:
            from sklearn.mixture import GaussianMixture
            from sklearn.mixture._gaussian_mixture import _estimate_gaussian_parameters
        except ImportError:
            say("scikit-learn does not import here: no host run")
        else:
            threads = os.environ.get("OMP_NUM_THREADS", "?")
            X64 = Xh.astype(np.float64)
            onehot = np.zeros((N, K))
            onehot[np.arange(N), start] = 1.0
            nk, mu, var = _estimate_gaussian_parameters(X64, onehot, 1e-6, "diag")
            t0 = time.perf_counter()
            gm = GaussianMixture(K, covariance_type="diag", n_init=1, weights_init=nk / N, means_init=mu,
                                 precisions_init=1.0 / var).fit(X64)
            t_host = time.perf_counter() - t0
            same = int((gm.predict(X64) == fit.labels.cpu().numpy()).sum())
            say(f"scikit-learn on the host ({threads} threads): GaussianMixture {t_host:.3f} s, {gm.n_iter_} iterations, lower "
                f"bound {gm.lower_bound_:.6f} (device - host = {fit.lower_bound - gm.lower_bound_:.2e}), {same} of {N} labels "
                f"equal, means within {np.abs(gm.means_ - fit.means.cpu().numpy()).max():.2e}, variances within "
                f"{np.abs(gm.covariances_ / fit.covariances.cpu().numpy() - 1).max():.2e} relative; device fit / host fit = "
                f"{t_fit / t_host:.3f}")
    if out:
        out.close()


if __name__ == "__main__":
    main()
