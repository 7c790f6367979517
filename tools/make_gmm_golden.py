"""Writes tests/golden/gmm.npz from scikit-learn 1.7.2 alone (the reference is not involved): what
symbols-from-video_amd/mixture.py and tests/_gmm_ref.py are pinned to.

    python tools/make_gmm_golden.py

Input: X of tests/golden/latent_scores.npz (tools/make_scores_golden.py) cast to f64 -- given f32, scikit-learn computes in
f32, which moves its lower bound by up to 6.6e-5; only results are stored.  For K in KS, S in SEEDS:
    init_K_S                KMeans(n_clusters=K, n_init=1, random_state=RandomState(S)).fit(X64).labels_: the labelling
                            GaussianMixture(init_params="kmeans", random_state=S) starts from
    weights_K_S, means_K_S, covars_K_S, n_iter_K_S, converged_K_S, lower_bound_K_S, lower_bounds_K_S
                            GaussianMixture(K, covariance_type="diag", n_init=1, init_params="kmeans", random_state=S).fit(X64)
    predict_K_S, score_samples_K_S, bic_K_S, aic_K_S    of that fit on X64
    *_short                 the K = 8, S = 42 fit with max_iter=3 (not converged)
    *_unused                K = 4 from the labels init_unused, which leave component 2 without a row: scikit-learn's own
                            formulas (_estimate_gaussian_parameters, weights / N) give the start, passed in as weights_init,
                            means_init and precisions_init
"""
import os
import warnings

import numpy as np
import sklearn
from sklearn.cluster import KMeans
from sklearn.exceptions import ConvergenceWarning
from sklearn.mixture import GaussianMixture
from sklearn.mixture._gaussian_mixture import _estimate_gaussian_parameters

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
KS, SEEDS = (2, 8, 17, 32), (0, 42)


def record(out, t, gm, X64):
    out["weights_" + t], out["means_" + t], out["covars_" + t] = gm.weights_, gm.means_, gm.covariances_
    out["n_iter_" + t], out["converged_" + t] = np.int32(gm.n_iter_), np.bool_(gm.converged_)
    out["lower_bound_" + t], out["lower_bounds_" + t] = np.float64(gm.lower_bound_), np.asarray(gm.lower_bounds_, dtype=np.float64)
    out["predict_" + t] = gm.predict(X64).astype(np.int32)
    out["score_samples_" + t] = gm.score_samples(X64)
    out["bic_" + t], out["aic_" + t] = np.float64(gm.bic(X64)), np.float64(gm.aic(X64))
    return (f"{t}: {gm.n_iter_} iterations, converged {gm.converged_}, lower bound {gm.lower_bound_:.6f}, BIC "
            f"{out['bic_' + t]:.2f}, AIC {out['aic_' + t]:.2f}, smallest weight x N {gm.weights_.min() * len(X64):.3f}, "
            f"smallest variance {gm.covariances_.min():.3g}")


def main():
    assert sklearn.__version__ == "1.7.2", sklearn.__version__
    X64 = np.load(os.path.join(GOLDEN, "latent_scores.npz"))["X"].astype(np.float64)
    N = len(X64)
    out, said = {}, []
    for K in KS:
        for seed in SEEDS:
            t = f"{K}_{seed}"
            out["init_" + t] = KMeans(n_clusters=K, n_init=1, random_state=np.random.RandomState(seed)).fit(X64).labels_.astype(np.int32)
            gm = GaussianMixture(K, covariance_type="diag", n_init=1, init_params="kmeans", random_state=seed).fit(X64)
            said.append(record(out, t, gm, X64))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", ConvergenceWarning)
        gm = GaussianMixture(8, covariance_type="diag", n_init=1, init_params="kmeans", random_state=42, max_iter=3).fit(X64)
    said.append(record(out, "short", gm, X64))
    lab = (np.arange(N) * 3 // N).astype(np.int32)
    lab[lab == 2] = 3                                       # component 2 of 4 holds no row
    resp = np.zeros((N, 4))
    resp[np.arange(N), lab] = 1.0
    nk, means, covars = _estimate_gaussian_parameters(X64, resp, 1e-6, "diag")
    gm = GaussianMixture(4, covariance_type="diag", n_init=1, weights_init=nk / N, means_init=means,
                         precisions_init=1.0 / covars).fit(X64)
    out["init_unused"] = lab
    said.append(record(out, "unused", gm, X64))
    path = os.path.join(GOLDEN, "gmm.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes\n  " + "\n  ".join(said))


if __name__ == "__main__":
    main()
