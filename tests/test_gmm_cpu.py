"""CPU: tests/_gmm_ref.py (the f64 restatement the GPU tests compare the mixture kernels and mixture.py with) against the
scikit-learn fixture tests/golden/gmm.npz (tools/make_gmm_golden.py) and, on one case, the installed scikit-learn; each
check of the GPU tests against the named defect it has to reject; and the host side of mixture.py.

Measured here, over K in {2, 8, 17, 32} x seed in {0, 42}: n_iter (7, 10, 11, 8, 15, 12, 11, 5), converged and predict
equal scikit-learn's; lower_bound within 2.2e-14 and its history within 5.0e-14, score_samples within 1.1e-11 (K = 32, seed
42; 1.6e-12 on the others), means within 1.3e-14 and weights within 6.7e-16 (gates 1e-10); variances within 3.1e-11 relative
(K = 32, seed 42, where they reach 2e-6 and scikit-learn's expanded square cancels; 1e-8); BIC within 2.0e-15 and AIC within
6.5e-15 relative (1e-10).  The smallest gap between a row's two largest weighted log-probabilities is above 0.03 and no
change of the lower bound is within 5e-6 of tol.  The start equals
tests/golden/kmeans.npz's labels on all eight cases.  weights_over_n is not separated by any gate on a fit: see
test_weights_over_n_needs_unnormalised_responsibilities and DESIGN.md."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _gmm_ref as R
import sfv_amd as sfv

HERE = os.path.dirname(os.path.abspath(__file__))
KS, SEEDS = R.KS, R.SEEDS


@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(os.path.join(HERE, "golden", "gmm.npz")))
    g["X"] = np.load(os.path.join(HERE, "golden", "latent_scores.npz"))["X"]
    return g


@pytest.fixture(scope="module")
def fits(gold):
    return {(K, s): R.fit(gold["X"], gold[f"init_{K}_{s}"], K) for K in KS for s in SEEDS}


def test_fixture_size_and_start(gold):
    assert os.path.getsize(os.path.join(HERE, "golden", "gmm.npz")) <= 400 * 1024
    km = np.load(os.path.join(HERE, "golden", "kmeans.npz"))
    for K in KS:
        for s in SEEDS:                                     # the start is the fit symbols.kmeans reproduces label for label
            assert np.array_equal(gold[f"init_{K}_{s}"], km[f"labels_{K}_{s}"]), (K, s)
    assert [int(gold[f"n_iter_{K}_{s}"]) for K in KS for s in SEEDS] == [7, 10, 11, 8, 15, 12, 11, 5]


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("K", KS)
def test_fit_equals_sklearn(gold, fits, K, seed):
    t, fit = f"{K}_{seed}", fits[(K, seed)]
    bad, diff = R.against_fixture(fit, gold, t)
    print(f"K = {K}, seed {seed}: {fit['n_iter']} iterations, " + ", ".join(f"{k} {v:.3g}" for k, v in diff.items()))
    assert not bad, (bad, diff)
    assert fit["converged"] and fit["lower_bound"] == fit["lower_bounds"][-1] and len(fit["lower_bounds"]) == fit["n_iter"]
    lp = R.estep(gold["X"], fit["means"], fit["prec"], fit["logc"])[0]
    top = np.sort(lp, axis=1)
    assert (top[:, -1] - top[:, -2]).min() > 0.03           # no row is undecided between two components
    change = np.abs(np.diff(np.concatenate([[-np.inf], fit["lower_bounds"]])))
    assert np.abs(change - 1e-3).min() > 5e-6               # no stop decision rests on rounding


def test_short_and_unused_cases(gold):
    short = R.fit(gold["X"], gold["init_8_42"], 8, max_iter=3)
    bad, diff = R.against_fixture(short, gold, "short")
    assert not bad and not short["converged"] and short["n_iter"] == 3, (bad, diff)
    unused = R.fit(gold["X"], gold["init_unused"], 4)
    bad, diff = R.against_fixture(unused, gold, "unused")
    print("unused component: " + ", ".join(f"{k} {v:.3g}" for k, v in diff.items()))
    assert not bad, (bad, diff)
    assert not (gold["init_unused"] == 2).any() and unused["weights"][2] < 1e-15
    assert np.all(unused["means"][2] == 0.0) and np.all(unused["covars"][2] == 1e-6) and not (unused["labels"] == 2).any()


def test_selection_rule(gold, fits):
    for s in SEEDS:
        assert R.choose(KS, [float(gold[f"bic_{K}_{s}"]) for K in KS]) == 2
        assert R.choose(KS, [float(gold[f"aic_{K}_{s}"]) for K in KS]) == 8
        assert R.choose(KS, [fits[(K, s)]["bic"] for K in KS]) == 2 and R.choose(KS, [fits[(K, s)]["aic"] for K in KS]) == 8
    assert R.choose((5, 3, 4), [1.0, 1.0, 2.0]) == 3          # a tie goes to the smaller K
    table = [{"K": 5, "bic": 1.0, "aic": 3.0}, {"K": 3, "bic": 1.0, "aic": 4.0}, {"K": 4, "bic": 2.0, "aic": 0.5}]
    assert sfv.mixture.choose(table, "bic") == 1 and sfv.mixture.choose(table, "aic") == 2
    with pytest.raises(ValueError, match="criterion"):
        sfv.mixture.choose(table, "icl")
    assert sfv.mixture.n_parameters(17, 50) == R.n_parameters(17, 50) == 1716


def test_live_sklearn(gold, fits):
    GaussianMixture = pytest.importorskip("sklearn.mixture").GaussianMixture
    K, seed = 8, 42
    X64 = gold["X"].astype(np.float64)
    gm = GaussianMixture(K, covariance_type="diag", n_init=1, init_params="kmeans", random_state=seed).fit(X64)
    fit = fits[(K, seed)]
    assert gm.n_iter_ == fit["n_iter"] and gm.converged_ and abs(gm.lower_bound_ - fit["lower_bound"]) <= 1e-10
    assert np.abs(gm.means_ - fit["means"]).max() <= 1e-10 and np.abs(gm.covariances_ / fit["covars"] - 1).max() <= 1e-8
    assert np.abs(gm.precisions_cholesky_ / fit["prec"] - 1).max() <= 1e-8
    assert np.array_equal(gm.predict(X64), fit["labels"]) and np.abs(gm.score_samples(X64) - fit["score_samples"]).max() <= 1e-10
    assert np.abs(gm.predict_proba(X64) - R.estep(X64, fit["means"], fit["prec"], fit["logc"])[2]).max() <= 1e-10
    assert abs(gm.bic(X64) / fit["bic"] - 1) <= 1e-10 and abs(gm.aic(X64) / fit["aic"] - 1) <= 1e-10


# ---- the checks reject the named defects -----------------------------------------------------------------------------------

def far_case():
    """one row 1e3 standard deviations from every mean, in every coordinate"""
    X, means, prec, logc, _, covars = R.params_case(65, 3, 4)
    X[7] = (means.max() + 1e3 * np.sqrt(covars.max())).astype(np.float32)
    return X, means, prec, logc


def tie_case():
    """components 1 and 3 are component 0 and 2 again, weights included: every row ties exactly"""
    X, means, prec, logc, _, _ = R.params_case(300, 5, 2)
    return X, np.concatenate([means, means]), np.concatenate([prec, prec]), np.concatenate([logc, logc])


@pytest.mark.parametrize("defect", ["var_not_centred_on_new_mean", "no_reg_covar", "logdet_sign", "lower_bound_after_mstep",
                                    "n_iter_off_by_one", "bic_param_count_full"])
def test_fit_defects_rejected(gold, defect):
    K, seed = 32, 42                                        # variances reach 2e-6 here: reg_covar = 1e-6 shows
    bad, diff = R.against_fixture(R.fit(gold["X"], gold[f"init_{K}_{seed}"], K, defect=defect), gold, f"{K}_{seed}")
    print(f"{defect}: outside their gates: {bad}")
    assert bad, diff
    want = {"var_not_centred_on_new_mean": "covars_rel", "no_reg_covar": "covars_rel", "logdet_sign": "lower_bound",
            "lower_bound_after_mstep": "lower_bounds", "n_iter_off_by_one": "n_iter", "bic_param_count_full": "bic_rel"}[defect]
    assert want in bad


def test_nk_without_eps_rejected(gold):
    with np.errstate(all="ignore"):
        bad, _ = R.against_fixture(R.fit(gold["X"], gold["init_unused"], 4, defect="nk_without_eps"), gold, "unused")
    assert "means" in bad and "lower_bound" in bad          # 0 / 0: the unused component's mean is not a number


def test_stop_on_relative_change_rejected(gold):
    moved = [(K, s) for K in KS for s in SEEDS
             if R.fit(gold["X"], gold[f"init_{K}_{s}"], K, defect="stop_on_relative_change")["n_iter"] != int(gold[f"n_iter_{K}_{s}"])]
    print(f"stop_on_relative_change: n_iter differs on {moved}")
    assert len(moved) >= 4


def test_estep_defects_rejected():
    X, means, prec, logc = far_case()
    ref = R.estep_bounds(X, means, prec, logc)
    lp, lognorm, resp, label = R.estep(X, means, prec, logc)
    assert np.isfinite(ref["lognorm"]).all() and ref["lognorm"][7] < -1e5
    R.within(lognorm, ref["lognorm"], ref["b_ln"], "f64 lognorm against long double")
    R.within(resp, ref["resp"], ref["b_r"], "f64 resp against long double")
    assert abs(resp[7].sum() - 1.0) <= ref["b_r"][7].sum() + 4 * R.U < 1e-6
    with np.errstate(all="ignore"):
        bad = R.estep(X, means, prec, logc, "lognorm_without_max")[1]
    assert not np.isfinite(bad[7]) and R.rejects(bad, ref["lognorm"], ref["b_ln"])       # exp underflows to 0: log 0
    X, means, prec, logc = tie_case()
    lp, _, resp, label = R.estep(X, means, prec, logc)
    high = R.estep(X, means, prec, logc, "tie_high")[3]
    assert np.array_equal(lp[:, :2], lp[:, 2:]) and np.all(label < 2) and np.array_equal(high, label + 2)
    assert np.array_equal(resp[:, :2], resp[:, 2:])


def test_weights_over_n_needs_unnormalised_responsibilities(gold):
    """rows of responsibilities add to 1, so sum_k nk = N + K * 10 eps and nk / N differs from nk / sum nk by 2e-16 relative
    on the fixture: no gate of a fit separates the two.  The M-step entry itself takes any responsibilities, and on
    unnormalised ones the weights' bound and their sum do."""
    K, seed = 32, 42
    bad, _ = R.against_fixture(R.fit(gold["X"], gold[f"init_{K}_{seed}"], K, defect="weights_over_n"), gold, f"{K}_{seed}")
    assert not bad
    X = R.soft_rows(300, 5, 1)
    resp = 0.7 * R.resp_case(300, 4, "soft")
    w, mu, var, _, _, _ = R.mstep(X, resp)
    ref = R.mstep_bounds(X, resp, 1e-6, mu, var, w)
    R.within(w, ref["weights"], ref["b_weights"], "weights")
    assert abs(w.sum() - 1.0) <= 2 * 4 * R.U
    wrong = R.mstep(X, resp, defect="weights_over_n")[0]
    assert R.rejects(wrong, ref["weights"], ref["b_weights"]) and abs(wrong.sum() - 1.0) > 0.2


@pytest.mark.parametrize("N,Ld,K", [c for c in R.ESTEP_CASES if c[0] <= 300])
def test_estep_cases_are_decided_and_bounds_hold(N, Ld, K):
    """the synthetic inputs of the GPU E-step test: no row is undecided, the f64 restatement is inside the bounds and a
    relative error of 1e-12 outside"""
    X, means, prec, logc, _, _ = R.params_case(N, Ld, K)
    ref = R.estep_bounds(X, means, prec, logc)
    lp, lognorm, resp, label = R.estep(X, means, prec, logc)
    assert ref["decided"].all() and np.array_equal(label, ref["label"])
    R.within(lp, ref["lp"], ref["b_lp"], "lp")
    R.within(lognorm, ref["lognorm"], ref["b_ln"], "lognorm")
    R.within(resp, ref["resp"], ref["b_r"], "resp")
    assert R.rejects(ref["lognorm"] * (1 + 1e-10), ref["lognorm"], ref["b_ln"])
    if Ld == 128:
        assert R.chunk_components(Ld) == 16 and K == 17


@pytest.mark.parametrize("kind", ["soft", "one_hot", "empty", "one"])
def test_mstep_bounds_hold(kind):
    X = R.soft_rows(300, 7, 3)
    resp = R.resp_case(300, 5, kind)
    w, mu, var, s, logc, nk = R.mstep(X, resp)
    ref = R.mstep_bounds(X, resp, 1e-6, mu, var, w)
    for name, got in (("nk", nk), ("means", mu), ("covars", var), ("weights", w), ("prec", s), ("logc", logc)):
        R.within(got, ref[name], ref["b_" + name], f"{name} ({kind})")
    assert R.rejects(mu * (1 + 1e-11) + 1e-13, ref["means"], ref["b_means"])
    if kind == "one_hot":                                   # equal to the per-cluster mean and variance
        lab = resp.argmax(axis=1)
        for k in range(5):
            rows = X[lab == k].astype(np.float64)
            assert np.abs(mu[k] - rows.mean(0)).max() <= 1e-14 and np.abs(var[k] - (rows.var(0) + 1e-6)).max() <= 1e-14
    if kind == "empty":
        assert nk[2] == R.NK_EPS and np.all(mu[2] == 0.0) and np.all(var[2] == 1e-6)
    lb = R.lower_bound(np.linspace(-9.0, 2.0, 2500))
    assert abs(lb - (-3.5)) <= R.lower_bound_bound(np.linspace(-9.0, 2.0, 2500))


# ---- the host side of the package ------------------------------------------------------------------------------------------

NEW = ("rbvae_gmm_ok", "rbvae_gmm_chunk_components", "rbvae_gmm_ws_bytes", "rbvae_gmm_estep", "rbvae_gmm_mstep", "rbvae_gmm_decide")


def test_header_and_library():
    protos = sfv._lib.parse_header()
    raw = ctypes.CDLL(sfv._lib.LIB_PATH)
    for name in NEW:
        assert name in protos and hasattr(raw, name), name
    assert [len(protos[n][1]) for n in NEW] == [3, 1, 3, 12, 14, 8]
    q = sfv._lib.query
    assert q("rbvae_version") >= 104
    assert q("rbvae_gmm_ok", 12298, 50, 17) == 1 and q("rbvae_gmm_ok", 1 << 20, 128, 64) == 1 and q("rbvae_gmm_ok", 1, 1, 1) == 1
    assert q("rbvae_gmm_ok", 1 << 20, 128, 65) == 0 and q("rbvae_gmm_ok", 1 << 18, 2, 256) == 1      # N K <= 2^26
    assert q("rbvae_gmm_ok", (1 << 18) + 1, 2, 256) == 0 and q("rbvae_gmm_ok", (1 << 20) + 1, 2, 2) == 0
    assert q("rbvae_gmm_ok", 3, 2, 4) == 0 and q("rbvae_gmm_ok", 300, 129, 4) == 0 and q("rbvae_gmm_ok", 300, 4, 257) == 0
    assert q("rbvae_gmm_ok", 300, 0, 4) == 0 and q("rbvae_gmm_ok", 300, 4, 0) == 0
    for Ld in (1, 3, 8, 9, 50, 128):
        assert q("rbvae_gmm_chunk_components", Ld) == R.chunk_components(Ld)
    assert q("rbvae_gmm_chunk_components", 0) == 0 and q("rbvae_gmm_chunk_components", 129) == 0
    assert R.chunk_components(128) == 16 and R.chunk_components(8) == 256
    assert q("rbvae_gmm_ws_bytes", 300, 129, 4) == 0
    for shape in ((12298, 50, 17), (1 << 20, 128, 64), (65537, 2, 2), (1, 1, 1)):
        assert q("rbvae_gmm_ws_bytes", *shape) == R.ws_bytes(*shape)
    assert q("rbvae_gmm_ws_bytes", 12298, 50, 17) == 16 * 49 * 17 * 51 and R.blocks_rows(65537) == (256, 257)


def test_cpu_inputs_raise():
    X = torch.zeros((8, 4))
    fit = sfv.GMMResult(*([None] * 10))
    for call in (lambda: sfv.gmm(X, 2), lambda: sfv.gmm_select(X, [2, 3]),
                 lambda: sfv.latent_mixture(None, torch.zeros((2, 3, 8, 8)), [0, 1], [1])):
        with pytest.raises(ValueError, match="GPU"):
            call()
    with pytest.raises(ValueError, match="tensor"):
        sfv.gmm(np.zeros((8, 4), dtype=np.float32), 2)
    with pytest.raises(ValueError, match="ks is empty"):
        sfv.gmm_select(X, [])
    assert fit.means is None and sfv.mixture.gmm is sfv.gmm and sfv.mixture.MAX_COMPONENTS == 256 and sfv.mixture.ENQUEUE == 8
