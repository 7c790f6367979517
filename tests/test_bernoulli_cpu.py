"""CPU: tests/_bernoulli_ref.py (the f64 restatement the GPU tests compare csrc/bernoulli.hip and bernoulli.py with) against its
long double twin inside the bounds it derives, against scikit-learn's BernoulliNB through tests/golden/bernoulli.npz, against
the hidden Markov model whose pi and rows of A equal the mixture's weights, and on the planted chains; and the host side of
bernoulli.py.

Measured here: the restatement is at most 0.81 of its long double bounds (lp at L = 2, where the bound is two roundings; lb
0.19, lognorm 0.05, resp 0.12, e 0.37, theta 0.013, log(1 - theta) 0.30); against scikit-learn log theta 0.19, log(1 - theta)
0.16, log w 0.07, lp 0.04 and the responsibilities 0.02 of the bounds for its forms (4.8e-15, 3.1e-14, 6.7e-15, 1e-12, 2e-12).
The planted chains, from _kmeans_ref's start: nine_states (900 x 25, 9 states, flip 0.3) ARI 0.324 -> 0.929 in 10 iterations,
the closest stop decision 3.47e-4 from tol; hundred_bits (600 x 100, 5 states, flip 0.35) 0.838 -> 0.988 in 4, 4.83e-4; the
fixture's codes 0.963 -> 0.991 in 3, 7.1e-4; the mixture alone reaches 0.347, 0.855 and 0.963, its closest decision 8.4e-6
(nine_states).  The f64 / long double differences (the device gates are 64 times
these) are printed by test_planted_chains and quoted in DESIGN.md."""
import ctypes

import numpy as np
import pytest
import torch

import _gmm_ref as G
import _hmm_ref as H
import _bernoulli_ref as R
import sfv_amd as sfv

CASES = [(2, 1, 1), (257, 128, 17), (300, 2, 64), (300, 33, 65), (65, 128, 20)]


# ---- the restatement against long double -------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,L,K", CASES)
def test_emit_and_estep_within_long_double_bounds(N, L, K):
    X, logt, logf, logw = R.tables_case(N, L, K)
    ref = R.emit_bounds(X, logt, logf)
    lb, m, e = R.emit(X, logt, logf)
    w = [R.within(lb, ref["lb"], ref["b_lb"], "lb"), R.within(m, ref["m"], ref["b_m"], "m"), R.within(e, ref["e"], ref["b_e"], "e")]
    assert (e.max(axis=1) == 1.0).all() and np.array_equal(m, lb.max(axis=1))
    er = R.estep_bounds(X, logt, logf, logw)
    lp, lognorm, resp, label = R.estep(X, logt, logf, logw)
    w += [R.within(lp, er["lp"], er["b_lp"], "lp"), R.within(lognorm, er["lognorm"], er["b_ln"], "lognorm"),
          R.within(resp, er["resp"], er["b_r"], "resp")]
    assert np.array_equal(label[er["decided"]], er["label"][er["decided"]]) and er["decided"].mean() > 0.9
    assert np.array_equal(lp, lb + logw[None, :])           # log w is added last
    print(f"({N}, {L}, {K}): worst |err|/bound lb, m, e, lp, lognorm, resp = " + ", ".join(f"{x:.3g}" for x in w))
    if L > 1:                                               # one table entry cannot round
        assert R.rejects(lb * (1 + 1e-12), ref["lb"], ref["b_lb"])
    assert R.rejects(lognorm + 1e-11, er["lognorm"], er["b_ln"]) and R.rejects(resp * (1 + 1e-11), er["resp"], er["b_r"])
    assert R.rejects(e * (1 + 1e-11), ref["e"], ref["b_e"]) or K == 1


@pytest.mark.parametrize("N,L,K,kind", [(2, 1, 1, "soft"), (300, 33, 5, "soft"), (300, 128, 7, "empty"), (1025, 7, 3, "one_hot")])
def test_mstep_within_long_double_bounds(N, L, K, kind):
    X = R.tables_case(N, L, K)[0]
    resp = G.resp_case(N, K, kind)
    got = R.mstep(X, resp, 0.75)
    ref = R.mstep_bounds(X, resp, 0.75, got)
    w = [R.within(got[n], ref[n], ref["b_" + n], n) for n in ("S", "nk", "theta", "weights", "logt", "logf", "logw")]
    print(f"M-step ({N}, {L}, {K}, {kind}): worst |err|/bound S, nk, theta, weights, logt, logf, logw = "
          + ", ".join(f"{x:.3g}" for x in w))
    assert abs(float(got["weights"].astype(R.LD).sum()) - 1) <= 2 * K * R.U
    if kind == "empty":                                     # a component without mass: theta = 1 / 2
        assert np.all(got["theta"][K // 2] == 0.5) and np.all(got["S"][K // 2] == 0) and got["weights"][K // 2] < 1e-14
    assert R.rejects(got["theta"] * (1 + 1e-11), ref["theta"], ref["b_theta"])
    assert R.rejects(got["logf"] + 1e-13, ref["logf"], ref["b_logf"])
    assert R.block_partials(X, resp).shape == (G.blocks_rows(N)[0], K, L + 1)


def test_pack():
    X = R.tables_case(70, 33, 1)[0]
    w = R.pack(X)
    assert w.shape == (70, 4) and w.dtype == np.uint32 and np.all(w[:, 2:] == 0) and np.all(w[:, 1] < 2)
    bits = (w[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :]) & 1
    assert np.array_equal(bits.reshape(70, 128)[:, :33].astype(bool), X > 0.5) and (X == 0.5).any()


# ---- scikit-learn's BernoulliNB ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("a", [0, 1])
def test_against_scikit_learn(a):
    g = R.golden()
    X, s = g["X"].astype(np.float32), g["states"]
    N, L, K = R.FIXTURE[:3]
    Xp, sp, _ = R.planted_chain(*R.FIXTURE)
    assert np.array_equal(Xp, X) and np.array_equal(sp, s)  # the tool and the restatement draw the same codes
    alpha = float(g["alphas"][a])
    M = R.mstep(X, G.one_hot(s, K), alpha)
    b = R.sklearn_bounds(X, s, K, alpha)
    flp = g[f"feature_log_prob_{a}"]
    with np.errstate(divide="ignore"):
        neg = np.log(1 - np.exp(flp))                       # BernoulliNB's own form
    lp, lognorm, resp, label = R.estep(X, M["logt"], M["logf"], M["logw"])
    w = [R.within(M["logt"], flp, b["d_t"], "log theta"), R.within(M["logf"], neg, b["d_f"], "log(1 - theta)"),
         R.within(M["logw"], g[f"class_log_prior_{a}"], b["d_w"], "log w"), R.within(lp, g[f"joint_{a}"], b["b_lp"], "lp"),
         R.within(resp, g[f"predict_proba_{a}"], b["b_r"], "resp")]
    print(f"alpha = {alpha}: worst |difference|/bound log theta, log(1 - theta), log w, lp, resp = "
          + ", ".join(f"{x:.3g}" for x in w) + f"; the largest bounds {b['d_t'].max():.2g}, {b['d_f'].max():.2g}, "
          f"{b['d_w'].max():.2g}, {b['b_lp'].max():.2g}, {b['b_r'].max():.2g}")
    assert np.array_equal(label, np.argmax(g[f"joint_{a}"], axis=1))
    assert max(b["d_t"].max(), b["d_f"].max(), b["d_w"].max()) < 1e-13 and b["b_lp"].max() < 1e-11
    assert R.rejects(lp + 1e-11, g[f"joint_{a}"], b["b_lp"])


# ---- the mixture as a hidden Markov model ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["fixture", "hundred_bits"])
def test_mixture_identity(name):
    """pi and every row of A equal to the mixture's weights: ll_t is the mixture's lognorm and gamma its responsibilities"""
    X, s, start, K = R.case(name)
    M = R.mstep(X, G.one_hot(start, K), 1.0)
    w = M["weights"]
    A = np.tile(w, (K, 1))
    lb, m, e = R.emit(X, M["logt"], M["logf"])
    alpha, ll, sa = H.forward(e, m, w, A)
    beta, sb = H.backward(e, A)
    gamma = H.posterior(alpha, beta, e, A)[0]
    lp, lognorm, resp, _ = R.estep(X, M["logt"], M["logf"], M["logw"])
    rec = H.recurrence_bounds(e, m, w, A)
    eb = R.estep_bounds(X, M["logt"], M["logf"], M["logw"])
    # both are within their bounds of the exact value for the tables and w as given; log w and w differ by log's 4 u |log w|
    tol = rec["b_ll"] + eb["b_ln"] + 4 * R.U * np.abs(M["logw"]).max() + 2 * K * R.U
    d = np.abs(ll - lognorm)
    dg = float(np.abs(gamma - resp).max())
    print(f"{name}: |ll_t - lognorm| / bound <= {float((d / tol).max()):.3g}, |gamma - responsibilities| <= {dg:.3g}")
    assert np.all(d <= tol) and dg <= 1e-12 and sa[0] == sb[0] == 0


# ---- planted chains and the measured gates ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(R.PLANTED) + ["fixture"])
def test_planted_chains(name):
    X, s, start, K = R.case(name)
    mix, mix_ld, mix_gates = R.fitted(name, "bmm")
    hm, hm_ld, hm_gates = R.fitted(name, "bhmm")
    a0, a_mix, a_hmm = H.ari(s, start), H.ari(s, mix["labels"]), H.ari(s, hm["path"])
    closest = float(np.abs(hm["changes"] - 1e-3).min())
    closest_mix = float(np.abs(mix["changes"] - 1e-3).min())
    print(f"{name} {R.PLANTED.get(name, R.FIXTURE)}: k-means ARI {a0:.3f}, mixture ARI {a_mix:.3f} ({mix['n_iter']} iterations, "
          f"closest stop decision {closest_mix:.2e} from tol), Viterbi ARI {a_hmm:.3f} ({hm['n_iter']} iterations, {hm['why']}, "
          f"closest {closest:.2e})")
    print("  mixture, f64 - long double: " + ", ".join(f"{k} {v:.3g}" for k, v in mix_gates.items()))
    print("  hidden Markov model, f64 - long double: " + ", ".join(f"{k} {v:.3g}" for k, v in hm_gates.items()))
    assert a_hmm >= 0.85 and a_hmm >= a0
    if name == "nine_states":
        assert a0 <= 0.5
    assert hm["converged"] and mix["converged"] and closest > 1e-4
    # the mixture's decisions come closer to tol (8.4e-6 on nine_states); what matters is that no decision can turn inside the
    # device's gate of the lower bound
    assert closest_mix > 1e3 * R.GATE_FACTOR * mix_gates["lower_bounds"] and closest_mix > 1e-9
    assert not R.outside(mix_gates, mix_gates, R.BMM_QUANTITIES, "labels")
    assert not R.outside(hm_gates, hm_gates, R.BHMM_QUANTITIES, "path")
    assert all(R.GATE_FACTOR * mix_gates[q] < 1e-9 for q in R.BMM_QUANTITIES)
    assert all(R.GATE_FACTOR * hm_gates[q] < 1e-9 for q in R.BHMM_QUANTITIES)
    assert all(mix_gates[q] > 0 for q in R.BMM_QUANTITIES), "a gate of zero would ask for bit equality"
    assert all(hm_gates[q] > 0 for q in R.BHMM_QUANTITIES), "a gate of zero would ask for bit equality"
    blocked = R.bhmm_fit(X, start, K, R=H.BLOCK_ROWS)       # the device's default order stays inside the gate as well
    assert not R.outside(R.differences(blocked, hm, R.BHMM_QUANTITIES, "path"), hm_gates, R.BHMM_QUANTITIES, "path")
    wrong = R.bhmm_fit(X, start, K, prior=1.0 + 1e-9)       # the gates are no blank cheque
    assert "probs" in R.outside(R.differences(wrong, hm, R.BHMM_QUANTITIES, "path"), hm_gates, R.BHMM_QUANTITIES, "path")


def test_parameter_counts():
    assert R.bmm_n_parameters(9, 25) == 9 * 25 + 8 == sfv.bernoulli.bmm_n_parameters(9, 25)
    assert R.bhmm_n_parameters(9, 25) == 8 + 72 + 225 == sfv.bernoulli.bhmm_n_parameters(9, 25)
    assert sfv.bernoulli.bmm_n_parameters(9, 25) != sfv.mixture.n_parameters(9, 25)
    assert sfv.bernoulli.bhmm_n_parameters(9, 25) != sfv.hmm_model.n_parameters(9, 25)


# ---- the host side of the package -------------------------------------------------------------------------------------------

NEW = ("rbvae_bern_ok", "rbvae_bern_chunk_components", "rbvae_bern_ws_bytes", "rbvae_bern_pack", "rbvae_bern_emit",
       "rbvae_bern_estep", "rbvae_bern_mstep")


def test_header_and_library():
    protos = sfv._lib.parse_header()
    raw = ctypes.CDLL(sfv._lib.LIB_PATH)
    for name in NEW:
        assert name in protos and hasattr(raw, name), name
    assert [len(protos[n][1]) for n in NEW] == [3, 1, 3, 5, 11, 12, 14]
    q = sfv._lib.query
    assert q("rbvae_version") >= 106
    for shape in ((12298, 50, 17), (1 << 20, 128, 64), (1, 1, 1), (2, 1, 2), (256, 128, 256), (255, 2, 256), (300, 129, 4),
                  (300, 4, 257), (300, 0, 4), (300, 4, 0), ((1 << 20) + 1, 2, 2), (3, 2, 4), (1 << 20, 2, 65)):
        assert q("rbvae_bern_ok", *shape) == int(R.ok(*shape)) == q("rbvae_gmm_ok", *shape), shape
        assert q("rbvae_bern_ws_bytes", *shape) == (R.ws_bytes(*shape) if R.ok(*shape) else 0)
    for L in (1, 2, 25, 33, 100, 128):
        assert q("rbvae_bern_chunk_components", L) == R.chunk_components(L) == 2048 // L
    assert q("rbvae_bern_chunk_components", 0) == 0 and q("rbvae_bern_chunk_components", 129) == 0
    assert R.chunk_components(128) == 16


def test_refused_on_the_host():
    X = torch.zeros((8, 4))
    mix = sfv.BMMResult(*([None] * 10))
    mix.probs = torch.zeros((2, 4), dtype=torch.float64)
    chain = sfv.BHMMResult(*([None] * 13))
    chain.probs = torch.zeros((2, 4), dtype=torch.float64)
    for call in (lambda: sfv.bmm(X, 2), lambda: sfv.bhmm(X, 2), lambda: sfv.pack_codes(X), lambda: sfv.bmm_select(X, [2, 3]),
                 lambda: sfv.bhmm_select(X, [2]), lambda: sfv.bmm_predict(mix, X), lambda: sfv.bmm_score(mix, X),
                 lambda: sfv.bhmm_predict(chain, X), lambda: sfv.bhmm_predict_proba(chain, X), lambda: sfv.bhmm_score(chain, X),
                 lambda: sfv.latent_code_models(None, torch.zeros((2, 3, 8, 8)), [0, 1], [1])):
        with pytest.raises(ValueError, match="GPU"):
            call()
    with pytest.raises(ValueError, match="tensor"):
        sfv.bmm(np.zeros((8, 4), dtype=np.float32), 2)
    for prior in (0.0, -1.0, float("nan")):
        for fit in (sfv.bmm, sfv.bhmm):
            with pytest.raises(ValueError, match="prior"):
                fit(X, 2, prior=prior)
    for fit in (sfv.bmm, sfv.bhmm):
        with pytest.raises(ValueError, match="init must be"):
            fit(X, 2, init="random")
        with pytest.raises(ValueError, match="max_iter"):
            fit(X, 2, max_iter=0)
        with pytest.raises(ValueError, match="tol"):
            fit(X, 2, tol=-1.0)
    for fn in (sfv.bmm_predict, sfv.bmm_predict_proba, sfv.bmm_score_samples, sfv.bmm_bic):
        with pytest.raises(ValueError, match="5 columns, the fit 4"):
            fn(mix, torch.zeros((8, 5)))
    for fn in (sfv.bhmm_predict, sfv.bhmm_predict_proba, sfv.bhmm_score_samples, sfv.bhmm_aic):
        with pytest.raises(ValueError, match="5 columns, the fit 4"):
            fn(chain, torch.zeros((8, 5)))
    for fn, match in ((lambda: sfv.bmm(X, 9), "K=9"), (lambda: sfv.bmm(torch.zeros((300, 129)), 2), "L=129"),
                      (lambda: sfv.bmm(torch.zeros((300, 4)), 257), "K=257"), (lambda: sfv.bmm(X, 0), "K=0"),
                      (lambda: sfv.bhmm(torch.zeros((300, 4)), 65), "K=65"), (lambda: sfv.bhmm(torch.zeros((1, 4)), 1), "N=1"),
                      (lambda: sfv.pack_codes(torch.zeros((4, 129))), "L=129"),
                      (lambda: sfv.bhmm_predict(chain, torch.zeros((1, 4))), "N=1")):
        with pytest.raises(ValueError, match=match):
            fn()
    with pytest.raises(ValueError, match="ks is empty"):
        sfv.bmm_select(X, [])
    assert sfv.bernoulli.bmm is sfv.bmm and sfv.bernoulli.MAX_COMPONENTS == 256 and sfv.bernoulli.MAX_STATES == 64
    assert sfv.bernoulli.ENQUEUE == 8
