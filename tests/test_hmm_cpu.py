"""CPU: tests/_hmm_ref.py (the f64 restatement the GPU tests compare the hidden-Markov-model kernels and hmm.py with) against
its long double twin inside the bounds it derives, against the enumeration of all paths on tiny cases, and against
scikit-learn's mixture through tests/golden/gmm.npz (an HMM whose pi and rows of A all equal the mixture's weights is that
mixture); each check of the GPU tests against the named defect it has to reject; and the host side of hmm.py.

Measured here: the f64 restatement is at most 0.15 of its long double bounds, sequentially and blocked; the mixture identity
holds within 2.6e-13 (K = 17) and 1.3e-11 (K = 32, seed 42: scikit-learn's own cancellation) for ll_t and 1e-12 for gamma.
The planted chains: k-means ARI 0.66 and 0.60, Viterbi ARI 0.97 and 0.93 after 6 and 9 iterations, no stop decision within
4e-4 of tol, f64 and long double paths equal.  The recorded f64 / long double differences (the device gates are 64 times
these) are printed by test_planted_chains and quoted in DESIGN.md."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _gmm_ref as G
import _hmm_ref as R
import sfv_amd as sfv

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(os.path.join(HERE, "golden", "gmm.npz")))
    g["X"] = np.load(os.path.join(HERE, "golden", "latent_scores.npz"))["X"]
    return g


def _passes(e, m, pi, A, Rr=None, defect=None):
    al, ll, sa = R.forward(e, m, pi, A, defect, R=Rr)
    be, sb = R.backward(e, A, defect, R=Rr)
    return al, be, ll, sa, sb


# ---- the restatement against long double and all paths ----------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["dense", "sticky", "left_to_right"])
@pytest.mark.parametrize("N,K,Rr", [(2, 1, None), (2, 2, 1), (65, 2, 7), (129, 17, 64), (129, 17, 1), (300, 5, 7), (64, 64, None)])
def test_recursions_within_long_double_bounds(N, K, Rr, kind):
    e, m, pi, A = R.random_chain(N, K, 3, kind)
    ref = R.recurrence_bounds(e, m, pi, A, Rr)
    al, be, ll, sa, sb = _passes(e, m, pi, A, Rr)
    w = [R.within(al, ref["alpha"], ref["b_alpha"], "alpha"), R.within(be, ref["beta"], ref["b_beta"], "beta"),
         R.within(ll, ref["ll"], ref["b_ll"], "ll")]
    post = R.posterior_bounds(ref["alpha"], ref["beta"], e, A, ref["rho_a"], ref["rho_b"])
    gamma, Xi, A_new, pi_new, sp = R.posterior(al, be, e, A)
    w += [R.within(gamma, post["gamma"], post["b_gamma"], "gamma"), R.within(Xi, post["xi"], post["b_xi"], "Xi"),
          R.within(A_new, post["A_new"], post["b_A_new"], "A_new")]
    assert np.array_equal(pi_new, gamma[0]) and sa[0] == sb[0] == sp[0] == 0 and sa[1] == R.NO_ROW
    assert np.abs(gamma.astype(R.LD).sum(axis=1) - 1).max() <= post["b_gamma_sum"]
    assert abs(float(Xi.astype(R.LD).sum()) - (N - 1)) <= post["b_xi_sum"]
    assert np.abs(A_new.astype(R.LD).sum(axis=1) - 1).max() <= 2 * K * R.U + 2 * post["b_xi"].max() / max(Xi.sum(axis=1).min(), 1e-300)
    print(f"({N}, {K}, block_rows {Rr}, {kind}): worst |err|/bound alpha, beta, ll, gamma, Xi, A_new = " + ", ".join(f"{x:.3g}" for x in w))
    assert R.rejects(al * (1 + 1e-9), ref["alpha"], ref["b_alpha"])     # the bounds are no blank cheque


@pytest.mark.parametrize("kind", ["dense", "left_to_right"])
@pytest.mark.parametrize("N,K", [(6, 2), (8, 3), (3, 3)])
def test_equals_all_paths(N, K, kind):
    e, m, pi, A = R.random_chain(N, K, 1, kind)
    if kind == "left_to_right":
        pi = np.eye(K)[0] * 1.0                             # the chain starts in state 0: most paths have probability 0
        assert (A == 0).sum() == K * K - (2 * K - 1)
    logb = np.log(e) + m[:, None]
    ll, g, Xi, path, margin = R.brute(logb, pi, A)
    al, be, llt, sa, sb = _passes(e, m, pi, A)
    gamma, X2, _, _, sp = R.posterior(al, be, e, A)
    assert abs(float(llt.astype(R.LD).sum()) - ll) <= 1e-13 * max(1.0, abs(ll))
    assert np.abs(gamma - g).max() <= 1e-13 and np.abs(X2 - Xi).max() <= 1e-13
    vp, score, _ = R.viterbi(logb, R.log0(pi), R.log0(A))
    assert margin > 1e-6 and np.array_equal(vp, path)
    for Rr in (1, 2):                                        # the blocked order, on the same tiny cases
        alb, beb, llb, _, _ = _passes(e, m, pi, A, Rr)
        assert np.abs(alb - al).max() <= 1e-13 and np.abs(beb - be).max() <= 1e-13 and np.abs(llb - llt).max() <= 1e-13


def _mixture_as_hmm(gold, K, seed):
    t = f"{K}_{seed}"
    w, mu, var = gold["weights_" + t], gold["means_" + t], gold["covars_" + t]
    return w, np.tile(w, (K, 1)), mu, 1.0 / np.sqrt(var)


@pytest.mark.parametrize("K,seed", [(2, 0), (8, 42), (17, 42), (32, 42)])
def test_mixture_identity(gold, K, seed):
    """pi and every row of A equal to the mixture's weights: ll_t is scikit-learn's score_samples and gamma its responsibilities"""
    w, A, mu, s = _mixture_as_hmm(gold, K, seed)
    lb, m, e = R.emit(gold["X"], mu, s)
    al, be, ll, sa, sb = _passes(e, m, w, A)
    gamma = R.posterior(al, be, e, A)[0]
    d = float(np.abs(ll - gold[f"score_samples_{K}_{seed}"]).max())
    logc = (np.log(w) + np.log(s).sum(axis=1)) - 0.5 * 50 * R.LOG_2PI
    resp = G.estep(gold["X"], mu, s, logc)[2]
    dg = float(np.abs(gamma - resp).max())
    print(f"K = {K}, seed {seed}: |ll_t - score_samples| <= {d:.3g}, |gamma - responsibilities| <= {dg:.3g}")
    assert d <= G.GATES["score_samples"] and dg <= 1e-10 and sa[0] == sb[0] == 0
    if (K, seed) == (32, 42):                               # the shift by the row maximum is necessary here
        span = float((lb.max(axis=1) - lb.min(axis=1)).max())
        zeros = float((e == 0).mean())
        print(f"  one row's lb spans {span:.3g} nats; {100 * zeros:.1f} % of e are exactly 0")
        assert span > 2e5 and 0.05 < zeros < 0.15


@pytest.mark.parametrize("N,Ld,K", [(1, 1, 1), (257, 128, 17), (65, 2, 64)])
def test_emit_within_bounds(N, Ld, K):
    N = max(N, K, 2)
    X, means, prec, _, _, _ = G.params_case(N, Ld, K)
    ref = R.emit_bounds(X, means, prec)
    lb, m, e = R.emit(X, means, prec)
    w = [R.within(lb, ref["lb"], ref["b_lb"], "lb"), R.within(m, ref["m"], ref["b_m"], "m"), R.within(e, ref["e"], ref["b_e"], "e")]
    print(f"emit ({N}, {Ld}, {K}): worst |err|/bound lb, m, e = " + ", ".join(f"{x:.3g}" for x in w))
    assert (e.max(axis=1) == 1.0).all()
    assert R.rejects(lb + 1e-9, ref["lb"], ref["b_lb"])


# ---- planted chains and the measured gates ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(R.PLANTED))
def test_planted_chains(name):
    X, z, start, f64, ld, gates = R.planted(name)
    a0, a1 = R.ari(z, start), R.ari(z, f64["path"])
    closest = float(np.abs(f64["changes"] - 1e-3).min())
    print(f"{name}: k-means ARI {a0:.3f}, Viterbi ARI {a1:.3f}, {f64['n_iter']} iterations ({f64['why']}), closest stop decision "
          f"{closest:.2e} from tol; f64 - long double: " + ", ".join(f"{k} {v:.3g}" for k, v in gates.items()))
    assert a0 <= 0.7 and a1 >= 0.9
    assert f64["converged"] and f64["n_iter"] == ld["n_iter"] and gates["path"] <= 0.01
    assert closest > 1e-5 and all(R.GATE_FACTOR * gates[q] < 1e-9 for q in R.QUANTITIES)
    assert all(gates[q] > 0 for q in R.QUANTITIES if q != "pi"), "a gate of zero would ask for bit equality"
    blocked = R.fit(X, start, 4, R=R.BLOCK_ROWS)            # the device's default order stays inside the gate as well
    assert not R.outside(R.differences(blocked, f64), gates)


def test_fixture_latents_fit(gold):
    for K, seed in ((2, 0), (8, 42)):
        init = gold[f"init_{K}_{seed}"]
        f64, ld = R.fit(gold["X"], init, K), R.fit(gold["X"], init, K, dtype=R.LD)
        d = R.differences(f64, ld)
        closest = float(np.abs(f64["changes"] - 1e-3).min())
        print(f"latents, K = {K}, seed {seed}: {f64['n_iter']} iterations, closest stop decision {closest:.2e}; f64 - long double: "
              + ", ".join(f"{k} {v:.3g}" for k, v in d.items()))
        assert f64["converged"] and d["n_iter"] == 0 and d["path"] <= 0.01 and closest > 1e-5


# ---- the checks reject the named defects ------------------------------------------------------------------------------------

def test_defect_list():
    assert R.DEFECTS == ("block_boundary_reset", "transfer_scale_dropped", "beta_uses_e_t", "xi_without_emission",
                         "A_column_normalised", "pi_not_updated", "loglik_without_rowmax", "viterbi_sum_for_max",
                         "viterbi_tie_high", "bic_param_count_gmm")


@pytest.mark.parametrize("defect", ["block_boundary_reset", "transfer_scale_dropped", "beta_uses_e_t", "loglik_without_rowmax"])
def test_recursion_defects_rejected(defect):
    e, m, pi, A = R.random_chain(300, 5, 3, "sticky")       # a sticky overlapping chain: the past matters at a block's edge
    ref = R.recurrence_bounds(e, m, pi, A, 7)
    al, be, ll, _, _ = _passes(e, m, pi, A, 7, defect)
    hit = {"alpha": R.rejects(al, ref["alpha"], ref["b_alpha"]), "beta": R.rejects(be, ref["beta"], ref["b_beta"]),
           "ll": R.rejects(ll, ref["ll"], ref["b_ll"])}
    print(f"{defect}: outside their bounds: {[k for k, v in hit.items() if v]}")
    want = {"block_boundary_reset": ("alpha", "beta"), "transfer_scale_dropped": ("alpha", "beta"), "beta_uses_e_t": ("beta",),
            "loglik_without_rowmax": ("ll",)}[defect]
    assert all(hit[k] for k in want)


@pytest.mark.parametrize("defect", ["xi_without_emission", "A_column_normalised"])
def test_posterior_defects_rejected(defect):
    e, m, pi, A = R.random_chain(300, 5, 3, "sticky")
    ref = R.recurrence_bounds(e, m, pi, A)
    post = R.posterior_bounds(ref["alpha"], ref["beta"], e, A, ref["rho_a"], ref["rho_b"])
    al, be, _, _, _ = _passes(e, m, pi, A)
    _, Xi, A_new, _, _ = R.posterior(al, be, e, A, defect)
    assert R.rejects(A_new, post["A_new"], post["b_A_new"])
    if defect == "xi_without_emission":
        assert R.rejects(Xi, post["xi"], post["b_xi"])
    else:
        assert np.abs(A_new.sum(axis=1) - 1).max() > 1e-3   # its rows no longer add to 1


@pytest.mark.parametrize("defect", ["block_boundary_reset", "beta_uses_e_t", "xi_without_emission", "A_column_normalised",
                                    "pi_not_updated", "loglik_without_rowmax"])
def test_fit_defects_rejected_at_the_measured_gate(defect):
    X, z, start, f64, ld, gates = R.planted("sticky_a")
    wrong = R.fit(X, start, 4, defect=defect, R=R.BLOCK_ROWS if defect == "block_boundary_reset" else None)
    bad = R.outside(R.differences(wrong, f64), gates)
    print(f"{defect}: outside the gate: {bad}")
    assert {"pi_not_updated": "pi", "loglik_without_rowmax": "log_likelihoods"}.get(defect, "A") in bad


def test_viterbi_defects_rejected():
    e, m, pi, A = R.random_chain(8, 3, 1, "dense")
    logb = np.log(e) + m[:, None]
    path, score, _ = R.viterbi(logb, R.log0(pi), R.log0(A))
    _, score2, _ = R.viterbi(logb, R.log0(pi), R.log0(A), "viterbi_sum_for_max")
    best = R.brute(logb, pi, A)[3]
    joint = np.log(pi[best[0]]) + logb[0, best[0]] + sum(np.log(A[best[t - 1], best[t]]) + logb[t, best[t]] for t in range(1, 8))
    assert abs(score - joint) <= 1e-13 * abs(joint) and abs(score2 - joint) > 1e-3       # the sum gives the likelihood instead
    # exact ties: two states given twice
    lb2 = np.concatenate([logb[:, :2], logb[:, :2]], axis=1)
    A2, pi2 = np.full((4, 4), 0.25), np.full(4, 0.25)
    low = R.viterbi(lb2, R.log0(pi2), R.log0(A2))[0]
    high = R.viterbi(lb2, R.log0(pi2), R.log0(A2), "viterbi_tie_high")[0]
    assert np.all(low < 2) and np.array_equal(high, low + 2)


def test_bic_param_count_rejected():
    assert R.n_parameters(17, 50) == 16 + 17 * 16 + 1700 == sfv.hmm_model.n_parameters(17, 50)
    assert R.n_parameters(17, 50, "bic_param_count_gmm") == G.n_parameters(17, 50) != R.n_parameters(17, 50)
    right, wrong = R.criteria(-1.25, 1500, 4, 3), R.criteria(-1.25, 1500, 4, 3, "bic_param_count_gmm")
    assert abs(right[0] / wrong[0] - 1) > 1e-3 and abs(sfv.hmm_model._criteria(-1.25, 1500, 4, 3)[0] / right[0] - 1) <= 4 * R.U
    assert abs(sfv.hmm_model._criteria(-1.25, 1500, 4, 3)[1] / right[1] - 1) <= 4 * R.U


# ---- the host side of the package -------------------------------------------------------------------------------------------

NEW = ("rbvae_hmm_ok", "rbvae_hmm_block_rows", "rbvae_hmm_ws_bytes", "rbvae_hmm_emit", "rbvae_hmm_forward", "rbvae_hmm_backward",
       "rbvae_hmm_posterior", "rbvae_hmm_viterbi")


def test_header_and_library():
    protos = sfv._lib.parse_header()
    raw = ctypes.CDLL(sfv._lib.LIB_PATH)
    for name in NEW:
        assert name in protos and hasattr(raw, name), name
    assert [len(protos[n][1]) for n in NEW] == [3, 0, 3, 11, 14, 11, 15, 10]
    q = sfv._lib.query
    assert q("rbvae_version") >= 105 and q("rbvae_hmm_block_rows") == R.BLOCK_ROWS == 64
    for shape in ((12298, 50, 17), (1 << 20, 128, 64), (2, 1, 1), (2, 1, 2), (64, 128, 64), (1, 1, 1), (63, 2, 64), (300, 129, 4),
                  (300, 4, 65), (300, 0, 4), (300, 4, 0), ((1 << 20) + 1, 2, 2), (3, 2, 4)):
        assert q("rbvae_hmm_ok", *shape) == int(R.ok(*shape)), shape
        if R.ok(*shape):                                    # a subset of the mixture's shapes: the posterior goes to its M-step
            assert q("rbvae_gmm_ok", *shape) == 1
    assert q("rbvae_hmm_ok", 1, 1, 1) == 0 and q("rbvae_hmm_ok", 1 << 20, 128, 64) == 1 and q("rbvae_hmm_ok", (1 << 20), 2, 65) == 0
    for N, K, Rr in ((12298, 17, 64), (4097, 64, 1), (2, 1, 64), (65537, 2, 7), (1 << 20, 64, 64)):
        assert q("rbvae_hmm_ws_bytes", N, K, Rr) == R.ws_bytes(N, K, Rr)
    assert q("rbvae_hmm_ws_bytes", 300, 65, 64) == 0 and q("rbvae_hmm_ws_bytes", 300, 4, 0) == 0


def test_cpu_inputs_raise():
    X = torch.zeros((8, 4))
    lb = torch.zeros((8, 2), dtype=torch.float64)
    fit = sfv.HMMResult(*([None] * 13))
    for call in (lambda: sfv.hmm(X, 2), lambda: sfv.hmm_select(X, [2, 3]), lambda: sfv.hmm_forward_backward(lb, [0.5, 0.5], np.eye(2)),
                 lambda: sfv.hmm_viterbi(lb, [0.5, 0.5], np.eye(2)),
                 lambda: sfv.latent_hmm(None, torch.zeros((2, 3, 8, 8)), [0, 1], [1])):
        with pytest.raises(ValueError, match="GPU"):
            call()
    with pytest.raises(ValueError, match="tensor"):
        sfv.hmm(np.zeros((8, 4), dtype=np.float32), 2)
    with pytest.raises(ValueError, match="ks is empty"):
        sfv.hmm_select(X, [])
    assert fit.means is None and sfv.hmm_model.hmm is sfv.hmm and sfv.hmm_model.MAX_STATES == 64 and sfv.hmm_model.ENQUEUE == 8
    assert sfv.hmm_model.change_points(np.array([0, 0, 1, 1, 0])) == [2, 4] and sfv.hmm_model.change_points(np.array([3])) == []
