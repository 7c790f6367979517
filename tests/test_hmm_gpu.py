"""GPU: the hidden-Markov-model kernels (csrc/hmm.hip) inside sentinel guard bands (tests/_bounds.py's buffers) against the
long double references and bounds of tests/_hmm_ref.py -- the emissions, alpha, beta, ll, gamma, Xi and A_new element-wise, the
plain recursion (block_rows >= N) and Viterbi bit for bit against the f64 restatement -- and hmm.py end to end against the
restatement's fit at the measured gates of tests/test_hmm_cpu.py (64 times the f64 / long double difference of each quantity).

rbvae_hmm_ok refuses N = 1, so the smallest emission case is 2 x 1 x 1 and 1 x 1 x 1 is asserted to be refused.  Every test
prints its worst |error| / bound; DESIGN.md section 7 quotes them.

Measured on one MI355X: the plain recursion equals the restatement bit for bit on all 29 (K, N) cases; blocked at block_rows
64, 1 and 7 alpha is at most 0.064, beta 0.105 and ll 0.122 of their bounds; lb 0.35 and e 0.17 (300 x 2 x 64); gamma 0.65
(65 537 rows), Xi 0.012, A_new 0.006; Viterbi equal bit for bit, backpointers included.  On the planted chains and the fixture's
latents n_iter, converged and every row of the path equal the restatement's and every quantity is at least five times inside
its gate.  The 58 tests take about 11 s together; the largest recursion cases (4097 rows, 63 and 64 states) 1.3 s each.
"""
import functools
import os

import numpy as np
import pytest
import torch

import _bounds as B
import _gmm_ref as Gm
import _hmm_ref as R
import sfv_amd as sfv

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GUARD = 4096
B.SENTINEL.setdefault(torch.float64, (torch.int64, 0x7FF8DEADDEADBEEF))
B.SENTINEL.setdefault(torch.int32, (torch.int32, -0x21524111))
B.SENTINEL.setdefault(torch.uint8, (torch.uint8, 0xA5))
call, query = sfv._lib.call, sfv._lib.query
F64, I32, U8 = torch.float64, torch.int32, torch.uint8


def G(dtype, *shape):
    g = B.GuardedFlat(int(np.prod(shape)), dtype, guard=GUARD)
    g.t = g.view.view(*shape)
    return g


def out(g, what):
    B.assert_guards(g, what)
    return g.t.cpu().numpy()


def untouched(g, what):
    B.assert_guards_where(g, torch.zeros(g.rows, dtype=torch.bool), what)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def _state(*v):
    return torch.tensor(list(v) or [0, 0, 0, 0], dtype=torch.int32, device="cuda")


def _status():
    g = G(I32, 2)
    g.t.copy_(torch.tensor([0, R.NO_ROW], dtype=torch.int32))
    return g


def bits(a):
    return np.asarray(a).view(np.int64) if np.asarray(a).dtype == np.float64 else np.asarray(a)


def _ws(N, K, Rr):
    n = query("rbvae_hmm_ws_bytes", N, K, Rr)
    assert n == R.ws_bytes(N, K, Rr)
    return G(F64, n // 8), n


def _ws_guards(ws, what):
    """a workspace is used in part: whatever was written lies inside it"""
    B.assert_guards_where(ws, (ws.view.view(torch.int64) != B.SENTINEL[F64][1]).cpu(), what)


# ---- emissions ---------------------------------------------------------------------------------------------------------------

def _emit(X, means, prec, state=None):
    N, Ld = X.shape
    K = len(means)
    logb, rowmax, e = G(F64, K, N), G(F64, N), G(F64, N, K)
    call("rbvae_hmm_emit", _dev(X), N, Ld, _dev(means), _dev(prec), K, logb.t, rowmax.t, e.t, state)
    what = f"({N}, {Ld}, {K})"
    return out(logb, "logb " + what).T, out(rowmax, "rowmax " + what), out(e, "e " + what)


def _check_emit(X, means, prec, what):
    ref = R.emit_bounds(X, means, prec)
    lb, m, e = _emit(X, means, prec)
    w = [R.within(lb, ref["lb"], ref["b_lb"], "lb " + what), R.within(m, ref["m"], ref["b_m"], "rowmax " + what),
         R.within(e, ref["e"], ref["b_e"], "e " + what)]
    assert np.array_equal(m, lb.max(axis=1)) and (e.max(axis=1) == 1.0).all()
    print(f"emit {what}: worst |err|/bound lb {w[0]:.3g}, rowmax {w[1]:.3g}, e {w[2]:.3g}")
    return lb, m, e


@pytest.mark.parametrize("N,Ld,K", [(2, 1, 1), (257, 128, 17), (300, 2, 64)])
def test_emit(N, Ld, K):
    X, means, prec, _, _, _ = Gm.params_case(N, Ld, K)
    lb, m, e = _check_emit(X, means, prec, f"({N}, {Ld}, {K})")
    lb2, m2, e2 = _emit(X, means, prec, _state())
    assert np.array_equal(bits(lb), bits(lb2)) and np.array_equal(bits(m), bits(m2)) and np.array_equal(bits(e), bits(e2))
    assert query("rbvae_hmm_ok", 1, 1, 1) == 0              # the limits refuse one row
    done = _state(1, 3, 1, 0)
    gs = [G(F64, K, N), G(F64, N), G(F64, N, K)]
    call("rbvae_hmm_emit", _dev(X), N, Ld, _dev(means), _dev(prec), K, gs[0].t, gs[1].t, gs[2].t, done)
    for g, name in zip(gs, ("logb", "rowmax", "e")):
        untouched(g, name + " behind done")


def test_emit_fixture_far_rows():
    """the K = 32, seed 42 parameters of tests/golden/gmm.npz: a row's lb spans 2.45e5 nats, and e is exactly 0 where the
    restatement's is"""
    g = np.load(os.path.join(HERE, "golden", "gmm.npz"))
    X = np.load(os.path.join(HERE, "golden", "latent_scores.npz"))["X"]
    means, prec = g["means_32_42"], 1.0 / np.sqrt(g["covars_32_42"])
    lb, m, e = _check_emit(X, means, prec, "fixture K = 32, seed 42")
    ref = R.emit(X, means, prec)
    assert float((lb.max(axis=1) - lb.min(axis=1)).max()) > 2e5
    assert np.array_equal(e == 0, ref[2] == 0) and 0.05 < float((e == 0).mean()) < 0.15


# ---- forward and backward given e ----------------------------------------------------------------------------------------------

def _forward(e, m, pi, A, Rr, state=None):
    N, K = e.shape
    alpha, ll, st = G(F64, N, K), G(F64, N), _status()
    ws, nb = _ws(N, K, Rr)
    call("rbvae_hmm_forward", _dev(e), _dev(m), N, K, _dev(pi), _dev(A), Rr, alpha.t, ll.t, st.t, ws.t, nb, state)
    what = f"forward ({N}, {K}, block_rows {Rr})"
    _ws_guards(ws, "workspace " + what)
    return out(alpha, "alpha " + what), out(ll, "ll " + what), out(st, "status " + what).tolist()


def _backward(e, A, Rr, state=None):
    N, K = e.shape
    beta, st = G(F64, N, K), _status()
    ws, nb = _ws(N, K, Rr)
    call("rbvae_hmm_backward", _dev(e), N, K, _dev(A), Rr, beta.t, st.t, ws.t, nb, state)
    what = f"backward ({N}, {K}, block_rows {Rr})"
    _ws_guards(ws, "workspace " + what)
    return out(beta, "beta " + what), out(st, "status " + what).tolist()


def _check_recursions(e, m, pi, A, what, block_rows=(R.BLOCK_ROWS, 1, 7)):
    N, K = e.shape
    seq_a, seq_ll, _ = R.forward(e, m, pi, A)
    seq_b, _ = R.backward(e, A)
    al, ll, sa = _forward(e, m, pi, A, N)
    be, sb = _backward(e, A, N + 5)
    assert np.array_equal(bits(al), bits(seq_a)) and np.array_equal(bits(be), bits(seq_b)), "the plain recursion is the restatement's"
    assert sa == sb == [0, R.NO_ROW]
    ld = R.ld_passes(e, m, pi, A)
    ref1 = R.recurrence_bounds(e, m, pi, A, ld=ld)
    worst = [R.within(ll, ref1["ll"], ref1["b_ll"], "ll " + what)]
    for Rr in block_rows:
        ref = R.recurrence_bounds(e, m, pi, A, Rr, ld=ld)
        al, ll, sa = _forward(e, m, pi, A, Rr)
        be, sb = _backward(e, A, Rr)
        assert sa == sb == [0, R.NO_ROW]
        worst += [R.within(al, ref["alpha"], ref["b_alpha"], f"alpha {what} block_rows {Rr}"),
                  R.within(be, ref["beta"], ref["b_beta"], f"beta {what} block_rows {Rr}"),
                  R.within(ll, ref["ll"], ref["b_ll"], f"ll {what} block_rows {Rr}")]
    print(f"recursions {what}: plain recursion bit-equal; worst |err|/bound (ll plain; alpha, beta, ll per block_rows "
          f"{block_rows}) " + ", ".join(f"{x:.3g}" for x in worst))


KN = sorted({(K, N) for K in (1, 2, 17, 63, 64) for N in (2, 63, 64, 65, 129, 4097) if N >= max(K, 2)} | {(17, 17), (63, 63)})


@pytest.mark.parametrize("K,N", KN)
def test_recursions(K, N):
    e, m, pi, A = R.random_chain(N, K, 3, "dense")
    _check_recursions(e, m, pi, A, f"({N}, {K})")


@pytest.mark.parametrize("kind", ["sticky", "left_to_right"])
def test_recursions_where_the_past_matters(kind):
    """a sticky overlapping chain and a left-to-right A with zeros: a block that forgot its past (block_boundary_reset) or its
    scales (transfer_scale_dropped) is outside the same bounds"""
    e, m, pi, A = R.random_chain(300, 5, 3, kind)
    _check_recursions(e, m, pi, A, f"(300, 5, {kind})")
    ref = R.recurrence_bounds(e, m, pi, A, 7)
    for defect in ("block_boundary_reset", "transfer_scale_dropped"):
        assert R.rejects(R.forward(e, m, pi, A, defect, R=7)[0], ref["alpha"], ref["b_alpha"])
        assert R.rejects(R.backward(e, A, defect, R=7)[0], ref["beta"], ref["b_beta"])
    al, ll, _ = _forward(e, m, pi, A, 7)
    al2, ll2, _ = _forward(e, m, pi, A, 7)
    assert np.array_equal(bits(al), bits(al2)) and np.array_equal(bits(ll), bits(ll2)), "two runs differ"


@pytest.mark.parametrize("Rr", [100, 7])
def test_impossible_observation(Rr):
    """a row no state can emit: its normaliser is 0, status counts it and names it, and nothing is written out of place"""
    N, K = 65, 5
    e, m, pi, A = R.random_chain(N, K, 4, "dense")
    ef = e.copy()
    ef[N - 1] = 0.0                                         # the last row: one zero normaliser in the forward pass
    al, ll, st = _forward(ef, m, pi, A, Rr)
    assert st == [1, N - 1] == R.forward(ef, m, pi, A, R=Rr)[2] and np.isnan(al[N - 1]).all() and np.isfinite(al[:N - 1]).all()
    eb = e.copy()
    eb[1] = 0.0                                             # row 1: beta_0's normaliser, the last the backward pass takes
    be, st = _backward(eb, A, Rr)
    assert st == [1, 0] == R.backward(eb, A, R=Rr)[1] and np.isnan(be[0]).all() and np.isfinite(be[1:]).all()
    em = e.copy()
    em[40] = 0.0                                            # in the middle: every later row has lost its past
    _, _, st = _forward(em, m, pi, A, Rr)
    assert st == [N - 40, 40] == R.forward(em, m, pi, A, R=Rr)[2]
    _, st = _backward(em, A, Rr)
    assert st == [40, 0] == R.backward(em, A, R=Rr)[1]


# ---- the posterior -----------------------------------------------------------------------------------------------------------

def _posterior(alpha, beta, e, A, state=None):
    N, K = e.shape
    gamma, xi, A_new, pi_new, st = G(F64, K, N), G(F64, K, K), G(F64, K, K), G(F64, K), _status()
    ws, nb = _ws(N, K, R.BLOCK_ROWS)
    call("rbvae_hmm_posterior", _dev(alpha), _dev(beta), _dev(e), N, K, _dev(A), gamma.t, xi.t, A_new.t, pi_new.t, st.t, ws.t,
         nb, state)
    what = f"posterior ({N}, {K})"
    return (out(gamma, "gamma " + what).T, out(xi, "Xi " + what), out(A_new, "A_new " + what), out(pi_new, "pi_new " + what),
            out(st, "status " + what).tolist())


def _rows_of_mass(N, K, seed, empty=None):
    r = np.random.RandomState(seed)
    a = np.exp(2.0 * r.randn(N, K))
    if empty is not None:
        a[:, empty] = 0.0
    return a / a.sum(axis=1, keepdims=True)


@pytest.mark.parametrize("N,K,empty", [(2, 1, None), (300, 5, None), (300, 5, 2), (129, 64, None), (65537, 2, None)])
def test_posterior(N, K, empty):
    """any alpha and beta with rows that add to 1 (the kernel does not ask where they come from): rho = 0 in the bounds"""
    e, _, _, A = R.random_chain(N, K, 5, "dense")
    alpha, beta = _rows_of_mass(N, K, 1, empty), _rows_of_mass(N, K, 2)
    post = R.posterior_bounds(alpha, beta, e, A, np.zeros(N), np.zeros(N))
    gamma, Xi, A_new, pi_new, st = _posterior(alpha, beta, e, A)
    w = [R.within(gamma, post["gamma"], post["b_gamma"], "gamma"), R.within(Xi, post["xi"], post["b_xi"], "Xi"),
         R.within(A_new, post["A_new"], post["b_A_new"], "A_new")]
    assert np.array_equal(bits(pi_new), bits(np.ascontiguousarray(gamma[0]))) and st == [0, R.NO_ROW]
    sg = float(np.abs(gamma.astype(R.LD).sum(axis=1) - 1).max())
    sx = abs(float(Xi.astype(R.LD).sum()) - (N - 1))
    print(f"posterior ({N}, {K}, empty state {empty}): worst |err|/bound gamma {w[0]:.3g}, Xi {w[1]:.3g}, A_new {w[2]:.3g}; "
          f"|sum gamma - 1| <= {sg:.3g} (bound {post['b_gamma_sum']:.3g}), |sum Xi - (N - 1)| = {sx:.3g} (bound {post['b_xi_sum']:.3g})")
    assert sg <= post["b_gamma_sum"] and sx <= post["b_xi_sum"]
    if empty is not None:                                   # a state without mass: a uniform row
        assert np.all(Xi[empty] == 0) and np.all(gamma[:, empty] == 0) and np.abs(A_new[empty] - 1.0 / K).max() <= 2 * R.U
    if N == 65537:
        assert Gm.blocks_rows(N) == (256, 257)              # all 256 row blocks, the last one ragged
    again = _posterior(alpha, beta, e, A)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip((gamma, Xi, A_new), again)), "two runs differ"
    az = alpha.copy()
    az[N // 2] = 0.0                                        # a zero normaliser: g of that row, and Z of it when it has a successor
    st = _posterior(az, beta, e, A)[4]
    assert st == [2 if N // 2 < N - 1 else 1, N // 2]


# ---- Viterbi -----------------------------------------------------------------------------------------------------------------

def _viterbi(logb, lpi, lA, state=None):
    N, K = logb.shape
    back, path, score = G(U8, N, K), G(I32, N), G(F64, 1)
    call("rbvae_hmm_viterbi", _dev(np.ascontiguousarray(logb.T)), N, K, _dev(lpi), _dev(lA), back.t, path.t, score.t, state)
    what = f"viterbi ({N}, {K})"
    return out(path, "path " + what), float(out(score, "score " + what)[0]), out(back, "back " + what)


@pytest.mark.parametrize("N,K,kind", [(2, 1, "dense"), (300, 5, "dense"), (300, 5, "left_to_right"), (129, 64, "dense"),
                                      (4097, 17, "sticky"), (513, 2, "ties")])
def test_viterbi(N, K, kind):
    e, m, pi, A = R.random_chain(N, K, 6, "dense" if kind == "ties" else kind)
    logb = np.log(e) + m[:, None]
    if kind == "left_to_right":
        pi = np.eye(K)[0]                                   # log 0 = -inf in log pi and log A
    if kind == "ties":                                      # two states given twice: every comparison ties exactly
        logb, A, pi, K = np.concatenate([logb, logb], axis=1), np.full((4, 4), 0.25), np.full(4, 0.25), 4
    lpi, lA = R.log0(pi), R.log0(A)
    path, score, back = R.viterbi(logb, lpi, lA)
    got = _viterbi(logb, lpi, lA)
    assert np.array_equal(got[0], path) and got[1] == score and np.array_equal(got[2], back)
    if kind == "ties":
        assert np.all(path < 2) and not np.array_equal(path, R.viterbi(logb, lpi, lA, "viterbi_tie_high")[0])
    if kind == "left_to_right":
        assert np.isneginf(lA).sum() == K * K - (2 * K - 1) and np.all(np.diff(path) >= 0)
    assert R.viterbi(logb, lpi, lA, "viterbi_sum_for_max")[1] != score or K == 1


@pytest.mark.parametrize("kind", ["dense", "left_to_right"])
def test_tiny_cases_equal_all_paths(kind):
    N, K = 8, 3
    e, m, pi, A = R.random_chain(N, K, 1, kind)
    if kind == "left_to_right":
        pi = np.eye(K)[0]
    logb = np.log(e) + m[:, None]
    ll, g, Xi, best, margin = R.brute(logb, pi, A)
    assert margin > 1e-6 and np.array_equal(_viterbi(logb, R.log0(pi), R.log0(A))[0], best)
    gamma, xi, llt, total = sfv.hmm_forward_backward(_dev(logb), pi, _dev(A))
    assert abs(total - ll) <= 1e-13 * max(1.0, abs(ll)) and np.abs(gamma.cpu().numpy() - g).max() <= 1e-13
    assert np.abs(xi.cpu().numpy() - Xi).max() <= 1e-13
    path, score = sfv.hmm_viterbi(_dev(logb), _dev(pi), A)
    assert np.array_equal(path.cpu().numpy(), best) and path.dtype == torch.int32


# ---- whole fits ----------------------------------------------------------------------------------------------------------------

def _as_dict(fit):
    return {"pi": fit.startprob.cpu().numpy(), "A": fit.transmat.cpu().numpy(), "means": fit.means.cpu().numpy(),
            "covars": fit.covariances.cpu().numpy(), "log_likelihoods": fit.log_likelihoods, "gamma": fit.posterior.cpu().numpy(),
            "n_iter": fit.n_iter, "converged": fit.converged, "path": fit.path.cpu().numpy()}


def _same(a, b):
    return (all(torch.equal(getattr(a, n).contiguous().view(torch.int64), getattr(b, n).contiguous().view(torch.int64))
                for n in ("startprob", "transmat", "means", "covariances", "precisions_cholesky", "posterior"))
            and torch.equal(a.path, b.path) and a.n_iter == b.n_iter and a.why == b.why and a.path_score == b.path_score
            and np.array_equal(bits(a.log_likelihoods), bits(b.log_likelihoods)))


def _check_fit(fit, ref, gates, what):
    diff = R.differences(_as_dict(fit), ref)
    bad = R.outside(diff, gates)
    print(f"{what}: device against the f64 restatement (gate = 64 x f64 / long double difference): "
          + ", ".join(f"{q} {diff[q]:.3g} ({R.GATE_FACTOR * gates[q]:.3g})" for q in R.QUANTITIES)
          + f", n_iter {fit.n_iter} = {ref['n_iter']}, path differs on {100 * diff['path']:.2f} % of the rows")
    assert not bad, (bad, diff)
    assert fit.why == ref["why"] and fit.log_likelihood == fit.log_likelihoods[-1] and len(fit.log_likelihoods) == fit.n_iter


@functools.lru_cache(maxsize=None)
def _planted_fit(name):
    X = R.planted(name)[0]
    return _dev(X), sfv.hmm(_dev(X), 4, init=R.planted(name)[2])


@pytest.mark.parametrize("name", sorted(R.PLANTED))
def test_fit_planted(name):
    X, z, start, f64, ld, gates = R.planted(name)
    Xd, fit = _planted_fit(name)
    assert fit.path.dtype == torch.int32 and fit.path.is_cuda and fit.transmat.dtype == F64 and tuple(fit.posterior.shape) == (1500, 4)
    _check_fit(fit, f64, gates, name)
    own = sfv.hmm(Xd, 4)                                    # from symbols.kmeans' labels: the recorded start
    assert torch.equal(sfv.kmeans(Xd, 4, seed=42).labels.cpu().long(), torch.from_numpy(start).long()) and _same(fit, own)
    a_start, a_path = R.ari(z, start), R.ari(z, fit.path.cpu().numpy())
    print(f"{name}: ARI of the k-means start {a_start:.3f}, of the device's Viterbi path {a_path:.3f}")
    assert a_path >= a_start and a_path >= 0.9
    assert torch.equal(sfv.hmm_predict(fit, Xd), fit.path) and torch.equal(sfv.hmm_predict_proba(fit, Xd), fit.posterior)
    ll = sfv.hmm_score_samples(fit, Xd).cpu().numpy()
    assert sfv.hmm_score(fit, Xd) == Gm.lower_bound(ll)
    bic, aic = R.criteria(Gm.lower_bound(ll), 1500, 4, 3)
    assert abs(sfv.hmm_bic(fit, Xd) / bic - 1) <= 4 * R.U and abs(sfv.hmm_aic(fit, Xd) / aic - 1) <= 4 * R.U
    assert abs(sfv.hmm_bic(fit, Xd) / R.criteria(Gm.lower_bound(ll), 1500, 4, 3, "bic_param_count_gmm")[0] - 1) > 1e-3
    assert abs(sfv.hmm_score(fit, Xd) - f64["score"]) <= R.GATE_FACTOR * gates["log_likelihoods"]


@pytest.mark.parametrize("K,seed", [(2, 0), (8, 42)])
def test_fit_fixture_latents(K, seed):
    X, start, f64, ld, gates = R.latents_case(K, seed)
    Xd = _dev(X)
    fit = sfv.hmm(Xd, K, init=start)
    _check_fit(fit, f64, gates, f"latents, K = {K}, seed {seed}")
    assert _same(fit, sfv.hmm(Xd, K, seed=seed)) and _same(fit, sfv.hmm(Xd, K, init=_dev(start)))


@pytest.mark.parametrize("name", sorted(R.PLANTED))
def test_run_ahead_changes_nothing(name):
    """iterations are enqueued eight at a time; those behind the decision must leave everything as it was: the fit equals one
    whose max_iter is exactly the iteration it converged at (6: inside the first batch; 9: the first of the second)"""
    X, z, start, f64, ld, gates = R.planted(name)
    Xd, fit = _planted_fit(name)
    n = f64["n_iter"]
    assert n == {"sticky_a": 6, "sticky_b": 9}[name] and sfv.hmm_model.ENQUEUE == 8 and fit.n_iter == n
    exact = sfv.hmm(Xd, 4, init=start, max_iter=n)
    assert exact.converged and _same(fit, exact)
    before = sfv.hmm(Xd, 4, init=start, max_iter=n - 1)
    assert not before.converged and before.why == "max_iter" and before.n_iter == n - 1
    assert np.array_equal(bits(before.log_likelihoods), bits(fit.log_likelihoods[:n - 1]))
    other = sfv.hmm(Xd, 4, init=start, block_rows=1500)     # the plain recursion: another order, the same decisions
    assert other.n_iter == n and not R.outside(R.differences(_as_dict(other), f64), gates)


def test_entries_behind_done_write_nothing():
    N, K = 65, 5
    e, m, pi, A = R.random_chain(N, K, 3, "dense")
    done = _state(1, 2, 1, 0)
    ws, nb = _ws(N, K, 7)
    gs = {"alpha": G(F64, N, K), "ll": G(F64, N), "beta": G(F64, N, K), "gamma": G(F64, K, N), "xi": G(F64, K, K),
          "A_new": G(F64, K, K), "pi_new": G(F64, K), "back": G(U8, N, K), "path": G(I32, N), "score": G(F64, 1), "ws": ws}
    st = _status()
    ed, Ad = _dev(e), _dev(A)
    call("rbvae_hmm_forward", ed, _dev(m), N, K, _dev(pi), Ad, 7, gs["alpha"].t, gs["ll"].t, st.t, ws.t, nb, done)
    call("rbvae_hmm_backward", ed, N, K, Ad, 7, gs["beta"].t, st.t, ws.t, nb, done)
    call("rbvae_hmm_posterior", ed, ed, ed, N, K, Ad, gs["gamma"].t, gs["xi"].t, gs["A_new"].t, gs["pi_new"].t, st.t, ws.t, nb, done)
    call("rbvae_hmm_viterbi", _dev(np.ascontiguousarray(e.T)), N, K, _dev(pi), Ad, gs["back"].t, gs["path"].t, gs["score"].t, done)
    for name, g in gs.items():
        untouched(g, name + " behind done")
    assert out(st, "status").tolist() == [0, R.NO_ROW] and done.cpu().tolist() == [1, 2, 1, 0]


def test_select_agrees_with_its_parts():
    X = R.planted("sticky_a")[0]
    Xd = _dev(X)
    table, K, best = sfv.hmm_select(Xd, (2, 4), max_iter=12)
    assert [row["K"] for row in table] == [2, 4] and K in (2, 4)
    for row in table:
        fit = sfv.hmm(Xd, row["K"], max_iter=12)
        score = sfv.hmm_score(fit, Xd)
        assert row["n_iter"] == fit.n_iter and row["converged"] == fit.converged and row["score"] == score
        assert row["bic"] == sfv.hmm_bic(fit, Xd) and row["aic"] == sfv.hmm_aic(fit, Xd)
        if row["K"] == K:
            assert _same(best, fit)
    assert K == [2, 4][sfv.mixture.choose(table, "bic")]


def test_latent_hmm_agrees_with_its_parts():
    F_, RES, LD = 40, 64, 16
    torch.manual_seed(0)
    model = sfv.Seq2SeqBinaryVAE(3, 3, LD, LD, variant="contrastive", input_hw=(RES, RES), compute_dtype="f32").cuda().eval()
    x = torch.rand(F_, 3, RES, RES, generator=torch.Generator().manual_seed(1)).cuda()
    u = torch.rand(F_, LD, generator=torch.Generator().manual_seed(2))
    flags = [10, 30]
    res = sfv.latent_hmm(model, x, range(F_), flags, u=u)
    mix = sfv.latent_mixture(model, x, range(F_), flags, u=u)
    assert torch.equal(res["latents"], mix["latents"]) and np.array_equal(res["labels"], mix["labels"]) and not model.training
    start = sfv.kmeans(res["latents"], 3, seed=42).labels
    fit = res["hmm"]
    assert fit.means.shape == (3, LD) and _same(fit, sfv.hmm(res["latents"], 3, init=start))
    for key, lab in (("agreement", fit.path), ("kmeans_agreement", start)):
        ref = sfv.clustering_agreement(res["labels"], lab, 3, 3)
        assert all(res[key][n] == ref[n] for n in ("ari", "nmi", "v_measure", "fowlkes_mallows"))
    path = fit.path.cpu().numpy()
    cps = [t for t in range(1, F_) if path[t] != path[t - 1]]
    assert res["change_points"] == cps and res["boundaries"] == sfv.boundary_agreement(cps, [10, 30], 2)
    assert np.array_equal(res["dwell"], 1.0 / (1.0 - np.diag(fit.transmat.cpu().numpy())))
    assert res["mean_max_posterior"] == float(fit.posterior.max(dim=1).values.mean()) and 1 / 3 <= res["mean_max_posterior"] <= 1
    again = sfv.latent_hmm(model, x, range(F_), flags, projections={"latents": res["latents"].clone()}, n_states=4)
    assert again["hmm"].means.shape == (4, LD) and again["agreement"]["contingency"].shape == (3, 4)


# ---- refused arguments -------------------------------------------------------------------------------------------------------

def test_refused_arguments_write_nothing():
    zd = lambda *s: torch.zeros(s, dtype=F64, device="cuda")      # noqa: E731
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")       # noqa: E731
    outs = {n: G(F64, 4096) for n in ("a", "b", "c", "d", "ws")}
    st, path, back = _status(), G(I32, 64), G(U8, 4096)
    X, par, mat, vec = z(300, 129), zd(65, 129), zd(300, 65), zd(300)
    nb = 4096 * 8
    for N, Ld, K, match in ((1, 1, 1, "N=1"), (8, 3, 9, "K=9"), (8, 129, 2, "L=129"), (300, 3, 65, "K=65"), (8, 0, 2, "L=0"),
                            (8, 3, 0, "K=0"), ((1 << 20) + 1, 3, 2, "N=1048577")):
        assert query("rbvae_hmm_ok", N, Ld, K) == 0
        with pytest.raises(RuntimeError, match=match):
            call("rbvae_hmm_emit", X, N, Ld, par, par, K, outs["a"].t, outs["b"].t, outs["c"].t, None)
        if Ld == 3:
            assert query("rbvae_hmm_ws_bytes", N, K, 64) == 0
            with pytest.raises(RuntimeError, match=match):
                call("rbvae_hmm_forward", mat, vec, N, K, vec, mat, 64, outs["a"].t, outs["b"].t, st.t, outs["ws"].t, nb, None)
            with pytest.raises(RuntimeError, match=match):
                call("rbvae_hmm_backward", mat, N, K, mat, 64, outs["a"].t, st.t, outs["ws"].t, nb, None)
            with pytest.raises(RuntimeError, match=match):
                call("rbvae_hmm_posterior", mat, mat, mat, N, K, mat, outs["a"].t, outs["b"].t, outs["c"].t, outs["d"].t, st.t,
                     outs["ws"].t, nb, None)
            with pytest.raises(RuntimeError, match=match):
                call("rbvae_hmm_viterbi", mat, N, K, vec, mat, back.t, path.t, outs["a"].t, None)
    with pytest.raises(ValueError, match="null"):
        call("rbvae_hmm_emit", X, 8, 3, None, par, 2, outs["a"].t, outs["b"].t, outs["c"].t, None)
    with pytest.raises(ValueError, match="null"):
        call("rbvae_hmm_forward", mat, vec, 8, 2, vec, mat, 64, outs["a"].t, outs["b"].t, None, outs["ws"].t, nb, None)
    with pytest.raises(ValueError, match="block_rows=0"):
        call("rbvae_hmm_forward", mat, vec, 8, 2, vec, mat, 0, outs["a"].t, outs["b"].t, st.t, outs["ws"].t, nb, None)
    with pytest.raises(ValueError, match="workspace"):
        call("rbvae_hmm_backward", mat, 64, 2, mat, 1, outs["a"].t, st.t, outs["ws"].t, 8, None)
    with pytest.raises(ValueError, match="workspace"):
        call("rbvae_hmm_posterior", mat, mat, mat, 8, 2, mat, outs["a"].t, outs["b"].t, outs["c"].t, outs["d"].t, st.t, None, nb, None)
    with pytest.raises(ValueError, match="null"):
        call("rbvae_hmm_viterbi", mat, 8, 2, vec, mat, None, path.t, outs["a"].t, None)
    for n, g in outs.items():
        untouched(g, n)
    untouched(path, "path")
    untouched(back, "back")
    assert out(st, "status").tolist() == [0, R.NO_ROW]
    ok = torch.rand(8, 3, generator=torch.Generator().manual_seed(0)).cuda()
    bad = ok.clone()
    bad[2, 1] = float("nan")
    fit = sfv.hmm(ok, 2, init=np.array([0, 0, 0, 0, 1, 1, 1, 1]))
    lb = zd(8, 2)
    for fn, match in ((lambda: sfv.hmm(z(8, 3), 9), "K=9"), (lambda: sfv.hmm(z(8, 129), 2), "L=129"), (lambda: sfv.hmm(z(1, 3), 1), "N=1"),
                      (lambda: sfv.hmm(z(300, 3), 65), "K=65"), (lambda: sfv.hmm(ok.cpu(), 2), "GPU"),
                      (lambda: sfv.hmm(ok.double(), 2), "float32"), (lambda: sfv.hmm(ok, 2, max_iter=0), "max_iter"),
                      (lambda: sfv.hmm(ok, 2, tol=-1.0), "tol"), (lambda: sfv.hmm(ok, 2, reg_covar=-1.0), "reg_covar"),
                      (lambda: sfv.hmm(ok, 2, init="random"), "init"), (lambda: sfv.hmm(ok, 2, block_rows=0), "block_rows"),
                      (lambda: sfv.hmm(ok, 2, init=np.array([0, 0, 0, 0, 1, 1, 1, 2])), "labels in"),
                      (lambda: sfv.hmm(ok, 2, init=np.array([0, 1, 1])), "labels in"), (lambda: sfv.hmm(bad, 2), "NaN"),
                      (lambda: sfv.hmm_predict(fit, z(8, 4)), "columns"), (lambda: sfv.hmm_score(fit, ok.cpu()), "GPU"),
                      (lambda: sfv.hmm_predict_proba(fit, bad), "NaN"), (lambda: sfv.hmm_select(ok, [2], criterion="icl"), "criterion"),
                      (lambda: sfv.hmm_forward_backward(lb.float(), [0.5, 0.5], np.eye(2)), "float64"),
                      (lambda: sfv.hmm_forward_backward(lb, [0.5, 0.5, 0.0], np.eye(2)), "pi must"),
                      (lambda: sfv.hmm_viterbi(lb, [0.5, 0.5], np.eye(3)), "A must"),
                      (lambda: sfv.hmm_viterbi(zd(1, 1), [1.0], np.eye(1)), "N=1"),
                      (lambda: sfv.latent_hmm(None, z(2, 3, 8, 8), [0], [1]), "frame indices")):
        with pytest.raises(ValueError, match=match):
            fn()
