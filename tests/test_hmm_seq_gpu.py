"""GPU: the hidden Markov model over several stacked sequences -- the rbvae_hmm_seq_ entries of csrc/hmm.hip inside sentinel
guard bands, and hmm.py's / bernoulli.py's lengths= -- against three references:
  1. the single-sequence entries run on every sequence alone (tests/test_hmm_gpu.py's guarded calls): alpha, ll, beta, back,
     path and score[s] bit for bit at the same block_rows, wherever those entries accept the sequence (n_s >= max(K, 2));
  2. with S = 1 every output of the forward, backward, posterior and Viterbi entries bit for bit;
  3. the long double restatement of tests/_hmm_seq_ref.py within its bounds, sequences of one row included, and its f64
     Viterbi bit for bit.
K in {1, 2, 17, 64} x block_rows in {64, 7} on the length lists of _hmm_seq_ref.LENGTHS (K = 64 where the lengths total at
least 64).  rbvae_hmm_ok must hold for the stacked N, so (1, 1) and (2,) with K = 17 are refused, which
test_lists_shorter_than_k_are_refused asserts with nothing written.  Whole fits against the restatement's at
tests/test_hmm_gpu.py's gates (64 times the f64 / long double difference).  Every test prints its worst |error| / bound;
DESIGN.md section 7 quotes them.

Measured on one MI355X: every run of a sequence alone (up to 400 per case) and every S = 1 output bit-equal; alpha at most
0.112, beta 0.117, ll 0.387 of their bounds (300 sequences of 1 to 3 rows, K = 2), gamma 0.074, Xi 0.010, A_new 0.005, pi_new
0.020 (both block_rows on every list); Viterbi equal to the restatement bit for bit.  The planted fits (6 and 7 iterations) and the Bernoulli fits at L = 32,
50, 128 (3, 5, 6 iterations) have n_iter and every row of the path equal and every quantity at least 100 times inside its
gate; the held-out video is labelled with ARI 0.989, the restatement's path.  The 81 tests take 8 s together, the largest
(4097 rows, K = 64) 1.0 s.
"""
import functools

import numpy as np
import pytest
import torch

import _bernoulli_ref as Bn
import _bounds as B
import _gmm_ref as Gm
import _hmm_ref as R
import _hmm_seq_ref as Q
import sfv_amd as sfv
import test_hmm_gpu as T                                    # its guarded buffers and single-sequence calls

pytestmark = pytest.mark.gpu

call, query = sfv._lib.call, sfv._lib.query
F64, I32, U8 = torch.float64, torch.int32, torch.uint8
G, out, untouched, bits, _dev, _state, _status = T.G, T.out, T.untouched, T.bits, T._dev, T._state, T._status
BLOCK_ROWS = (64, 7)
ALL = [(name, K) for name in Q.LENGTHS for K in (1, 2, 17, 64) if K < 64 or sum(Q.LENGTHS[name]) >= 64]
CASES = [(name, K) for name, K in ALL if Q.ok(sum(Q.LENGTHS[name]), 1, K, len(Q.LENGTHS[name]))]
REFUSED = [c for c in ALL if c not in CASES]


# ---- guarded calls of the entries --------------------------------------------------------------------------------------------

def _plan(lengths, Rr, N=None):
    """the device plan inside guard bands; its words are the restatement's"""
    N, S = int(np.sum(lengths)) if N is None else N, len(lengths)
    nb = query("rbvae_hmm_seq_plan_bytes", N, S, Rr)
    assert nb == Q.plan_bytes(N, S, Rr)
    g = G(I32, nb // 4)
    h = np.ascontiguousarray(lengths, dtype=np.int32)
    call("rbvae_hmm_seq_plan", h.ctypes.data, S, N, Rr, g.t, nb)
    assert np.array_equal(out(g, f"plan {lengths[:6]} block_rows {Rr}"), Q.plan(lengths, Rr))
    return g


def _ws(N, K, S, Rr):
    n = query("rbvae_hmm_seq_ws_bytes", N, K, S, Rr)
    assert n == Q.ws_bytes(N, K, S, Rr)
    return G(F64, n // 8), n


def _forward(e, m, pi, A, lengths, Rr, state=None, plan=None):
    N, K = e.shape
    S = len(lengths)
    plan = _plan(lengths, Rr) if plan is None else plan
    alpha, ll, st = G(F64, N, K), G(F64, N), _status()
    ws, nb = _ws(N, K, S, Rr)
    call("rbvae_hmm_seq_forward", _dev(e), _dev(m), N, K, _dev(pi), _dev(A), Rr, plan.t, S, alpha.t, ll.t, st.t, ws.t, nb, state)
    what = f"seq forward ({N}, {K}, S {S}, block_rows {Rr})"
    T._ws_guards(ws, "workspace " + what)
    B.assert_guards(plan, "plan after " + what)
    return out(alpha, "alpha " + what), out(ll, "ll " + what), out(st, "status " + what).tolist()


def _backward(e, A, lengths, Rr, state=None, plan=None):
    N, K = e.shape
    S = len(lengths)
    plan = _plan(lengths, Rr) if plan is None else plan
    beta, st = G(F64, N, K), _status()
    ws, nb = _ws(N, K, S, Rr)
    call("rbvae_hmm_seq_backward", _dev(e), N, K, _dev(A), Rr, plan.t, S, beta.t, st.t, ws.t, nb, state)
    what = f"seq backward ({N}, {K}, S {S}, block_rows {Rr})"
    T._ws_guards(ws, "workspace " + what)
    return out(beta, "beta " + what), out(st, "status " + what).tolist()


def _posterior(alpha, beta, e, A, lengths, state=None):
    N, K = e.shape
    S = len(lengths)
    plan = _plan(lengths, R.BLOCK_ROWS)
    gamma, xi, A_new, pi_new, st = G(F64, K, N), G(F64, K, K), G(F64, K, K), G(F64, K), _status()
    nb = 8 * (N + Gm.blocks_rows(N)[0] * K * K)            # its own need, below the recurrence's at many short sequences
    ws = G(F64, nb // 8)
    call("rbvae_hmm_seq_posterior", _dev(alpha), _dev(beta), _dev(e), N, K, plan.t, S, _dev(A), gamma.t, xi.t, A_new.t, pi_new.t,
         st.t, ws.t, nb, state)
    what = f"seq posterior ({N}, {K}, S {S})"
    T._ws_guards(ws, "workspace " + what)
    return (out(gamma, "gamma " + what).T, out(xi, "Xi " + what), out(A_new, "A_new " + what), out(pi_new, "pi_new " + what),
            out(st, "status " + what).tolist())


def _viterbi(logb, lpi, lA, lengths, state=None):
    N, K = logb.shape
    S = len(lengths)
    plan = _plan(lengths, 7)                                # Viterbi reads the parts that do not depend on block_rows
    back, path, score = G(U8, N, K), G(I32, N), G(F64, S)
    call("rbvae_hmm_seq_viterbi", _dev(np.ascontiguousarray(logb.T)), N, K, plan.t, S, _dev(lpi), _dev(lA), back.t, path.t, score.t,
         state)
    what = f"seq viterbi ({N}, {K}, S {S})"
    return out(path, "path " + what), out(score, "score " + what), out(back, "back " + what)


def _accepted(lengths, K):
    return [(s, lo, hi) for s, (lo, hi) in enumerate(Q.spans(lengths)) if hi - lo >= max(K, 2)]


# ---- 1 and 3: every sequence alone, and the long double bounds -----------------------------------------------------------------

@pytest.mark.parametrize("name,K", CASES)
def test_recursions(name, K):
    lengths, e, m, pi, A = Q.chain(name, K)
    ld = Q.ld_passes(e, m, pi, A, lengths)
    worst, alone = [], 0
    for Rr in BLOCK_ROWS:
        ref = Q.recurrence_bounds(e, m, pi, A, lengths, Rr, ld=ld)
        plan = _plan(lengths, Rr)
        al, ll, sa = _forward(e, m, pi, A, lengths, Rr, plan=plan)
        be, sb = _backward(e, A, lengths, Rr, plan=plan)
        assert sa == sb == [0, R.NO_ROW]
        worst += [R.within(al, ref["alpha"], ref["b_alpha"], f"alpha block_rows {Rr}"),
                  R.within(be, ref["beta"], ref["b_beta"], f"beta block_rows {Rr}"),
                  R.within(ll, ref["ll"], ref["b_ll"], f"ll block_rows {Rr}")]
        for s, lo, hi in _accepted(lengths, K):
            a1, l1, _ = T._forward(e[lo:hi], m[lo:hi], pi, A, Rr)
            b1, _ = T._backward(e[lo:hi], A, Rr)
            assert np.array_equal(bits(al[lo:hi]), bits(a1)) and np.array_equal(bits(ll[lo:hi]), bits(l1)), (s, Rr, "forward")
            assert np.array_equal(bits(be[lo:hi]), bits(b1)), (s, Rr, "backward")
            alone += 1
    print(f"seq recursions {name} {lengths[:6]}, K = {K}: {alone} runs of a sequence alone bit-equal; worst |err|/bound (alpha, "
          f"beta, ll per block_rows {BLOCK_ROWS}) " + ", ".join(f"{x:.3g}" for x in worst))
    al2, ll2, _ = _forward(e, m, pi, A, lengths, BLOCK_ROWS[0])
    assert np.array_equal(bits(al2), bits(_forward(e, m, pi, A, lengths, BLOCK_ROWS[0])[0])), "two runs differ"
    # the posterior of the device's own alpha and beta at the default block_rows
    ref = Q.recurrence_bounds(e, m, pi, A, lengths, R.BLOCK_ROWS, ld=ld)
    be, _ = _backward(e, A, lengths, R.BLOCK_ROWS)
    post = Q.posterior_bounds(ref["alpha"], ref["beta"], e, A, ref["rho_a"], ref["rho_b"], lengths)
    gamma, Xi, A_new, pi_new, st = _posterior(al2, be, e, A, lengths)
    N, S = len(e), len(lengths)
    w = [R.within(gamma, post["gamma"], post["b_gamma"], "gamma"), R.within(Xi, post["xi"], post["b_xi"], "Xi"),
         R.within(A_new, post["A_new"], post["b_A_new"], "A_new"), R.within(pi_new, post["pi_new"], post["b_pi_new"], "pi_new")]
    sg = float(np.abs(gamma.astype(R.LD).sum(axis=1) - 1).max())
    sx = abs(float(Xi.astype(R.LD).sum()) - (N - S))
    print(f"seq posterior {name}, K = {K}: worst |err|/bound gamma {w[0]:.3g}, Xi {w[1]:.3g}, A_new {w[2]:.3g}, pi_new {w[3]:.3g}; "
          f"|sum gamma - 1| <= {sg:.3g} ({post['b_gamma_sum']:.3g}), |sum Xi - (N - S)| = {sx:.3g} ({post['b_xi_sum']:.3g})")
    assert st == [0, R.NO_ROW] and sg <= post["b_gamma_sum"] and sx <= post["b_xi_sum"]
    again = _posterior(al2, be, e, A, lengths)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip((gamma, Xi, A_new, pi_new), again)), "two runs differ"


@pytest.mark.parametrize("name,K", CASES)
def test_viterbi(name, K):
    lengths, e, m, pi, A = Q.chain(name, K, 6, "sticky" if K in (2, 17) else "dense")
    logb = np.log(e) + m[:, None]
    lpi, lA = R.log0(pi), R.log0(A)
    path, score, back = _viterbi(logb, lpi, lA, lengths)
    rp, rs, rb = Q.viterbi(logb, lpi, lA, lengths)
    assert np.array_equal(path, rp) and np.array_equal(bits(score), bits(rs)) and np.array_equal(back, rb)
    assert not back[[lo for lo, _ in Q.spans(lengths)]].any()
    for s, lo, hi in _accepted(lengths, K):
        p1, s1, b1 = T._viterbi(logb[lo:hi], lpi, lA)
        assert np.array_equal(path[lo:hi], p1) and score[s] == s1 and np.array_equal(back[lo:hi], b1), s
    if len(lengths) > 1 and K > 1:
        assert not np.array_equal(Q.viterbi(logb, lpi, lA, lengths, "viterbi_crosses_boundary")[2], back)


@pytest.mark.parametrize("name,K", REFUSED)
def test_lists_shorter_than_k_are_refused(name, K):
    """the stacked N is below K: outside rbvae_hmm_ok, so every entry refuses without a launch"""
    lengths, N, S = Q.LENGTHS[name], sum(Q.LENGTHS[name]), len(Q.LENGTHS[name])
    assert (name, K) in (("ones", 17), ("pair", 17)) and query("rbvae_hmm_seq_ok", N, 1, K, S) == 0
    assert query("rbvae_hmm_seq_ws_bytes", N, K, S, 64) == 0
    plan = _plan(lengths, 64)                               # the plan itself does not ask for K
    big, st, back, path = {n: G(F64, 4096) for n in "abcdw"}, _status(), G(U8, 4096), G(I32, 64)
    mat = torch.zeros(64, 64, dtype=F64, device="cuda")
    with pytest.raises(RuntimeError, match=f"K={K}"):
        call("rbvae_hmm_seq_forward", mat, mat, N, K, mat, mat, 64, plan.t, S, big["a"].t, big["b"].t, st.t, big["w"].t, 32768, None)
    with pytest.raises(RuntimeError, match=f"K={K}"):
        call("rbvae_hmm_seq_backward", mat, N, K, mat, 64, plan.t, S, big["a"].t, st.t, big["w"].t, 32768, None)
    with pytest.raises(RuntimeError, match=f"K={K}"):
        call("rbvae_hmm_seq_posterior", mat, mat, mat, N, K, plan.t, S, mat, big["a"].t, big["b"].t, big["c"].t, big["d"].t, st.t,
             big["w"].t, 32768, None)
    with pytest.raises(RuntimeError, match=f"K={K}"):
        call("rbvae_hmm_seq_viterbi", mat, N, K, plan.t, S, mat, mat, back.t, path.t, big["a"].t, None)
    for n, g in list(big.items()) + [("back", back), ("path", path)]:
        untouched(g, n)
    assert out(st, "status").tolist() == [0, R.NO_ROW]


# ---- 2: one sequence is the single-sequence entries' bytes -----------------------------------------------------------------------

@pytest.mark.parametrize("name,K", [(n, K) for n, K in CASES if len(Q.LENGTHS[n]) == 1])
def test_one_sequence_is_the_existing_entries(name, K):
    lengths, e, m, pi, A = Q.chain(name, K, 5)
    N = len(e)
    for Rr in BLOCK_ROWS + (N, N + 5):
        al, ll, sa = _forward(e, m, pi, A, lengths, Rr)
        be, sb = _backward(e, A, lengths, Rr)
        a1, l1, s1 = T._forward(e, m, pi, A, Rr)
        b1, s2 = T._backward(e, A, Rr)
        assert np.array_equal(bits(al), bits(a1)) and np.array_equal(bits(ll), bits(l1)) and np.array_equal(bits(be), bits(b1))
        assert sa == s1 and sb == s2
    alpha, beta = T._rows_of_mass(N, K, 1), T._rows_of_mass(N, K, 2)
    alpha[N // 2] = 0.0                                     # a zero normaliser: the same count and row
    for x, y in zip(_posterior(alpha, beta, e, A, lengths), T._posterior(alpha, beta, e, A)):
        assert np.array_equal(bits(np.asarray(x)), bits(np.asarray(y)))
    logb = np.log(e) + m[:, None]
    p, s, b = _viterbi(logb, R.log0(pi), R.log0(A), lengths)
    p1, s1, b1 = T._viterbi(logb, R.log0(pi), R.log0(A))
    assert np.array_equal(p, p1) and s[0] == s1 and np.array_equal(b, b1)


# ---- 4: where a missed reset shows ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["sticky", "left_to_right"])
@pytest.mark.parametrize("name", ["mixed", "tail"])
def test_recursions_where_a_reset_matters(name, kind):
    """a sticky overlapping chain and a left-to-right A: a sequence that started from its predecessor's last row
    (no_reset_at_start, beta_not_reset) is outside the same bounds"""
    lengths, e, m, pi, A = Q.chain(name, 5, 3, kind)
    ld = Q.ld_passes(e, m, pi, A, lengths)
    for Rr in BLOCK_ROWS:
        ref = Q.recurrence_bounds(e, m, pi, A, lengths, Rr, ld=ld)
        al, ll, sa = _forward(e, m, pi, A, lengths, Rr)
        be, sb = _backward(e, A, lengths, Rr)
        w = [R.within(al, ref["alpha"], ref["b_alpha"], "alpha"), R.within(be, ref["beta"], ref["b_beta"], "beta"),
             R.within(ll, ref["ll"], ref["b_ll"], "ll")]
        print(f"{name}, {kind}, block_rows {Rr}: worst |err|/bound alpha, beta, ll " + ", ".join(f"{x:.3g}" for x in w))
        assert sa == sb == [0, R.NO_ROW]
        assert R.rejects(Q.forward(e, m, pi, A, lengths, "no_reset_at_start", R_=Rr)[0], ref["alpha"], ref["b_alpha"])
        assert R.rejects(Q.backward(e, A, lengths, "beta_not_reset", R_=Rr)[0], ref["beta"], ref["b_beta"])


@pytest.mark.parametrize("Rr", BLOCK_ROWS)
def test_impossible_first_observation_of_the_second_sequence(Rr):
    """no state can emit the first row of sequence 1: that row is status[1], its sequence is lost, no other is touched"""
    lengths, e, m, pi, A = Q.chain("mixed", 5, 4)
    (lo, hi), N = Q.spans(lengths)[1], len(e)
    ez = e.copy()
    ez[lo] = 0.0
    al, ll, st = _forward(ez, m, pi, A, lengths, Rr)
    good = _forward(e, m, pi, A, lengths, Rr)[0]
    assert st == [hi - lo, lo] == Q.forward(ez, m, pi, A, lengths, R_=Rr)[2]
    assert np.isnan(al[lo:hi]).all() and np.array_equal(bits(al[:lo]), bits(good[:lo])) and np.array_equal(bits(al[hi:]), bits(good[hi:]))
    be, st = _backward(ez, A, lengths, Rr)
    good = _backward(e, A, lengths, Rr)[0]
    assert st == [1, lo - 1] if lengths[0] > 1 else st == [0, R.NO_ROW]      # sequence 0 has one row: beta = 1 / K, no normaliser
    assert np.array_equal(bits(be[lo:]), bits(good[lo:])) and np.isfinite(be).all()
    alpha, beta = T._rows_of_mass(N, 5, 1), T._rows_of_mass(N, 5, 2)
    az = alpha.copy()
    az[hi - 1] = 0.0                                        # the last row of a sequence: its g only, no Z exists there
    assert _posterior(az, beta, e, A, lengths)[4] == [1, hi - 1]
    az = alpha.copy()
    az[hi - 2] = 0.0                                        # the row before: g and Z
    assert _posterior(az, beta, e, A, lengths)[4] == [2, hi - 2]


# ---- 5: whole fits -------------------------------------------------------------------------------------------------------------

def _same(a, b):
    return T._same(a, b) and a.lengths == b.lengths and np.array_equal(bits(a.path_scores), bits(b.path_scores))


@functools.lru_cache(maxsize=None)
def _planted_fit(name):
    X, z, lengths, start = Q.planted(name)[:4]
    return _dev(X), sfv.hmm(_dev(X), 4, init=start, lengths=lengths)


@pytest.mark.parametrize("name", sorted(Q.FITS))
def test_fit_planted(name):
    X, z, lengths, start, f64, ld, gates = Q.planted(name)
    Xd, fit = _planted_fit(name)
    N, S = len(X), len(lengths)
    T._check_fit(fit, f64, gates, f"{name} {lengths[:4]}")
    assert fit.lengths == tuple(lengths) and fit.path_scores.shape == (S,) and fit.path_scores.dtype == np.float64
    assert fit.path_score == Q.sum_ascending(fit.path_scores) and np.abs(fit.path_scores - f64["path_scores"]).max() <= 1e-9
    assert _same(fit, sfv.hmm(Xd, 4, init=start, lengths=list(lengths))), "two runs differ"
    a_start, a_path = R.ari(z, start), R.ari(z, fit.path.cpu().numpy())
    print(f"{name}: ARI of the k-means start {a_start:.3f}, of the device's Viterbi path {a_path:.3f}")
    assert a_path >= a_start and a_path >= 0.9
    # run-ahead: the fit equals one whose max_iter is exactly the iteration it converged at
    n = f64["n_iter"]
    assert fit.n_iter == n and sfv.hmm_model.ENQUEUE == 8
    exact = sfv.hmm(Xd, 4, init=start, max_iter=n, lengths=lengths)
    assert exact.converged and _same(fit, exact)
    before = sfv.hmm(Xd, 4, init=start, max_iter=n - 1, lengths=lengths)
    assert not before.converged and before.why == "max_iter" and np.array_equal(bits(before.log_likelihoods), bits(fit.log_likelihoods[:n - 1]))
    other = sfv.hmm(Xd, 4, init=start, block_rows=7, lengths=lengths)       # another order, the same decisions
    assert other.n_iter == n and not R.outside(R.differences(T._as_dict(other), f64), gates)
    # the fit's own parameters on its data, all at once and sequence by sequence
    assert torch.equal(sfv.hmm_predict(fit, Xd, lengths), fit.path) and torch.equal(sfv.hmm_predict_proba(fit, Xd, lengths), fit.posterior)
    ll = sfv.hmm_score_samples(fit, Xd, lengths)
    proba = sfv.hmm_predict_proba(fit, Xd, lengths)
    for s, lo, hi in _accepted(lengths, 4):
        assert torch.equal(sfv.hmm_predict(fit, Xd[lo:hi]), fit.path[lo:hi])
        assert torch.equal(sfv.hmm_score_samples(fit, Xd[lo:hi]).view(torch.int64), ll[lo:hi].view(torch.int64))
        assert torch.equal(sfv.hmm_predict_proba(fit, Xd[lo:hi]).contiguous().view(torch.int64), proba[lo:hi].contiguous().view(torch.int64))
    scores = sfv.hmm_sequence_scores(fit, Xd, lengths)
    assert np.array_equal(bits(scores), bits(Q.sequence_scores(ll.cpu().numpy(), lengths))) and scores.shape == (S,)
    assert np.abs(scores - Q.sequence_scores(f64["ll"], lengths)).max() <= 1e-9
    assert sfv.hmm_score(fit, Xd, lengths) == Gm.lower_bound(ll.cpu().numpy())
    bic, aic = R.criteria(Gm.lower_bound(ll.cpu().numpy()), N, 4, 3)
    assert abs(sfv.hmm_bic(fit, Xd, lengths) / bic - 1) <= 4 * R.U and abs(sfv.hmm_aic(fit, Xd, lengths) / aic - 1) <= 4 * R.U
    assert sfv.hmm_model.change_points(fit.path, lengths) == Q.change_points(fit.path.cpu().numpy(), lengths)
    # no boundary: another model
    assert not torch.equal(sfv.hmm(Xd, 4, init=start).transmat, fit.transmat)


def test_entries_behind_done_write_nothing():
    lengths, e, m, pi, A = Q.chain("tail", 5)
    N, K, S = len(e), 5, len(lengths)
    done = _state(1, 2, 1, 0)
    plan = _plan(lengths, 7)
    ws, nb = _ws(N, K, S, 7)
    gs = {"alpha": G(F64, N, K), "ll": G(F64, N), "beta": G(F64, N, K), "gamma": G(F64, K, N), "xi": G(F64, K, K),
          "A_new": G(F64, K, K), "pi_new": G(F64, K), "back": G(U8, N, K), "path": G(I32, N), "score": G(F64, S), "ws": ws}
    st = _status()
    ed, Ad = _dev(e), _dev(A)
    call("rbvae_hmm_seq_forward", ed, _dev(m), N, K, _dev(pi), Ad, 7, plan.t, S, gs["alpha"].t, gs["ll"].t, st.t, ws.t, nb, done)
    call("rbvae_hmm_seq_backward", ed, N, K, Ad, 7, plan.t, S, gs["beta"].t, st.t, ws.t, nb, done)
    call("rbvae_hmm_seq_posterior", ed, ed, ed, N, K, plan.t, S, Ad, gs["gamma"].t, gs["xi"].t, gs["A_new"].t, gs["pi_new"].t, st.t,
         ws.t, nb, done)
    call("rbvae_hmm_seq_viterbi", _dev(np.ascontiguousarray(e.T)), N, K, plan.t, S, _dev(pi), Ad, gs["back"].t, gs["path"].t,
         gs["score"].t, done)
    for name, g in gs.items():
        untouched(g, name + " behind done")
    assert out(st, "status").tolist() == [0, R.NO_ROW] and done.cpu().tolist() == [1, 2, 1, 0]


# ---- 6: refused arguments --------------------------------------------------------------------------------------------------------

def test_refused_arguments_write_nothing():
    zd = lambda *s: torch.zeros(s, dtype=F64, device="cuda")      # noqa: E731
    outs = {n: G(F64, 4096) for n in ("a", "b", "c", "d", "ws")}
    st, path, back, plan = _status(), G(I32, 64), G(U8, 4096), G(I32, 4096)
    mat, vec = zd(300, 65), zd(300)
    nb, pb = 4096 * 8, 4096 * 4
    h = lambda *l: np.ascontiguousarray(l, dtype=np.int32)        # noqa: E731
    for lengths, N, kw, err, match in (((3, 0, 5), 8, {}, ValueError, "lengths"), ((3, 4), 8, {}, ValueError, "add to 7"),
                                       ((3, 6), 8, {}, ValueError, "more than"), ((3, 5), 8, {"Rr": 0}, ValueError, "block_rows=0"),
                                       ((3, 5), 8, {"pb": Q.plan_bytes(8, 2, 64) - 4}, ValueError, "plan of"),
                                       ((1,) * 9, 8, {}, RuntimeError, "S=9"), ((3, 5), 8, {"S": 0}, RuntimeError, "S=0"),
                                       ((3, 5), 8, {"dev": None}, ValueError, "null")):
        with pytest.raises(err, match=match):
            call("rbvae_hmm_seq_plan", h(*lengths).ctypes.data, kw.get("S", len(lengths)), N, kw.get("Rr", 64),
                 kw["dev"] if "dev" in kw else plan.t, kw.get("pb", pb))
    with pytest.raises(ValueError, match="null"):
        call("rbvae_hmm_seq_plan", None, 2, 8, 64, plan.t, pb)
    for N, K, S, match in ((1, 1, 1, "N=1"), (8, 9, 2, "K=9"), (300, 65, 2, "K=65"), (8, 2, 0, "S=0"), (8, 2, 9, "S=9")):
        assert query("rbvae_hmm_seq_ok", N, 3, K, S) == 0 and query("rbvae_hmm_seq_ws_bytes", N, K, S, 64) == 0
        with pytest.raises(RuntimeError, match=match):
            call("rbvae_hmm_seq_forward", mat, vec, N, K, vec, mat, 64, plan.t, S, outs["a"].t, outs["b"].t, st.t, outs["ws"].t, nb, None)
        with pytest.raises(RuntimeError, match=match):
            call("rbvae_hmm_seq_backward", mat, N, K, mat, 64, plan.t, S, outs["a"].t, st.t, outs["ws"].t, nb, None)
        with pytest.raises(RuntimeError, match=match):
            call("rbvae_hmm_seq_posterior", mat, mat, mat, N, K, plan.t, S, mat, outs["a"].t, outs["b"].t, outs["c"].t, outs["d"].t,
                 st.t, outs["ws"].t, nb, None)
        with pytest.raises(RuntimeError, match=match):
            call("rbvae_hmm_seq_viterbi", mat, N, K, plan.t, S, vec, mat, back.t, path.t, outs["a"].t, None)
    with pytest.raises(ValueError, match="null"):
        call("rbvae_hmm_seq_forward", mat, vec, 8, 2, vec, mat, 64, None, 2, outs["a"].t, outs["b"].t, st.t, outs["ws"].t, nb, None)
    with pytest.raises(ValueError, match="null"):
        call("rbvae_hmm_seq_backward", mat, 8, 2, mat, 64, plan.t, 2, outs["a"].t, None, outs["ws"].t, nb, None)
    with pytest.raises(ValueError, match="block_rows=0"):
        call("rbvae_hmm_seq_forward", mat, vec, 8, 2, vec, mat, 0, plan.t, 2, outs["a"].t, outs["b"].t, st.t, outs["ws"].t, nb, None)
    with pytest.raises(ValueError, match="workspace"):
        call("rbvae_hmm_seq_backward", mat, 64, 2, mat, 1, plan.t, 2, outs["a"].t, st.t, outs["ws"].t, 8, None)
    with pytest.raises(ValueError, match="workspace"):
        call("rbvae_hmm_seq_posterior", mat, mat, mat, 8, 2, plan.t, 2, mat, outs["a"].t, outs["b"].t, outs["c"].t, outs["d"].t, st.t,
             None, nb, None)
    with pytest.raises(ValueError, match="null"):
        call("rbvae_hmm_seq_viterbi", mat, 8, 2, None, 2, vec, mat, back.t, path.t, outs["a"].t, None)
    with pytest.raises(ValueError, match="null"):
        call("rbvae_hmm_seq_viterbi", mat, 8, 2, plan.t, 2, vec, mat, None, path.t, outs["a"].t, None)
    for n, g in outs.items():
        untouched(g, n)
    for g, n in ((path, "path"), (back, "back"), (plan, "plan")):
        untouched(g, n)
    assert out(st, "status").tolist() == [0, R.NO_ROW]
    ok = torch.rand(8, 3, generator=torch.Generator().manual_seed(0)).cuda()
    fit = sfv.hmm(ok, 2, init=np.array([0, 0, 0, 0, 1, 1, 1, 1]), lengths=(3, 5))
    lb = zd(8, 2)
    for fn in (lambda: sfv.hmm(ok, 2, lengths=(3, 4)), lambda: sfv.hmm(ok, 2, lengths=(3, 0, 5)), lambda: sfv.hmm(ok, 2, lengths=()),
               lambda: sfv.hmm_predict(fit, ok, (9,)), lambda: sfv.hmm_score(fit, ok, (4, 5)), lambda: sfv.hmm_sequence_scores(fit, ok, (8, 1)),
               lambda: sfv.hmm_forward_backward(lb, [0.5, 0.5], np.eye(2), lengths=(7,)), lambda: sfv.bhmm(ok, 2, lengths=(3, 4)),
               lambda: sfv.hmm_viterbi(lb, [0.5, 0.5], np.eye(2), lengths=(-1, 9)), lambda: sfv.hmm_select(ok, [2], lengths=(1, 1))):
        with pytest.raises(ValueError, match="lengths"):
            fn()


# ---- 7: the Python surface -------------------------------------------------------------------------------------------------------

def test_no_lengths_and_one_length_are_the_existing_path():
    X, z, start = R.planted("sticky_a")[:3]
    Xd = _dev(X)
    old = sfv.hmm(Xd, 4, init=start)
    none, one = sfv.hmm(Xd, 4, init=start, lengths=None), sfv.hmm(Xd, 4, init=start, lengths=(len(X),))
    assert T._same(old, none) and none.lengths is None and none.path_scores is None
    assert T._same(old, one) and one.lengths == (len(X),) and one.path_scores.tolist() == [old.path_score]
    assert torch.equal(sfv.hmm_predict(old, Xd, (len(X),)), old.path) and sfv.hmm_score(old, Xd, (len(X),)) == sfv.hmm_score(old, Xd)
    lb = _dev(np.log(R.random_chain(300, 5, 3)[0]))
    pi, A = R.random_chain(300, 5, 3)[2:]
    a, b = sfv.hmm_forward_backward(lb, pi, A), sfv.hmm_forward_backward(lb, pi, A, lengths=(300,))
    assert all(torch.equal(x.contiguous().view(torch.int64), y.contiguous().view(torch.int64)) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]
    p, s = sfv.hmm_viterbi(lb, pi, A)
    p1, s1, each = sfv.hmm_viterbi(lb, pi, A, lengths=(300,))
    assert torch.equal(p, p1) and s == s1 == each[0]
    lengths = (1, 100, 2, 197)
    g, xi, ll, total = sfv.hmm_forward_backward(lb, pi, A, lengths=lengths)
    assert abs(float(xi.sum()) - 296) <= 1e-9 and abs(total - float(ll.sum())) <= 1e-9
    p2, s2, each = sfv.hmm_viterbi(lb, pi, A, lengths=lengths)
    rp, rs, _ = Q.viterbi(lb.cpu().numpy(), R.log0(pi), R.log0(A), lengths)
    assert np.array_equal(p2.cpu().numpy(), rp) and np.array_equal(bits(each), bits(rs)) and s2 == Q.sum_ascending(rs)


@pytest.mark.parametrize("Ld", sorted(Q.CODES))
def test_bhmm_with_lengths(Ld):
    X, s, start, f64, ld, gates = Q.planted_codes(Ld)
    lengths, K, N = Q.CODE_LENGTHS, Q.CODES[Ld][2], len(X)
    Xd = _dev(X)
    fit = sfv.bhmm(Xd, K, init=start, lengths=lengths)
    as_dict = {"pi": fit.startprob.cpu().numpy(), "A": fit.transmat.cpu().numpy(), "probs": fit.probs.cpu().numpy(),
               "log_likelihoods": fit.log_likelihoods, "gamma": fit.posterior.cpu().numpy(), "n_iter": fit.n_iter,
               "converged": fit.converged, "path": fit.path.cpu().numpy()}
    d = Bn.differences(as_dict, f64, Bn.BHMM_QUANTITIES, "path")
    print(f"bhmm, L = {Ld}, lengths {lengths}, n_iter {fit.n_iter} = {f64['n_iter']}: device against the f64 restatement (gate = 64 x "
          f"f64 / long double difference): " + ", ".join(f"{q} {d[q]:.3g} ({Bn.GATE_FACTOR * gates[q]:.3g})" for q in Bn.BHMM_QUANTITIES))
    bad = Bn.outside(d, gates, Bn.BHMM_QUANTITIES, "path")
    assert not bad, (bad, d)
    assert fit.why == f64["why"] and fit.lengths == lengths and fit.path_score == Q.sum_ascending(fit.path_scores)
    assert np.abs(fit.path_scores - f64["path_scores"]).max() <= 1e-9 and R.ari(s, fit.path.cpu().numpy()) >= 0.95
    again = sfv.bhmm(Xd, K, init=_dev(start), lengths=lengths)
    names = ("startprob", "transmat", "probs", "posterior", "path")
    same = lambda a, b: all(torch.equal(getattr(a, n).contiguous(), getattr(b, n).contiguous()) for n in names)   # noqa: E731
    assert same(fit, again) and np.array_equal(bits(fit.path_scores), bits(again.path_scores)), "two runs differ"
    assert np.array_equal(bits(fit.log_likelihoods), bits(again.log_likelihoods))
    assert torch.equal(sfv.bhmm_predict(fit, Xd, lengths), fit.path) and torch.equal(sfv.bhmm_predict_proba(fit, Xd, lengths), fit.posterior)
    ll = sfv.bhmm_score_samples(fit, Xd, lengths)
    for _, lo, hi in _accepted(lengths, K):
        assert torch.equal(sfv.bhmm_predict(fit, Xd[lo:hi]), fit.path[lo:hi])
        assert torch.equal(sfv.bhmm_score_samples(fit, Xd[lo:hi]).view(torch.int64), ll[lo:hi].view(torch.int64))
    assert sfv.bhmm_score(fit, Xd, lengths) == Gm.lower_bound(ll.cpu().numpy())
    assert abs(sfv.bhmm_bic(fit, Xd, lengths) / Bn.criteria(Gm.lower_bound(ll.cpu().numpy()), N, Bn.bhmm_n_parameters(K, Ld))[0] - 1) <= 4 * R.U
    one, old = sfv.bhmm(Xd, K, init=start, lengths=(N,)), sfv.bhmm(Xd, K, init=start)
    assert same(one, old) and one.path_scores.tolist() == [old.path_score] and old.lengths is None
    assert not torch.equal(old.transmat, fit.transmat)


def test_select_agrees_with_its_parts():
    X, z, lengths, start = Q.planted("uneven")[:4]
    Xd = _dev(X)
    table, K, best = sfv.hmm_select(Xd, (2, 4), max_iter=12, lengths=lengths)
    assert [row["K"] for row in table] == [2, 4] and K == [2, 4][sfv.mixture.choose(table, "bic")]
    for row in table:
        fit = sfv.hmm(Xd, row["K"], max_iter=12, lengths=lengths)
        assert row["n_iter"] == fit.n_iter and row["score"] == sfv.hmm_score(fit, Xd, lengths)
        assert row["bic"] == sfv.hmm_bic(fit, Xd, lengths) and row["aic"] == sfv.hmm_aic(fit, Xd, lengths)
        if row["K"] == K:
            assert _same(best, fit)


def test_held_out_video_is_labelled_from_the_others():
    """three planted videos of one task: the model of the first two labels the third (the restatement alone reaches ARI 0.989)"""
    X, z, lengths, f, rpath, rari = Q.videos()
    n = lengths[0] + lengths[1]
    Xd = _dev(X)
    fit = sfv.hmm(Xd[:n].contiguous(), 4, init=R.kmeans_labels(X[:n], 4), lengths=lengths[:2])    # the restatement's start
    path = sfv.hmm_predict(fit, Xd[n:].contiguous()).cpu().numpy()
    ari = R.ari(z[n:], path)
    print(f"held-out video: ARI {ari:.4f} on the device, {rari:.4f} by the restatement; paths differ on {(path != rpath).mean():.4f}")
    assert ari >= 0.98 and (path != rpath).mean() <= 0.01
    both = sfv.hmm_predict(fit, Xd, lengths).cpu().numpy()
    assert np.array_equal(both[n:], path) and np.array_equal(both[:n], fit.path.cpu().numpy())
    scores = sfv.hmm_sequence_scores(fit, Xd, lengths)
    assert scores.shape == (3,) and np.isfinite(scores).all()


def test_latent_hmm_videos_agrees_with_its_parts():
    RES, LD, frames = 64, 16, (40, 30, 35)
    torch.manual_seed(0)
    model = sfv.Seq2SeqBinaryVAE(3, 3, LD, LD, variant="contrastive", input_hw=(RES, RES), compute_dtype="f32").cuda().eval()
    xs = [torch.rand(F_, 3, RES, RES, generator=torch.Generator().manual_seed(1 + v)).cuda() for v, F_ in enumerate(frames)]
    us = [torch.rand(F_, LD, generator=torch.Generator().manual_seed(7 + v)) for v, F_ in enumerate(frames)]
    idx, flags = [range(F_) for F_ in frames], [[10, 30], [8, 20], [12, 25]]
    res = sfv.latent_hmm_videos(model, xs, idx, flags, holdout=2, u=us)
    for v in range(3):
        one = sfv.latent_hmm(model, xs[v], idx[v], flags[v], u=us[v], max_iter=1)
        assert torch.equal(res["latents"][v], one["latents"]) and np.array_equal(res["labels"][v], one["labels"])
    z = res["latents"]
    assert res["lengths"] == [40, 30] and not model.training
    fit = res["hmm"]
    assert _same(fit, sfv.hmm(torch.cat(z[:2]).contiguous(), 3, lengths=(40, 30))) and fit.means.shape == (3, LD)
    paths = [fit.path[:40], fit.path[40:], sfv.hmm_predict(fit, z[2])]
    for v, entry in enumerate(res["videos"]):
        assert entry["fitted"] == (v != 2) and torch.equal(entry["path"], paths[v])
        ref = sfv.clustering_agreement(res["labels"][v], paths[v], 3, 3)
        assert all(entry["agreement"][k] == ref[k] for k in ("ari", "nmi", "v_measure", "fowlkes_mallows"))
        p = paths[v].cpu().numpy()
        cps = [t for t in range(1, frames[v]) if p[t] != p[t - 1]]
        assert entry["change_points"] == cps and entry["boundaries"] == sfv.boundary_agreement(cps, flags[v], 2)
    held = res["videos"][2]
    assert held["predict_agreement"]["ari"] == held["agreement"]["ari"] and held["predict_boundaries"] == held["boundaries"]
    assert "predict_agreement" not in res["videos"][0]
    every = sfv.latent_hmm_videos(model, xs, idx, flags, u=us, n_states=4)
    assert every["lengths"] == [40, 30, 35] and every["hmm"].means.shape == (4, LD) and all(e["fitted"] for e in every["videos"])
