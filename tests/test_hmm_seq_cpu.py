"""CPU: tests/_hmm_seq_ref.py (the restatement of the hidden Markov model over several stacked sequences that
tests/test_hmm_seq_gpu.py compares the rbvae_hmm_seq_ entries and hmm.py's lengths= with) against the enumeration of all
paths per sequence, against its long double twin inside the bounds it states, and every check of the GPU tests against the
named defect it has to reject, on the GPU tests' own inputs; the header, the sizes and the host side of hmm.py.

Measured here: the planted chains cut into (300, 1, 299) and into 20 pieces converge after 6 and 7 iterations (k-means ARI
0.65 and 0.59, Viterbi ARI 0.97 and 0.94, f64 and long double paths equal); the third of three planted videos is labelled
from a fit on the other two with ARI 0.989 by the restatement alone."""
import ctypes

import numpy as np
import pytest
import torch

import _hmm_ref as R
import _hmm_seq_ref as Q
import sfv_amd as sfv


def _passes(lengths, e, m, pi, A, Rr=None, defect=None):
    al, ll, sa = Q.forward(e, m, pi, A, lengths, defect, R_=Rr)
    be, sb = Q.backward(e, A, lengths, defect, R_=Rr)
    return al, be, ll, sa, sb


# ---- the restatement against all paths and long double ------------------------------------------------------------------------

@pytest.mark.parametrize("lengths,K,kind", [((2, 1, 3), 2, "dense"), ((1, 1), 1, "dense"), ((3, 1, 1, 2), 3, "left_to_right"),
                                            ((6,), 2, "dense")])
def test_equals_all_paths_per_sequence(lengths, K, kind):
    N = sum(lengths)
    e, m, pi, A = R.random_chain(N, K, 1, kind)
    logb = np.log(e) + m[:, None]
    ll, g, Xi, path, margin = Q.brute(logb, pi, A, lengths)
    for Rr in (None, 1, 2):
        al, be, llt, sa, sb = _passes(lengths, e, m, pi, A, Rr)
        gamma, X2, _, pi_new, sp = Q.posterior(al, be, e, A, lengths)
        assert abs(float(llt.astype(R.LD).sum()) - ll) <= 1e-13 * max(1.0, abs(ll))
        assert np.abs(gamma - g).max() <= 1e-13 and np.abs(X2 - Xi).max() <= 1e-13 and sa[0] == sb[0] == sp[0] == 0
        first = [lo for lo, _ in Q.spans(lengths)]
        assert np.abs(pi_new - g[first].sum(axis=0) / len(lengths)).max() <= 1e-13
    vp, scores, back = Q.viterbi(logb, R.log0(pi), R.log0(A), lengths)
    assert margin > 1e-6 and np.array_equal(vp, path) and len(scores) == len(lengths) and not back[first].any()
    if len(lengths) == 1:                                   # one sequence: the single-sequence restatement, bit for bit
        assert np.array_equal(al, R.forward(e, m, pi, A, R=2)[0]) and np.array_equal(be, R.backward(e, A, R=2)[0])
        assert np.array_equal(Q.posterior(al, be, e, A, lengths)[3], R.posterior(al, be, e, A)[3])
        assert np.array_equal(Q.posterior(al, be, e, A, lengths)[1], R.posterior(al, be, e, A)[1])


@pytest.mark.parametrize("name,K,Rr", [("ones", 1, 64), ("pair", 2, 64), ("mixed", 17, 7), ("mixed", 2, 64), ("tail", 17, 64),
                                       ("many", 17, 7), ("single", 17, 64)])
def test_within_long_double_bounds_and_sums(name, K, Rr):
    lengths, e, m, pi, A = Q.chain(name, K)
    N, S = len(e), len(lengths)
    ref = Q.recurrence_bounds(e, m, pi, A, lengths, Rr)
    al, be, ll, sa, sb = _passes(lengths, e, m, pi, A, Rr)
    w = [R.within(al, ref["alpha"], ref["b_alpha"], "alpha"), R.within(be, ref["beta"], ref["b_beta"], "beta"),
         R.within(ll, ref["ll"], ref["b_ll"], "ll")]
    post = Q.posterior_bounds(ref["alpha"], ref["beta"], e, A, ref["rho_a"], ref["rho_b"], lengths)
    gamma, Xi, A_new, pi_new, sp = Q.posterior(al, be, e, A, lengths)
    w += [R.within(gamma, post["gamma"], post["b_gamma"], "gamma"), R.within(Xi, post["xi"], post["b_xi"], "Xi"),
          R.within(A_new, post["A_new"], post["b_A_new"], "A_new"), R.within(pi_new, post["pi_new"], post["b_pi_new"], "pi_new")]
    print(f"{name} {lengths[:6]}, K = {K}, block_rows {Rr}: worst |err|/bound alpha, beta, ll, gamma, Xi, A_new, pi_new = "
          + ", ".join(f"{x:.3g}" for x in w))
    assert sa == sb == [0, R.NO_ROW] and sp == [0, R.NO_ROW]
    assert np.abs(gamma.astype(R.LD).sum(axis=1) - 1).max() <= post["b_gamma_sum"]
    assert abs(float(Xi.astype(R.LD).sum()) - (N - S)) <= post["b_xi_sum"]
    assert abs(float(pi_new.astype(R.LD).sum()) - 1) <= 2 * K * R.U + (S + 1) * R.U
    assert R.rejects(al * (1 + 1e-9), ref["alpha"], ref["b_alpha"])     # the bounds are no blank cheque


def test_blocked_helper_is_the_restatement():
    """_hmm_seq_ref._blocked with a sequence's own cuts is _hmm_ref's blocked recurrence bit for bit: the defect
    "blocks_on_stacked_rows" differs from the reference in its cuts alone"""
    for n, K, Rr in ((129, 5, 7), (65, 17, 64), (64, 3, 64), (130, 2, 64)):
        e, m, pi, A = R.random_chain(n, K, 3, "sticky")
        a, ll = Q._blocked(e, m, pi, A, True, Q.own_cuts(n, Rr), np.float64)
        b = Q._blocked(e, None, None, A, False, Q.own_cuts(n, Rr), np.float64)[0]
        ra, rll, _ = R.forward(e, m, pi, A, R=Rr)
        assert np.array_equal(a, ra) and np.array_equal(ll, rll) and np.array_equal(b, R.backward(e, A, R=Rr)[0])
    assert Q._stacked_cuts(194, 323, 64) == [0, 62, 126, 129] and Q._stacked_cuts(64, 128, 64) == [0, 64] == Q.own_cuts(64, 64)


# ---- the checks reject the named defects, on the GPU test's own inputs -------------------------------------------------------

def test_defect_list():
    assert Q.DEFECTS == ("no_reset_at_start", "beta_not_reset", "boundary_pair_counted", "pi_first_sequence_only",
                         "pi_not_divided", "blocks_on_stacked_rows", "viterbi_crosses_boundary", "initial_A_counts_boundary")


@pytest.mark.parametrize("name", ["mixed", "tail", "many"])
@pytest.mark.parametrize("kind", ["sticky", "left_to_right"])
def test_recursion_defects_rejected(name, kind):
    """check 3 of the GPU tests (the long double bounds) on the sticky and left-to-right chains of its check 4"""
    lengths, e, m, pi, A = Q.chain(name, 17 if name != "many" else 2, 3, kind)
    for Rr in (64, 7):
        ref = Q.recurrence_bounds(e, m, pi, A, lengths, Rr)
        assert R.rejects(Q.forward(e, m, pi, A, lengths, "no_reset_at_start", R_=Rr)[0], ref["alpha"], ref["b_alpha"])
        assert R.rejects(Q.forward(e, m, pi, A, lengths, "no_reset_at_start", R_=Rr)[1], ref["ll"], ref["b_ll"])
        assert R.rejects(Q.backward(e, A, lengths, "beta_not_reset", R_=Rr)[0], ref["beta"], ref["b_beta"])


@pytest.mark.parametrize("name,K,Rr", [("mixed", 17, 64), ("mixed", 2, 7), ("tail", 17, 64)])
def test_blocks_on_stacked_rows_rejected(name, K, Rr):
    """check 1 of the GPU tests (bit-equality with the sequence alone): blocks cut from the stack's first row stay inside
    the bounds and change the bits of a sequence that does not start on a multiple of block_rows (one of three blocks or
    more: with two the second takes the first's own recursion and nothing is combined)"""
    lengths, e, m, pi, A = Q.chain(name, K)
    ref = Q.recurrence_bounds(e, m, pi, A, lengths, Rr)
    al, be, ll, _, _ = _passes(lengths, e, m, pi, A, Rr)
    wa, wb, wl, _, _ = _passes(lengths, e, m, pi, A, Rr, "blocks_on_stacked_rows")
    assert not R.rejects(wa, ref["alpha"], ref["b_alpha"])
    hit = [s for s, (lo, hi) in enumerate(Q.spans(lengths)) if not (np.array_equal(al[lo:hi], wa[lo:hi])
                                                                     and np.array_equal(be[lo:hi], wb[lo:hi]))]
    moved = [s for s, (lo, hi) in enumerate(Q.spans(lengths)) if Q._stacked_cuts(lo, hi, Rr) != Q.own_cuts(hi - lo, Rr)]
    print(f"{name}, K = {K}, block_rows {Rr}: sequences whose cuts move {moved}, whose bits change {hit}")
    assert hit and set(hit) <= set(moved)


@pytest.mark.parametrize("name,K", [("mixed", 17), ("tail", 2), ("many", 17), ("ones", 2)])
def test_posterior_defects_rejected(name, K):
    lengths, e, m, pi, A = Q.chain(name, K, 3, "sticky")
    ref = Q.recurrence_bounds(e, m, pi, A, lengths)
    post = Q.posterior_bounds(ref["alpha"], ref["beta"], e, A, ref["rho_a"], ref["rho_b"], lengths)
    al, be, _, _, _ = _passes(lengths, e, m, pi, A)
    N, S = len(e), len(lengths)
    _, Xi, A_new, _, _ = Q.posterior(al, be, e, A, lengths, "boundary_pair_counted")
    assert R.rejects(Xi, post["xi"], post["b_xi"]) and abs(Xi.sum() - (N - S)) > post["b_xi_sum"]
    for defect in ("pi_first_sequence_only", "pi_not_divided"):
        assert R.rejects(Q.posterior(al, be, e, A, lengths, defect)[3], post["pi_new"], post["b_pi_new"]), defect


@pytest.mark.parametrize("name,K", [("mixed", 17), ("tail", 2), ("many", 17)])
def test_viterbi_crosses_boundary_rejected(name, K):
    lengths, e, m, pi, A = Q.chain(name, K, 6, "sticky")
    logb = np.log(e) + m[:, None]
    path, scores, back = Q.viterbi(logb, R.log0(pi), R.log0(A), lengths)
    wp, ws, wb = Q.viterbi(logb, R.log0(pi), R.log0(A), lengths, "viterbi_crosses_boundary")
    first = [lo for lo, _ in Q.spans(lengths)][1:]
    assert not np.array_equal(wb, back) and wb[first].any() and not back[first].any()
    assert not np.array_equal(ws, scores) and abs(ws[0] - Q.sum_ascending(scores)) > 1e-6


@pytest.mark.parametrize("name", sorted(Q.FITS))
def test_planted_fits_and_their_defects(name):
    """check 5 of the GPU tests: the measured gates (_hmm_ref.outside) put every defect that changes a number outside"""
    X, z, lengths, start, f64, ld, gates = Q.planted(name)
    a0, a1 = R.ari(z, start), R.ari(z, f64["path"])
    closest = float(np.abs(f64["changes"] - 1e-3).min())
    print(f"{name} {lengths[:4]}: k-means ARI {a0:.3f}, Viterbi ARI {a1:.3f}, {f64['n_iter']} iterations ({f64['why']}), closest "
          f"stop decision {closest:.2e} from tol; f64 - long double: " + ", ".join(f"{k} {v:.3g}" for k, v in gates.items()))
    assert a0 <= 0.7 and a1 >= 0.9 and f64["converged"] and f64["n_iter"] == ld["n_iter"] and gates["path"] == 0
    assert closest > 1e-5 and all(R.GATE_FACTOR * gates[q] < 1e-9 for q in R.QUANTITIES)
    assert all(gates[q] > 0 for q in R.QUANTITIES), "a gate of zero would ask for bit equality"
    assert f64["path_score"] == Q.sum_ascending(f64["path_scores"]) and len(f64["path_scores"]) == len(lengths)
    assert not R.outside(R.differences(Q.fit(X, start, 4, lengths, R_=R.BLOCK_ROWS), f64), gates)
    for defect in ("no_reset_at_start", "beta_not_reset", "boundary_pair_counted", "pi_first_sequence_only", "pi_not_divided",
                   "initial_A_counts_boundary"):
        bad = R.outside(R.differences(Q.fit(X, start, 4, lengths, defect=defect), f64), gates)
        print(f"  {defect}: outside the gate: {bad}")
        assert "pi" in bad and "log_likelihoods" in bad
    A0 = Q.initial_transitions(start, 4, lengths)
    assert not np.array_equal(A0, Q.initial_transitions(start, 4, lengths, "initial_A_counts_boundary"))
    assert np.array_equal(Q.initial_transitions(start, 4, (len(start),)), R.initial_transitions(start, 4))


def test_held_out_video_is_labelled_by_the_restatement():
    X, z, lengths, f, path, ari = Q.videos()
    print(f"three planted videos {lengths}: fit on the first two ({f['n_iter']} iterations, {f['why']}), the third's Viterbi path "
          f"under it has ARI {ari:.4f}")
    assert f["converged"] and ari >= 0.98


# ---- the header, the sizes and the host side ---------------------------------------------------------------------------------

NEW = ("rbvae_hmm_seq_ok", "rbvae_hmm_seq_plan_bytes", "rbvae_hmm_seq_plan", "rbvae_hmm_seq_ws_bytes", "rbvae_hmm_seq_forward",
       "rbvae_hmm_seq_backward", "rbvae_hmm_seq_posterior", "rbvae_hmm_seq_viterbi")


def test_header_and_library():
    protos = sfv._lib.parse_header()
    raw = ctypes.CDLL(sfv._lib.LIB_PATH)
    for name in NEW:
        assert name in protos and hasattr(raw, name), name
    # the single-sequence entries' arguments (3, -, -, 3, 14, 11, 15, 10) with plan and S
    assert [len(protos[n][1]) for n in NEW] == [4, 3, 7, 4, 16, 13, 17, 12]
    names = lambda n: [a for _, a in protos[n][1]]          # noqa: E731
    assert names("rbvae_hmm_seq_forward")[6:9] == ["block_rows", "plan", "S"] and names("rbvae_hmm_seq_backward")[4:7] == ["block_rows", "plan", "S"]
    assert names("rbvae_hmm_seq_posterior")[4:7] == ["K", "plan", "S"] and names("rbvae_hmm_seq_viterbi")[2:5] == ["K", "plan", "S"]
    q = sfv._lib.query
    assert q("rbvae_version") >= 110
    for N, Ld, K, S in ((12298, 50, 17, 16), (2, 1, 1, 2), (2, 1, 1, 3), (2, 1, 1, 0), (600, 3, 64, 300), (63, 3, 64, 2), (300, 129, 4, 2),
                        (1 << 20, 128, 64, 1 << 20), ((1 << 20) + 1, 2, 2, 2)):
        assert q("rbvae_hmm_seq_ok", N, Ld, K, S) == int(Q.ok(N, Ld, K, S)), (N, Ld, K, S)
    for N, K, S, Rr in ((12298, 17, 16, 64), (600, 64, 300, 64), (600, 2, 300, 7), (2, 1, 2, 64), (4098, 17, 2, 7), (129, 17, 1, 64),
                        (129, 17, 1, 1000), (1 << 20, 64, 30000, 64)):
        assert q("rbvae_hmm_seq_plan_bytes", N, S, Rr) == Q.plan_bytes(N, S, Rr), (N, S, Rr)
        assert q("rbvae_hmm_seq_ws_bytes", N, K, S, Rr) == Q.ws_bytes(N, K, S, Rr), (N, K, S, Rr)
    assert q("rbvae_hmm_seq_plan_bytes", 8, 9, 64) == 0 and q("rbvae_hmm_seq_plan_bytes", 8, 0, 64) == 0
    assert q("rbvae_hmm_seq_plan_bytes", 8, 2, 0) == 0 and q("rbvae_hmm_seq_ws_bytes", 8, 9, 2, 64) == 0
    assert q("rbvae_hmm_seq_ws_bytes", 8, 2, 9, 64) == 0 and q("rbvae_hmm_seq_ws_bytes", 8, 2, 2, 0) == 0
    for lengths, Rr in (((1, 63, 64, 65, 1, 129), 64), ((2, 1, 3), 7), ((129,), 1000)):
        p = Q.plan(lengths, Rr)
        N, S = sum(lengths), len(lengths)
        assert 4 * len(p) == Q.plan_bytes(N, S, Rr) and p[3] == sum(-(-n // min(Rr, N)) for n in lengths) <= Q.max_blocks(N, S, Rr)


def test_plan_refuses_bad_lengths_before_anything_is_copied():
    """the host lengths are checked first: these calls return before the plan's memory is looked at"""
    lib = sfv._lib.lib()
    room = np.zeros(1024, dtype=np.int32)

    def plan(lengths, N, Rr=64, S=None, nbytes=4096, where=room.ctypes.data):
        h = np.ascontiguousarray(lengths, dtype=np.int32)
        return lib.rbvae_hmm_seq_plan(h.ctypes.data, len(h) if S is None else S, N, Rr, where, nbytes, None)

    for lengths, N, match in (((3, 0, 5), 8, "lengths[1]=0"), ((3, -1, 6), 8, "lengths[1]=-1"), ((3, 4), 8, "add to 7"),
                              ((3, 6), 8, "more than N=8")):
        assert plan(lengths, N) == sfv._lib.E_INVALID and match in lib.rbvae_last_error().decode(), lengths
    assert plan((3, 5), 8, nbytes=Q.plan_bytes(8, 2, 64) - 1) == sfv._lib.E_INVALID and b"plan of" in lib.rbvae_last_error()
    assert plan((3, 5), 8, where=None) == sfv._lib.E_INVALID and plan((3, 5), 8, Rr=0) == sfv._lib.E_INVALID
    assert plan((1,) * 9, 8) == sfv._lib.E_UNSUPPORTED and plan((8,), 8, S=0) == sfv._lib.E_UNSUPPORTED
    assert not room.any()


def test_host_side_of_the_package():
    M = sfv.hmm_model
    assert M._lengths(None, 5, "x") is None and M._lengths([2, np.int64(3)], 5, "x") == (2, 3)
    for bad in ((), (5, 0), (2, 2), (6, -1)):
        with pytest.raises(ValueError, match="lengths"):
            M._lengths(bad, 5, "x")
    path = np.array([0, 0, 1, 1, 0, 2, 2, 0])
    assert M.change_points(path) == [2, 4, 5, 7] and M.change_points(path, (4, 1, 3)) == [2, 7] == Q.change_points(path, (4, 1, 3))
    assert M.change_points(torch.from_numpy(path), (8,)) == [2, 4, 5, 7] and M.change_points(path, (2, 6)) == [4, 5, 7]
    with pytest.raises(ValueError, match="lengths"):
        M.change_points(path, (4, 3))
    assert M._sum_ascending([1e16, 1.0, 1.0]) == Q.sum_ascending([1e16, 1.0, 1.0]) == 1e16
    fit = sfv.HMMResult(*([None] * 13))
    assert fit.lengths is None and fit.path_scores is None and sfv.BHMMResult(*([None] * 13)).path_scores is None
    X = torch.zeros((8, 4))
    lb = torch.zeros((8, 2), dtype=torch.float64)
    for call in (lambda: sfv.hmm(X, 2, lengths=(3, 5)), lambda: sfv.hmm_select(X, [2], lengths=(3, 5)),
                 lambda: sfv.hmm_forward_backward(lb, [0.5, 0.5], np.eye(2), lengths=(3, 5)),
                 lambda: sfv.hmm_viterbi(lb, [0.5, 0.5], np.eye(2), lengths=(3, 5)), lambda: sfv.bhmm(X, 2, lengths=(3, 5)),
                 lambda: sfv.latent_hmm_videos(None, [torch.zeros((2, 3, 8, 8))] * 2, [[0, 1]] * 2, [[1]] * 2)):
        with pytest.raises(ValueError, match="GPU"):
            call()
    with pytest.raises(ValueError, match="as many"):
        sfv.latent_hmm_videos(None, [X, X], [[0]], [[1], [1]])
    with pytest.raises(ValueError, match="holdout"):
        sfv.latent_hmm_videos(None, [X, X], [[0], [0]], [[1], [1]], holdout=2)
    assert sfv.hmm_sequence_scores is M.hmm_sequence_scores and sfv.latent_hmm_videos is M.latent_hmm_videos
