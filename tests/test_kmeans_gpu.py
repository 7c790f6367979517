"""GPU: the k-means kernels (csrc/kmeans.hip) against tests/_kmeans_ref.py's restatement inside sentinel guard bands -- d2,
centres, within, spread and the k-means++ potentials element-wise within the bounds its docstring derives, labels, counts
and `changed` exact -- and symbols.py end to end against the scikit-learn fixture tests/golden/kmeans.npz
(tools/make_kmeans_golden.py).

Measured on one MI355X: no undecided row on any assign case and every label equal; d2 at most 0.40 of its bound (at
(16 385, 2, 3); 0.28 at (65, 3, 4), 0.06 to 0.08 on the cases of 50 and 128 values); `changed` exact; the centres equal to
the correctly rounded long double means on every case (the sums of a few thousand f32 values are exact in f64), `within`
at most 0.50 and `spread` 0.64 of `n_k u` times their value (both at (300, 128, 256)), and 0.02 and 0.04 of the bounds
with d2's own where cluster_sums takes the distances itself; the k-means++ minima at most
0.40 and the potentials 0.026 of theirs.  On the eight fixture cases init indices, labels and n_iter equal scikit-learn's,
centres within 4.4e-16 and inertia within 3.3e-16 relative (gates 1e-12); the agreement scores differ by 0.0 (gate 1e-15),
Davies-Bouldin by at most 2.2e-14 and Calinski-Harabasz by 3.6e-15 (gates 1e-12).  The 69 tests take
about 3 s together; no case takes more than 0.2 s.
"""
import os

import numpy as np
import pytest
import torch

import _kmeans_ref as R
import sfv_amd as sfv

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GUARD = 4096
SENT = {torch.float64: (torch.int64, 0x7FF8DEADDEADBEEF), torch.int32: (torch.int32, -0x21524111)}
KS, SEEDS = (2, 8, 17, 32), (0, 42)
TOL_CASE = (8, 42, 0.1)                 # test_kmeans_cpu.py: the restatement stops on the shift at iteration 11


class Guarded:
    """n elements of dtype inside GUARD sentinel elements on each side (a NaN sentinel for f64)"""

    def __init__(self, dtype, *shape):
        self.n = int(np.prod(shape))
        raw, self.sent = SENT[dtype]
        self.buf = torch.full((GUARD + self.n + GUARD,), self.sent, dtype=raw, device="cuda")
        self.t = self.buf[GUARD:GUARD + self.n].view(dtype).view(*shape)

    def check(self, what, untouched=False, full=True):
        bits = self.buf.cpu().numpy()
        inner = np.zeros(bits.shape, dtype=bool)
        inner[GUARD:GUARD + self.n] = True
        stray = np.nonzero((bits != self.sent) & ~inner)[0]
        assert stray.size == 0, f"{what}: {stray.size} elements outside the output were written; first at {stray[0] - GUARD}"
        unwritten = np.nonzero((bits == self.sent) & inner)[0]
        if untouched:
            assert unwritten.size == self.n, f"{what}: a refused call wrote {self.n - unwritten.size} elements"
        elif full:
            assert unwritten.size == 0, f"{what}: {unwritten.size} elements never written; first at {unwritten[0] - GUARD}"
        return self.t.cpu().numpy()


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def _state():
    return torch.zeros(4, dtype=torch.int32, device="cuda")


def _ws(N, Ld, K):
    return Guarded(torch.float64, sfv._lib.query("rbvae_kmeans_ws_bytes", N, Ld, K) // 8)


@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(os.path.join(HERE, "golden", "kmeans.npz")))
    g.update({k: v for k, v in np.load(os.path.join(HERE, "golden", "latent_scores.npz")).items() if k in ("X", "lab", "lab_edge")})
    g["Xd"] = _dev(g["X"])
    return g


def _init(gold, K, seed):
    return gold["X"][gold[f"pp_{K}_{seed}"]].astype(np.float64)


# ---- assign ------------------------------------------------------------------------------------------------------------------

def _assign(X, C, prev=None, own=None, state=None):
    N, Ld = X.shape
    K = len(C)
    label, d2 = Guarded(torch.int32, N), Guarded(torch.float64, N)
    sfv._lib.call("rbvae_kmeans_assign", _dev(X), N, Ld, _dev(C), K, None if prev is None else _dev(prev, torch.int32),
                  None if own is None else _dev(own, torch.int32), label.t, d2.t, state)
    return label.check(f"label ({N}, {Ld}, {K})"), d2.check(f"d2 ({N}, {Ld}, {K})")


@pytest.mark.parametrize("N,Ld,K", R.ASSIGN_CASES)
def test_assign(N, Ld, K):
    X, C = R.assign_case(N, Ld, K)
    assert sfv._lib.query("rbvae_kmeans_ok", N, Ld, K) == 1
    if Ld == 128:                                           # 33 centres just cross one LDS chunk, 256 span eight
        assert sfv._lib.query("rbvae_kmeans_chunk_centres", Ld) == R.chunk_centres(Ld) == 32
    D = R.d2_to(X, C, R.LD)
    ref = D.min(axis=1).astype(np.float64)
    decided = R.decided(D, Ld)
    state = _state()
    label, d2 = _assign(X, C, state=state)
    w = R.within(d2, ref, R.d2_bound(Ld, ref), f"d2 ({N}, {Ld}, {K})")
    assert int((~decided).sum()) == 0
    assert np.array_equal(label, np.argmin(D, axis=1))
    assert state.cpu().tolist() == [0, 0, 0, N]             # no previous labels: every row counts as moved
    print(f"assign ({N}, {Ld}, {K}): 0 undecided rows, d2 worst |err|/bound {w:.3g}")
    prev = label.copy()
    moved = np.random.RandomState(N).rand(N) < 0.3
    prev[moved] = (prev[moved] + 1) % (K + 1) - (K == 1)    # another value, K (no centre) included
    state = _state()
    label2, d22 = _assign(X, C, prev=prev, state=state)
    assert state.cpu().tolist() == [0, 0, 0, int((prev != label).sum())]
    assert np.array_equal(label, label2) and np.array_equal(d2.view(np.int64), d22.view(np.int64)), "two runs differ"
    label3, d23 = _assign(X, C)                             # without a state
    assert np.array_equal(label, label3) and np.array_equal(d2.view(np.int64), d23.view(np.int64))
    own = np.random.RandomState(K).randint(0, K, N).astype(np.int32)
    lo, do = _assign(X, C, own=own)
    ref_o = D[np.arange(N), own].astype(np.float64)
    assert np.array_equal(lo, own)
    R.within(do, ref_o, R.d2_bound(Ld, ref_o), "d2 to the own centre")
    done = _state()
    done[0] = 1
    label4, d24 = Guarded(torch.int32, N), Guarded(torch.float64, N)
    sfv._lib.call("rbvae_kmeans_assign", _dev(X), N, Ld, _dev(C), K, None, None, label4.t, d24.t, done)
    label4.check("label behind done", untouched=True)
    d24.check("d2 behind done", untouched=True)
    assert done.cpu().tolist() == [1, 0, 0, 0]


def test_assign_exact_ties():
    """duplicated centres and small-integer coordinates: d2 is exact and every tie goes to the lower centre"""
    X, C = R.tie_case()
    ref, ref_d2 = R.assign(X, C)
    high = R.assign(X, C, "tie_high")[0]
    state = _state()
    label, d2 = _assign(X, C, prev=high, state=state)
    assert np.array_equal(label, ref) and not np.array_equal(label, high)
    assert np.array_equal(d2, ref_d2)
    assert state.cpu().tolist() == [0, 0, 0, int((high != ref).sum())]


# ---- update ------------------------------------------------------------------------------------------------------------------

def _update(X, lab, d2, C_old, state=None):
    N, Ld = X.shape
    K = len(C_old)
    C, count = Guarded(torch.float64, K, Ld), Guarded(torch.int32, K)
    shift2, within, spread = (Guarded(torch.float64, K) for _ in range(3))
    C.t.copy_(_dev(C_old))
    ws = _ws(N, Ld, K)
    sfv._lib.call("rbvae_kmeans_update", _dev(X), N, Ld, _dev(lab, torch.int32), None if d2 is None else _dev(d2), K, C.t,
                  count.t, shift2.t, within.t, spread.t, ws.t, state)
    ws.check("workspace", full=False)
    what = f"({N}, {Ld}, {K})"
    return (C.check("centres " + what), count.check("count " + what), shift2.check("shift2 " + what),
            within.check("within " + what), spread.check("spread " + what))


@pytest.mark.parametrize("kind", ["random", "empty", "one", "striped"])
@pytest.mark.parametrize("N,Ld,K", R.ASSIGN_CASES)
def test_update(N, Ld, K, kind):
    X, C_old = R.assign_case(N, Ld, K)
    lab = R.update_labels(N, K, kind)
    if kind == "random" and N > 8:
        lab[5], lab[6] = -1, K                              # no cluster: skipped
    d2 = np.random.RandomState(N + K).rand(N) * 3.0
    C, count, shift2, within, spread = _update(X, lab, d2, C_old)
    rC, rn, _, rw, rs = R.update(X, lab, C_old, d2)
    assert np.array_equal(count, rn)
    empty = rn == 0
    if kind == "empty" and K > 1:
        assert empty.any()
    wc = R.within(C, rC, R.centre_bound(X, lab, rC), f"centres ({N}, {Ld}, {K}, {kind})")
    assert np.array_equal(C[empty].view(np.int64), C_old[empty].view(np.int64)), "an empty cluster's centre moved"
    assert np.all(shift2[empty] == 0.0) and np.all(within[empty] == 0.0) and np.all(spread[empty] == 0.0)
    rs2 = ((C - C_old).astype(R.LD) ** 2).sum(1).astype(np.float64)         # from the device's own centres
    R.within(shift2, rs2, (Ld + 4) * R.U * rs2 + R.TINY, "shift2")        # the difference, the square, L additions
    bw, bs = R.sum_bounds(rn, rw, rs)
    ww, wsp = R.within(within, rw, bw, "within"), R.within(spread, rs, bs, "spread")
    print(f"update ({N}, {Ld}, {K}, {kind}): clusters of {rn.min()}..{rn.max()} rows, worst |err|/bound centres {wc:.3g}, "
          f"within {ww:.3g}, spread {wsp:.3g}")
    again = _update(X, lab, d2, C_old)
    for a, b in zip((C, count, shift2, within, spread), again):
        assert np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a, b.view(np.int64) if b.dtype == np.float64 else b)
    if kind == "random":
        C0, n0, _, w0, s0 = _update(X, lab, None, C_old)    # without d2: the centres alone
        assert np.array_equal(C0.view(np.int64), C.view(np.int64)) and np.array_equal(n0, count)
        assert np.all(w0 == 0.0) and np.all(s0 == 0.0)


def test_update_across_all_row_blocks():
    """more than 256 x 256 rows: 256 row blocks of several hundred rows each, every cluster in all of them"""
    N, Ld, K = 70001, 3, 5
    X = R.soft_rows(N, Ld, 11)
    lab = R.update_labels(N, K, "striped")
    d2 = np.random.RandomState(3).rand(N)
    C_old = np.zeros((K, Ld))
    C, count, shift2, within, spread = _update(X, lab, d2, C_old)
    rC, rn, _, rw, rs = R.update(X, lab, C_old, d2)
    assert np.array_equal(count, rn) and rn.min() >= 14000
    R.within(C, rC, R.centre_bound(X, lab, rC), "centres")
    bw, bs = R.sum_bounds(rn, rw, rs)
    R.within(within, rw, bw, "within")
    R.within(spread, rs, bs, "spread")


def test_decide():
    shift2 = _dev(np.array([0.25, 0.5, 0.125]))
    for changed, tol_abs, max_iter, n_iter, want in ((0, 0.0, 9, 4, [1, 5, 1, 0]), (3, 0.875, 9, 4, [1, 5, 2, 0]),
                                                     (3, 0.874, 9, 4, [0, 5, 0, 0]), (3, 0.0, 5, 4, [1, 5, 3, 0]),
                                                     (0, 1.0, 5, 4, [1, 5, 1, 0])):
        state = _dev(np.array([0, n_iter, 0, changed], dtype=np.int32))
        sfv._lib.call("rbvae_kmeans_decide", shift2, 3, tol_abs, max_iter, state)
        assert state.cpu().tolist() == want, (changed, tol_abs, max_iter)
        sfv._lib.call("rbvae_kmeans_decide", shift2, 3, tol_abs, max_iter, state)
        if want[0]:
            assert state.cpu().tolist() == want             # done: nothing moves any more


# ---- k-means++ ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,Ld", [(1, 1), (65, 3), (257, 50), (300, 128), (16385, 2)])
def test_pp_trials(N, Ld):
    X = R.soft_rows(N, Ld, N + Ld)
    r = np.random.RandomState(N)
    T = 8
    cand = r.randint(0, N, T).astype(np.int32)
    cand[3] = cand[1]                                       # the same candidate twice
    D = R.d2_to(X, X[cand], R.LD).T                         # [T, N]
    for first in (True, False):
        closest = np.full(N, np.inf) if first else R.d2_to(X, X[r.randint(0, N, 1)])[:, 0] + 1e-3 * r.rand(N)
        out, pot = Guarded(torch.float64, T, N), Guarded(torch.float64, T)
        ws = _ws(N, Ld, 1)
        sfv._lib.call("rbvae_kmeans_pp_trials", _dev(X), N, Ld, _dev(cand), T, _dev(closest), out.t, pot.t, ws.t)
        ws.check("workspace", full=False)
        got, gp = out.check(f"minima ({N}, {Ld})"), pot.check(f"potentials ({N}, {Ld})")
        ref = np.minimum(closest[None, :].astype(R.LD), D)
        rp = ref.sum(1).astype(np.float64)
        ref = ref.astype(np.float64)
        w = R.within(got, ref, R.d2_bound(Ld, ref), "minima")
        wp = R.within(gp, rp, (N + Ld + 3) * R.U * rp + R.TINY, "potentials")
        print(f"k-means++ trials ({N}, {Ld}), first = {first}: worst |err|/bound minima {w:.3g}, potentials {wp:.3g}")
        assert np.array_equal(got[3].view(np.int64), got[1].view(np.int64)) and gp[3] == gp[1]
    bad = cand.copy()
    bad[0], bad[2] = -1, N                                  # no row: the minima stay what they were
    out, pot = Guarded(torch.float64, T, N), Guarded(torch.float64, T)
    sfv._lib.call("rbvae_kmeans_pp_trials", _dev(X), N, Ld, _dev(bad), T, _dev(closest), out.t, pot.t, _ws(N, Ld, 1).t)
    got2 = out.check("minima with candidates that are no row")
    assert np.array_equal(got2[0], closest) and np.array_equal(got2[2], closest)
    assert np.array_equal(got2[[1, 3, 4, 5, 6, 7]].view(np.int64), got[[1, 3, 4, 5, 6, 7]].view(np.int64))


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("K", KS)
def test_kmeans_plusplus_against_sklearn(gold, K, seed):
    idx = sfv.kmeans_plusplus(gold["Xd"], K, seed)
    assert idx.dtype == np.int64 and np.array_equal(idx, gold[f"pp_{K}_{seed}"])


# ---- the whole fit --------------------------------------------------------------------------------------------------------------

def _same(a, b):
    return (torch.equal(a.labels, b.labels) and torch.equal(a.centers.view(torch.int64), b.centers.view(torch.int64))
            and a.inertia == b.inertia and a.n_iter == b.n_iter and a.converged == b.converged
            and np.array_equal(a.counts, b.counts))


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("K", KS)
def test_fit_against_sklearn(gold, K, seed):
    t = f"{K}_{seed}"
    fit = sfv.kmeans(gold["Xd"], K, init=_init(gold, K, seed))
    assert fit.labels.dtype == torch.int32 and fit.labels.is_cuda and fit.centers.dtype == torch.float64
    assert np.array_equal(fit.labels.cpu().numpy(), gold["labels_" + t])
    assert fit.n_iter == int(gold["n_iter_" + t]) and fit.converged == "strict"
    dc = np.abs(fit.centers.cpu().numpy() - gold["centers_" + t]).max()
    di = abs(fit.inertia / float(gold["inertia_" + t]) - 1.0)
    print(f"K = {K}, seed {seed}: {fit.n_iter} iterations, centres within {dc:.3g} of scikit-learn's, inertia within {di:.3g}")
    assert dc <= 1e-12 and di <= 1e-12
    assert np.array_equal(fit.counts, np.bincount(gold["labels_" + t], minlength=K)) and fit.n_empty == 0
    assert _same(fit, sfv.kmeans(gold["Xd"], K, init=_init(gold, K, seed))), "two runs differ"
    own = sfv.kmeans(gold["Xd"], K, seed=seed)              # with its own k-means++ start
    assert _same(fit, own)


def test_fit_stops_on_tol(gold):
    K, seed, tol = TOL_CASE
    ref = R.lloyd(gold["X"], _init(gold, K, seed), tol=tol)
    fit = sfv.kmeans(gold["Xd"], K, init=_init(gold, K, seed), tol=tol)
    assert ref["converged"] == "tol" and fit.converged == "tol" and fit.n_iter == ref["n_iter"] == 11
    label, _ = _assign(gold["X"], fit.centers.cpu().numpy())
    assert np.array_equal(fit.labels.cpu().numpy(), label)  # the labels of the final centres
    assert np.array_equal(label, ref["labels"])
    assert not np.array_equal(label, R.lloyd(gold["X"], _init(gold, K, seed), tol=tol, defect="no_final_assign_after_tol")["labels"])
    assert np.abs(fit.centers.cpu().numpy() - ref["centers"]).max() <= 1e-12 and abs(fit.inertia / ref["inertia"] - 1.0) <= 1e-12


def test_fit_stops_on_max_iter(gold):
    K, seed = 8, 42
    ref = R.lloyd(gold["X"], _init(gold, K, seed), max_iter=3)
    fit = sfv.kmeans(gold["Xd"], K, init=_init(gold, K, seed), max_iter=3)
    assert fit.converged == "max_iter" and fit.n_iter == 3
    assert np.array_equal(fit.labels.cpu().numpy(), ref["labels"])
    assert np.abs(fit.centers.cpu().numpy() - ref["centers"]).max() <= 1e-12 and abs(fit.inertia / ref["inertia"] - 1.0) <= 1e-12


@pytest.mark.parametrize("K,seed", [(32, 0), (8, 42), (17, 0)])
def test_run_ahead_changes_nothing(gold, K, seed):
    """iterations are enqueued eight at a time; those behind the decision must leave everything as it was: the fit equals
    one whose max_iter is exactly the iteration it converged at (5: inside the first batch, 13: inside the second, 8: the
    last of the first)"""
    n = int(gold[f"n_iter_{K}_{seed}"])
    assert n == {32: 5, 8: 13, 17: 8}[K] and sfv.symbols.ENQUEUE == 8
    fit = sfv.kmeans(gold["Xd"], K, init=_init(gold, K, seed))
    exact = sfv.kmeans(gold["Xd"], K, init=_init(gold, K, seed), max_iter=n)
    assert exact.converged == "strict" and _same(fit, exact)
    before = sfv.kmeans(gold["Xd"], K, init=_init(gold, K, seed), max_iter=n - 1)
    assert before.converged == "max_iter" and before.n_iter == n - 1


def test_fit_keeps_an_empty_cluster(gold):
    K, seed = 8, 42
    C0 = np.concatenate([_init(gold, K, seed), np.full((1, 50), 40.0)])      # a ninth centre no row is near
    ref = R.lloyd(gold["X"], C0)
    fit = sfv.kmeans(gold["Xd"], K + 1, init=C0)
    assert fit.n_empty == 1 and fit.counts[K] == 0 and fit.n_iter == ref["n_iter"] and fit.converged == "strict"
    assert np.array_equal(fit.labels.cpu().numpy(), ref["labels"])
    assert np.array_equal(fit.centers.cpu().numpy()[K], C0[K])
    assert np.array_equal(fit.labels.cpu().numpy(), gold[f"labels_{K}_{seed}"])


# ---- plumbing and scores ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", [1, 6, 50])
def test_code_symbols_against_numpy(gold, m):
    sym, uniq, cnt = sfv.code_symbols(gold["Xd"][:, :m].contiguous())
    assert sym.dtype == torch.int64 and cnt.dtype == torch.int64 and uniq.dtype == torch.bool
    assert np.array_equal(sym.cpu().numpy(), gold[f"sym_{m}"]) and np.array_equal(uniq.cpu().numpy(), gold[f"uniq_{m}"])
    assert np.array_equal(cnt.cpu().numpy(), gold[f"cnt_{m}"])
    assert len(gold[f"cnt_{m}"]) == {1: 2, 6: 64, 50: 320}[m]


@pytest.mark.parametrize("bits", [33, 128])
def test_code_symbols_of_long_codes(bits):
    r = np.random.RandomState(bits)
    C = r.randint(0, 2, (40, bits))[r.randint(0, 40, 500)].astype(np.float32)
    C[C > 0.5] = 0.501 + 0.499 * r.rand(int((C > 0.5).sum())).astype(np.float32)       # the threshold is 0.5, not 1
    C[0, 0] = 0.5                                           # exactly 0.5 is a 0 bit
    u, inv, cnt = np.unique(C > 0.5, axis=0, return_inverse=True, return_counts=True)
    sym, uniq, counts = sfv.code_symbols(_dev(C))
    assert len(u) <= 41 and cnt.max() > 1
    assert np.array_equal(sym.cpu().numpy(), inv.reshape(-1)) and np.array_equal(uniq.cpu().numpy(), u)
    assert np.array_equal(counts.cpu().numpy(), cnt)


def test_contingency_and_agreement_against_sklearn(gold):
    lab = _dev(gold["lab"])
    worst = 0.0
    for name in ["edge"] + [f"{K}_{s}" for K in KS for s in SEEDS]:
        other = gold["lab_edge"] if name == "edge" else gold["labels_" + name]
        B = int(other.max()) + 1
        T = sfv.contingency(lab, _dev(other), 8, B + 2)
        assert T.dtype == torch.int64 and T.is_cuda and np.array_equal(T.cpu().numpy(), R.contingency(gold["lab"], other, 8, B + 2))
        for got in (sfv.clustering_agreement(lab, _dev(other)), sfv.clustering_agreement(gold["lab"], other, 8, B + 2)):
            worst = max([worst] + [abs(got[n] - gold["agree_" + name][i]) for i, n in enumerate(R.SCORES)])
            assert np.array_equal(got["contingency"][:, :B], R.contingency(gold["lab"], other, 8, B))
    print(f"agreement scores: max |device - sklearn| {worst:.3g}")
    assert worst <= 1e-15
    one, two = np.zeros(6, dtype=np.int64), np.array([0, 0, 0, 1, 1, 1])
    for a, b in ((one, one), (two, one), (one, two), (two, two)):
        got, ref = sfv.clustering_agreement(a, b), R.agreement(R.contingency(a, b))
        assert all(got[n] == ref[n] for n in R.SCORES), (a, b)


def test_indices_against_sklearn(gold):
    worst_db = worst_ch = 0.0
    for name in ["lab", "lab_edge"] + [f"{K}_{s}" for K in KS for s in SEEDS]:
        lab = gold[name] if name.startswith("lab") else gold["labels_" + name]
        db, ch = sfv.davies_bouldin(gold["Xd"], lab), sfv.calinski_harabasz(gold["Xd"], _dev(lab))
        worst_db, worst_ch = max(worst_db, abs(db - float(gold["db_" + name]))), max(worst_ch, abs(ch - float(gold["ch_" + name])))
        assert abs(db - float(gold["db_" + name])) <= 1e-12 and abs(ch - float(gold["ch_" + name])) <= 1e-12, name
    print(f"Davies-Bouldin within {worst_db:.3g} of scikit-learn's, Calinski-Harabasz within {worst_ch:.3g}")
    C, n, within, spread = sfv.cluster_sums(gold["Xd"], gold["lab_edge"])
    rC, rn, rw, rs = R.cluster_sums(gold["X"], gold["lab_edge"])
    assert np.array_equal(n, rn) and len(n) == 9            # the gap in lab_edge is closed
    R.within(C, rC, R.centre_bound(gold["X"], np.unique(gold["lab_edge"], return_inverse=True)[1], rC), "centroids")
    assert within[-1] == 0.0 and spread[-1] == 0.0 and n[-1] == 1           # the singleton sits on its centroid
    # within and spread of the device's own d2, against long double sums of long double distances to the same centroids
    dense = np.unique(gold["lab_edge"], return_inverse=True)[1].reshape(-1)
    d2 = R.d2_to(gold["X"], C, R.LD)[np.arange(320), dense]
    rw = np.array([float(d2[dense == k].sum()) for k in range(9)])
    rs = np.array([float(np.sqrt(d2[dense == k]).sum()) for k in range(9)])
    bw, bs = R.sum_bounds(n, rw, rs, 50)
    ww, wsp = R.within(within, rw, bw, "within of the own d2"), R.within(spread, rs, bs, "spread of the own d2")
    print(f"cluster_sums: worst |err|/bound within {ww:.3g}, spread {wsp:.3g}")
    dup = _dev(np.repeat(np.eye(3, dtype=np.float32), 2, axis=0))            # every row on its centroid
    assert sfv.davies_bouldin(dup, np.array([0, 0, 1, 1, 2, 2])) == 0.0
    assert sfv.calinski_harabasz(dup, np.array([0, 0, 1, 1, 2, 2])) == 1.0


def test_latent_symbols():
    F_, RES, LD = 40, 64, 16
    torch.manual_seed(0)
    model = sfv.Seq2SeqBinaryVAE(3, 3, LD, LD, variant="contrastive", input_hw=(RES, RES), compute_dtype="f32").cuda().eval()
    x = torch.rand(F_, 3, RES, RES, generator=torch.Generator().manual_seed(1)).cuda()
    u = torch.rand(F_, LD, generator=torch.Generator().manual_seed(2))
    flags = [10, 30]
    out = sfv.latent_symbols(model, x, range(F_), flags, u=u)
    scores = sfv.latent_scores(model, x, range(F_), flags, n_neighbors=5, u=u)
    assert torch.equal(out["latents"], scores["latents"]) and torch.equal(out["codes"], scores["codes"])
    assert np.array_equal(out["labels"], scores["labels"]) and not model.training
    km = out["kmeans"]
    assert km.centers.shape == (3, LD) and km.counts.sum() == F_ and _same(km, sfv.kmeans(out["latents"], 3))
    sym, uniq, cnt = sfv.code_symbols(out["codes"])
    assert torch.equal(out["symbols"], sym) and torch.equal(out["codes_unique"], uniq) and torch.equal(out["symbol_counts"], cnt)
    for key, other, B in (("kmeans_agreement", km.labels, 3), ("symbol_agreement", sym, len(cnt))):
        ref = sfv.clustering_agreement(out["labels"], other, 3, B)
        assert all(out[key][n] == ref[n] for n in R.SCORES) and all(np.isfinite(out[key][n]) for n in R.SCORES)
    assert out["davies_bouldin_states"] == sfv.davies_bouldin(out["latents"], out["labels"])
    assert out["calinski_harabasz_kmeans"] == sfv.calinski_harabasz(out["latents"], km.labels)
    assert out["davies_bouldin_kmeans"] > 0.0 and out["calinski_harabasz_states"] > 0.0
    proj = {"latents": out["latents"].clone()}
    again = sfv.latent_symbols(model, x, range(F_), flags, projections=proj, u=u, n_clusters=4)
    assert again["latents"] is proj["latents"] or torch.equal(again["latents"], proj["latents"])
    assert again["kmeans"].centers.shape == (4, LD) and again["kmeans_agreement"]["contingency"].shape == (3, 4)


# ---- refused arguments --------------------------------------------------------------------------------------------------------------

def test_refused_arguments_write_nothing():
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")       # noqa: E731
    zd = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")      # noqa: E731
    zi = lambda *s: torch.zeros(s, dtype=torch.int32, device="cuda")        # noqa: E731
    label, d2, state = Guarded(torch.int32, 8), Guarded(torch.float64, 8), Guarded(torch.int32, 4)
    C, count = Guarded(torch.float64, 257, 129), Guarded(torch.int32, 257)
    shift2, within, spread = (Guarded(torch.float64, 257) for _ in range(3))
    out, pot, ws = Guarded(torch.float64, 8, 8), Guarded(torch.float64, 8), Guarded(torch.float64, 8 * 257 * 132)
    X, cen = z(300, 129), zd(257, 129)
    for N, Ld, K, match in ((8, 3, 9, "K=9"), (8, 129, 2, "L=129"), (300, 3, 257, "K=257"), (0, 3, 1, "N=0"),
                            ((1 << 20) + 1, 3, 2, "N=1048577"), (8, 0, 2, "L=0"), (8, 3, 0, "K=0")):
        assert sfv._lib.query("rbvae_kmeans_ok", N, Ld, K) == 0 and sfv._lib.query("rbvae_kmeans_ws_bytes", N, Ld, K) == 0
        with pytest.raises(RuntimeError, match=match):
            sfv._lib.call("rbvae_kmeans_assign", X, N, Ld, cen, K, None, None, label.t, d2.t, state.t)
        with pytest.raises(RuntimeError, match=match):
            sfv._lib.call("rbvae_kmeans_update", X, N, Ld, zi(300), zd(300), K, C.t, count.t, shift2.t, within.t, spread.t,
                          ws.t, None)
    for N, Ld, match in ((8, 129, "L=129"), (0, 3, "N=0"), ((1 << 20) + 1, 3, "N=1048577"), (8, 0, "L=0")):
        with pytest.raises(RuntimeError, match=match):
            sfv._lib.call("rbvae_kmeans_pp_trials", X, N, Ld, zi(8), 8, zd(300), out.t, pot.t, ws.t)
    with pytest.raises(RuntimeError, match="T=9"):
        sfv._lib.call("rbvae_kmeans_pp_trials", X, 8, 3, zi(9), 9, zd(8), out.t, pot.t, ws.t)
    with pytest.raises(RuntimeError, match="K=257"):
        sfv._lib.call("rbvae_kmeans_decide", zd(257), 257, 0.0, 3, state.t)
    with pytest.raises(ValueError, match="null"):
        sfv._lib.call("rbvae_kmeans_assign", X, 8, 3, None, 2, None, None, label.t, d2.t, state.t)
    with pytest.raises(ValueError, match="max_iter=0"):
        sfv._lib.call("rbvae_kmeans_decide", zd(2), 2, 0.0, 0, state.t)
    for g, what in ((label, "label"), (d2, "d2"), (state, "state"), (C, "centres"), (count, "count"), (shift2, "shift2"),
                    (within, "within"), (spread, "spread"), (out, "minima"), (pot, "potentials"), (ws, "workspace")):
        g.check(what, untouched=True)
    bad = z(8, 3)
    bad[2, 1] = float("nan")
    for call in (lambda: sfv.kmeans(bad, 2), lambda: sfv.kmeans_plusplus(bad, 2), lambda: sfv.davies_bouldin(bad, [0] * 4 + [1] * 4)):
        with pytest.raises(ValueError, match="NaN"):
            call()
    for call, match in ((lambda: sfv.kmeans(z(8, 3), 9), "K=9"), (lambda: sfv.kmeans(z(8, 129), 2), "L=129"),
                        (lambda: sfv.kmeans(z(300, 3), 257), "K=257"), (lambda: sfv.kmeans(z(8, 3).cpu(), 2), "GPU"),
                        (lambda: sfv.kmeans(z(8, 3).double(), 2), "float32"), (lambda: sfv.kmeans(z(8, 3), 2, max_iter=0), "max_iter"),
                        (lambda: sfv.kmeans(z(8, 3), 2, init="random"), "init"), (lambda: sfv.kmeans(z(8, 3), 2, init=np.zeros((3, 3))), "init"),
                        (lambda: sfv.code_symbols(z(8, 3).cpu()), "GPU"), (lambda: sfv.contingency(zi(8), zi(8).cpu(), 2, 2), "GPU"),
                        (lambda: sfv.contingency(zi(8), zi(8) + 2, 2, 2), "labels outside"),
                        (lambda: sfv.contingency(zi(8), zi(7), 2, 2), "rows"),
                        (lambda: sfv.clustering_agreement(np.zeros(8), np.zeros(8)), "integers"),
                        (lambda: sfv.davies_bouldin(z(8, 3), np.zeros(8, dtype=np.int64)), "Number of labels is 1"),
                        (lambda: sfv.calinski_harabasz(z(8, 3), np.arange(8)), "Number of labels is 8"),
                        (lambda: sfv.davies_bouldin(z(8, 3), np.arange(7)), "labels must be 8"),
                        (lambda: sfv.latent_symbols(None, z(2, 3, 8, 8), [0], [1]), "frame indices")):
        with pytest.raises(ValueError, match=match):
            call()
