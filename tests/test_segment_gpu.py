"""GPU: the segmentation kernels (csrc/segment.hip) against tests/_segment_ref.py inside sentinel guard bands -- P, Q, out
and arg bit-equal to the f64 restatement and within the bounds its docstring derives of the long double form -- tables and
traces against the brute-force enumeration and the planted boundaries, and segments.py end to end.

Measured on one MI355X: P, Q, out and arg bit-equal to the f64 restatement on every case, the 4097-row one included, and
two runs bit-equal.  Against long double: P exact on every prefix shape (sums of at most 1025 f32 values are exact in
f64), Q at most 0.20 of its bound (at (1025, 2)); the layers' minima at most 0.040 of their bound on the soft cases (at
(130, 128), random prev) and 0.77 on the codes (at (1025, 8), D_2); no soft row undecided; 5 of 128, 1 of 508 and 2 of
1023 code rows undecided from D_2 (exact ties of integer costs, the device's arg a minimiser on each), none from the random
prev; D_1[N] at most 0.016 of its bound against the total sum of squares.  The 43 tests take 4.2 s together; no case
takes more than 0.4 s.
"""
import numpy as np
import pytest
import torch

import _segment_ref as R
import sfv_amd as sfv

pytestmark = pytest.mark.gpu

GUARD = 4096
SENT = {torch.float64: (torch.int64, 0x7FF8DEADDEADBEEF), torch.int32: (torch.int32, -0x21524111)}


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


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _same_scores(a, b):
    """two boundary_agreement dicts, NaN equal to NaN"""
    return a.keys() == b.keys() and all(a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]) for k in a)


def _ws(N, Ld):
    return Guarded(torch.float64, sfv._lib.query("rbvae_segment_ws_bytes", N, Ld) // 8)


# ---- prefix -------------------------------------------------------------------------------------------------------------------

def _prefix(X):
    N, Ld = X.shape
    P, Q = Guarded(torch.float64, N + 1, Ld), Guarded(torch.float64, N + 1)
    sfv._lib.call("rbvae_segment_prefix", _dev(X), N, Ld, P.t, Q.t)
    return P.check(f"P ({N}, {Ld})"), Q.check(f"Q ({N}, {Ld})")


@pytest.mark.parametrize("kind", ["soft", "code"])
@pytest.mark.parametrize("shape", R.PREFIX_SHAPES)
def test_prefix(shape, kind):
    N, Ld = shape
    X, _ = R.case(kind, N, Ld, 2)
    P, Q = _prefix(X)
    rP, rQ = R.prefix(X)
    assert _same(P, rP), f"P differs from the f64 restatement in {int((P != rP).sum())} places"
    assert _same(Q, rQ), f"Q differs from the f64 restatement in {int((Q != rQ).sum())} places"
    Pl, Ql = R.prefix(X, R.LD)
    wp = R.within(P, Pl.astype(np.float64), R.p_bound(X) + R.U * np.abs(P), f"P {shape}")
    wq = R.within(Q, Ql.astype(np.float64), R.q_bound(X) + R.U * np.abs(Q), f"Q {shape}")
    print(f"prefix {shape} {kind}: bit-equal to the restatement; worst |err|/bound P {wp:.3g}, Q {wq:.3g}")
    tP, tQ = sfv.segment_prefix(_dev(X))
    assert _same(tP.cpu().numpy(), P) and _same(tQ.cpu().numpy(), Q)


# ---- layer --------------------------------------------------------------------------------------------------------------------

def _layer(P, Q, prev, m):
    N, Ld = P.shape[0] - 1, P.shape[1]
    out, arg, ws = Guarded(torch.float64, N + 1), Guarded(torch.int32, N + 1), _ws(N, Ld)
    sfv._lib.call("rbvae_segment_layer", _dev(P), _dev(Q), N, Ld, _dev(prev), m, out.t, arg.t, ws.t)
    ws.check(f"workspace ({N}, {Ld})", full=False)
    return out.check(f"out ({N}, {Ld})"), arg.check(f"arg ({N}, {Ld})")


def _report_difference(out, arg, rout, rarg, what):
    bad = np.nonzero((_bits(out) != _bits(rout)) | (arg != rarg))[0]
    t = int(bad[0])
    return (f"{what}: {bad.size} rows differ from the f64 restatement; first t = {t}: device ({out[t]!r}, {arg[t]}), "
            f"restatement ({rout[t]!r}, {rarg[t]})")


@pytest.mark.parametrize("which", ["D2", "random"])
@pytest.mark.parametrize("kind,N,Ld,S,m", R.LAYER_CASES)
def test_layer(kind, N, Ld, S, m, which):
    what = f"layer {(kind, N, Ld, S, m, which)}"
    _, P, Q, prev, rout, rarg = R.layer_case(kind, N, Ld, S, m, which)
    out, arg = _layer(P, Q, prev, m)
    ref = R.layer_case_ld(kind, N, Ld, S, m, which)
    worst, und = R.check_layer(kind, out, arg, ref, what)                   # the gate: bounds, argmins, (+inf, -1) rows
    rows = int((ref["n_cand"] > 0).sum())
    print(f"{what}: worst |err|/bound {worst:.3g}, {und} of {rows} rows undecided")
    assert _same(out, rout) and np.array_equal(arg, rarg), _report_difference(out, arg, rout, rarg, what)
    out2, arg2 = _layer(P, Q, prev, m)
    assert _same(out, out2) and np.array_equal(arg, arg2), "two runs differ"
    tout, targ = sfv.segment_layer(_dev(P), _dev(Q), _dev(prev), m)
    assert _same(tout.cpu().numpy(), out) and np.array_equal(targ.cpu().numpy(), arg)


def test_layer_across_many_tiles_and_runs():
    """4097 rows: 65 end blocks, up to 9 runs of 8 start tiles each; against the f64 restatement only"""
    kind, N, Ld, S, m = R.LARGE_CASE
    for which in ("D2", "random"):
        _, P, Q, prev, rout, rarg = R.layer_case(kind, N, Ld, S, m, which)
        out, arg = _layer(P, Q, prev, m)
        what = f"layer {(kind, N, Ld, S, m, which)}"
        assert _same(out, rout) and np.array_equal(arg, rarg), _report_difference(out, arg, rout, rarg, what)


# ---- table and trace ----------------------------------------------------------------------------------------------------------

def _table(X, K, m=1):
    N, Ld = X.shape
    P, Q = Guarded(torch.float64, N + 1, Ld), Guarded(torch.float64, N + 1)
    cost, arg, cuts = Guarded(torch.float64, K, N + 1), Guarded(torch.int32, K, N + 1), Guarded(torch.int32, K, K)
    ws = _ws(N, Ld)
    Xd = _dev(X)
    sfv._lib.call("rbvae_segment_prefix", Xd, N, Ld, P.t, Q.t)
    prev = _dev(R.first_prev(N))
    for k in range(K):
        sfv._lib.call("rbvae_segment_layer", P.t, Q.t, N, Ld, prev, m, cost.t[k], arg.t[k], ws.t)
        prev = cost.t[k]
    sfv._lib.call("rbvae_segment_trace", arg.t, N, K, cost.t, cuts.t)
    ws.check("workspace", full=False)
    P.check("P"), Q.check("Q")
    what = f"({N}, {Ld}, {K}, {m})"
    return cost.check("cost " + what), arg.check("arg " + what), cuts.check("cuts " + what)


def _check_table(X, K, m):
    """the device's table and trace equal the restatement's bit for bit, and segment_table returns them"""
    cost, arg, cuts = _table(X, K, m)
    rcost, rarg, _, _ = R.table(X, K, m)
    assert _same(cost, rcost) and np.array_equal(arg, rarg)
    assert np.array_equal(cuts, R.trace(rcost, rarg))
    t = sfv.segment_table(_dev(X), K, m)
    assert _same(t.cost.cpu().numpy(), cost) and np.array_equal(t.arg.cpu().numpy(), arg) and np.array_equal(t.cuts, cuts)
    assert _same(t.costs, cost[:, -1]) and t.min_size == m and t.cuts.dtype == np.int32
    if m == 1:                                              # one more segment never costs more, up to the table's rounding
        assert np.all(np.diff(cost[:, len(X)]) <= 2.0 * R.table_bound(X, K))
    return cost, arg, cuts


@pytest.mark.parametrize("N,Ld,K,m", R.BRUTE_CASES)
def test_table_against_brute_force(N, Ld, K, m):
    X = np.random.RandomState(N + Ld).rand(N, Ld).astype(np.float32)
    cost, arg, cuts = _check_table(X, K, m)
    costs, best = R.brute(X, K, m)
    for k in range(1, K + 1):
        assert abs(cost[k - 1, N] - costs[k - 1]) <= 1e-12
        assert tuple(cuts[k - 1, :k - 1]) == best[k - 1] and np.all(cuts[k - 1, k - 1:] == -1)


@pytest.mark.parametrize("kind,N,Ld,S,m", R.PLANTED_CASES)
def test_planted_boundaries(kind, N, Ld, S, m):
    X, planted = R.case(kind, N, Ld, S)
    if N <= 257:
        cuts = _check_table(X, S, m)[2]
    else:                                                   # the restatement of 17 layers of 1000 rows takes seconds
        cuts = _table(X, S, m)[2]
    assert np.array_equal(cuts[S - 1, :S - 1], planted)
    res = sfv.segment(_dev(X), n_segments=S, min_size=m)
    assert np.array_equal(res.boundaries, planted) and res.boundaries.dtype == np.int64 and res.n_segments == S
    assert np.array_equal(res.labels.cpu().numpy(), R.labels_of(planted, N)) and res.labels.dtype == torch.int32


def test_table_properties():
    # K m = N leaves exactly one segmentation
    X = R.case("soft", 12, 3, 3)[0]
    cost, arg, cuts = _check_table(X, 4, 3)
    assert np.array_equal(cuts[3], [3, 6, 9, -1])
    assert np.isfinite(cost[3, 12]) and np.isinf(cost[3, :12]).all() and np.isinf(cost[2, :9]).all()
    # D_1[N] against the long double total sum of squares
    for kind, N, Ld, S, m in R.LAYER_CASES[2:5]:
        X = R.case(kind, N, Ld, S)[0]
        d1 = _table(X, 1)[0][0]
        Xl = X.astype(R.LD)
        tss = float(((Xl - Xl.mean(axis=0)) ** 2).sum())
        b = R.layer_ld(X, R.first_prev(N), 1)["bound"][N]
        w = R.within(d1[N:], np.array([tss]), b + R.U * tss, f"D_1[N] ({N}, {Ld})")
        print(f"D_1[N] ({N}, {Ld}): |err|/bound {w:.3g} against the total sum of squares")
    # K = N on 8 rows: every row its own segment, cost 0 within the accumulated bounds
    X = R.case("soft", 8, 3, 2)[0]
    cost, arg, cuts = _check_table(X, 8, 1)
    assert np.array_equal(cuts[7, :7], np.arange(1, 8))
    Pl, Ql = R.prefix(X, R.LD)
    t = np.arange(1, 9)
    b = R.candidates(Pl, Ql, np.zeros(9), 1, t, R.p_bound(X), R.q_bound(X))[2]
    assert abs(cost[7, 8]) <= b[np.arange(8), np.arange(8)].sum() + R.TINY, cost[7, 8]
    # constant rows of 0.5: every finite cost is exactly 0 and every tie goes to the lowest start
    for m in (1, 3):
        X = np.full((70, 5), 0.5, dtype=np.float32)
        cost, arg, cuts = _check_table(X, 4, m)
        for k in range(4):
            fin = np.isfinite(cost[k])
            assert np.array_equal(np.nonzero(fin)[0], np.arange((k + 1) * m, 71)) and np.all(cost[k][fin] == 0.0)
            assert np.all(arg[k][fin] == k * m) and np.all(arg[k][~fin] == -1)
        assert np.array_equal(cuts[3, :3], [m, 2 * m, 3 * m])


def test_two_runs_of_a_table_are_bit_equal():
    kind, N, Ld, S, m = R.LAYER_CASES[4]
    X = R.case(kind, N, Ld, S)[0]
    a, b = _table(X, 6, m), _table(X, 6, m)
    assert all(_same(x, y) for x, y in zip(a, b))


# ---- segment ------------------------------------------------------------------------------------------------------------------

def test_segment_selection():
    kind, N, Ld, S, m = "soft", 130, 50, 5, 1
    X, planted = R.case(kind, N, Ld, S)
    Xd = _dev(X)
    tab = sfv.segment_table(Xd, 8)
    by_n = sfv.segment(Xd, n_segments=3, max_segments=8)
    assert by_n.n_segments == 3 and _same(by_n.costs, tab.costs) and by_n.cost == tab.costs[2]
    assert np.array_equal(by_n.boundaries, tab.cuts[2, :2])
    assert np.array_equal(by_n.labels.cpu().numpy(), R.labels_of(by_n.boundaries, N))
    one = sfv.segment(Xd, n_segments=1)
    assert one.boundaries.size == 0 and int(one.labels.abs().sum()) == 0 and len(one.costs) == 1
    # a penalty between the gain of the last true boundary and that of the first spurious one recovers S
    c = tab.costs
    gain = c[:-1] - c[1:]
    pen = 0.5 * (gain[S - 2] + gain[S - 1])
    assert gain[S - 2] > 10 * gain[S - 1]
    by_p = sfv.segment(Xd, max_segments=8, penalty=pen)
    assert by_p.n_segments == S and np.array_equal(by_p.boundaries, planted) and by_p.cost == c[S - 1]
    assert sfv.segment(Xd, max_segments=8, penalty=0.0).n_segments == 8
    assert sfv.segment(Xd, max_segments=8, penalty=10.0 * c[0]).n_segments == 1
    # a tie goes to the smaller k: constant rows cost 0 for every k, and with penalty 0 every k ties
    flat = sfv.segment(torch.full((40, 4), 0.25, device="cuda"), max_segments=5, penalty=0.0)
    assert flat.n_segments == 1 and np.all(flat.costs == 0.0)
    # a penalty that is exactly the gain of the second segment ties k = 1 and k = 2 on integer costs
    two = np.zeros((8, 1), dtype=np.float32)
    two[4:] = 2.0
    t2 = sfv.segment_table(_dev(two), 3)
    assert list(t2.costs) == [8.0, 0.0, 0.0] and list(t2.cuts[1]) == [4, -1, -1]
    assert sfv.segment(_dev(two), max_segments=3, penalty=8.0).n_segments == 1
    assert sfv.segment(_dev(two), max_segments=3, penalty=7.5).n_segments == 2
    for call, match in ((lambda: sfv.segment(Xd), "n_segments"), (lambda: sfv.segment(Xd, penalty=1.0), "max_segments"),
                        (lambda: sfv.segment(Xd, n_segments=9, max_segments=8), "between"),
                        (lambda: sfv.segment(Xd, n_segments=2, penalty=1.0), "not both"),
                        (lambda: sfv.segment(Xd, max_segments=3, penalty=-1.0), "penalty")):
        with pytest.raises(ValueError, match=match):
            call()


# ---- refused arguments --------------------------------------------------------------------------------------------------------------

def test_refused_arguments_write_nothing():
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")       # noqa: E731
    zd = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")      # noqa: E731
    zi = lambda *s: torch.zeros(s, dtype=torch.int32, device="cuda")        # noqa: E731
    P, Q = Guarded(torch.float64, 301, 129), Guarded(torch.float64, 301)
    out, arg, ws = Guarded(torch.float64, 301), Guarded(torch.int32, 301), Guarded(torch.float64, 4096)
    cuts = Guarded(torch.int32, 257, 257)
    X, Pin, Qin, prev = z(300, 129), zd(301, 129), zd(301), zd(301)
    err = sfv._lib.lib().rbvae_last_error
    for N, Ld, match in ((1, 3, "N=1,"), (300, 0, "L=0"), (300, 129, "L=129"), (65537, 3, "N=65537")):
        assert sfv._lib.query("rbvae_segment_ok", N, Ld, 1, 1) == 0 and sfv._lib.query("rbvae_segment_ws_bytes", N, Ld) == 0
        with pytest.raises(RuntimeError, match=match):
            sfv._lib.call("rbvae_segment_prefix", X, N, Ld, P.t, Q.t)
        assert match.encode() in err()
        with pytest.raises(RuntimeError, match=match):
            sfv._lib.call("rbvae_segment_layer", Pin, Qin, N, Ld, prev, 1, out.t, arg.t, ws.t)
    for m, match in ((0, "min_size=0"), (301, "min_size=301"), (-2, "min_size=-2")):
        with pytest.raises(RuntimeError, match=match):
            sfv._lib.call("rbvae_segment_layer", Pin, Qin, 300, 3, prev, m, out.t, arg.t, ws.t)
        assert match.encode() in err()
    for N, K, match in ((300, 257, "K=257"), (300, 0, "K=0"), (8, 9, "K=9"), (1, 1, "N=1,")):
        with pytest.raises(RuntimeError, match=match):
            sfv._lib.call("rbvae_segment_trace", zi(257, 301), N, K, zd(257, 301), cuts.t)
    with pytest.raises(ValueError, match="null"):
        sfv._lib.call("rbvae_segment_prefix", None, 300, 3, P.t, Q.t)
    with pytest.raises(ValueError, match="null"):
        sfv._lib.call("rbvae_segment_layer", Pin, Qin, 300, 3, None, 1, out.t, arg.t, ws.t)
    with pytest.raises(ValueError, match="null"):
        sfv._lib.call("rbvae_segment_trace", None, 300, 3, zd(3, 301), cuts.t)
    for g, what in ((P, "P"), (Q, "Q"), (out, "out"), (arg, "arg"), (ws, "workspace"), (cuts, "cuts")):
        g.check(what, untouched=True)
    bad = z(8, 3)
    bad[2, 1] = float("nan")
    for call, match in ((lambda: sfv.segment(bad, n_segments=2), "NaN"), (lambda: sfv.segment_prefix(bad), "NaN"),
                        (lambda: sfv.segment_table(z(8, 3), 9), "K=9"), (lambda: sfv.segment_table(z(8, 3), 3, 3), "min_size=3"),
                        (lambda: sfv.segment_table(z(8, 129), 2), "L=129"), (lambda: sfv.segment_table(z(8, 3).cpu(), 2), "GPU"),
                        (lambda: sfv.segment_prefix(z(8, 3).double()), "float32"), (lambda: sfv.segment_prefix(z(1, 3)), "N=1,"),
                        (lambda: sfv.segment_layer(zd(9, 3).cpu(), zd(9), zd(9)), "GPU"),
                        (lambda: sfv.segment_layer(zd(9, 3), zd(8), zd(9)), r"\[N \+ 1\]"),
                        (lambda: sfv.segment_layer(zd(9, 3), zd(9), zd(8)), "prev"),
                        (lambda: sfv.segment_layer(zd(9, 3), zd(9), zd(9), 9), "min_size=9"),
                        (lambda: sfv.segment_layer(z(9, 3), zd(9), zd(9)), "float64"),
                        (lambda: sfv.latent_segments(None, z(2, 3, 8, 8), [0], [1]), "frame indices")):
        with pytest.raises(ValueError, match=match):
            call()


# ---- latent_segments ----------------------------------------------------------------------------------------------------------

def test_latent_segments():
    F_, hw, LD = 24, (16, 24), 32
    torch.manual_seed(0)
    model = sfv.Seq2SeqBinaryVAE(4, 4, LD, LD, variant="percep", input_hw=hw, compute_dtype="f32").cuda().eval()
    g = torch.Generator().manual_seed(1)
    base = torch.randn(3, 4, *hw, generator=g)
    frames = list(range(100, 100 + 2 * F_, 2))              # frame numbers 100, 102, ...: positions are not frame numbers
    flags = [frames[7], frames[15] + 1]                     # states of 7, 9 and 8 frames: boundaries at positions 7 and 16
    state = np.array([sfv.assign_label(f, flags) for f in frames])
    x = (base[state] + 0.05 * torch.randn(F_, 4, *hw, generator=g)).cuda()
    u = torch.rand(F_, LD, generator=torch.Generator().manual_seed(2))
    out = sfv.latent_segments(model, x, frames, flags, u=u)
    assert not model.training and np.array_equal(out["labels"], state) and out["n_segments"] == 3
    assert np.array_equal(out["true_boundaries"], [7, 16]) and np.array_equal(out["true_frames"], [frames[7], frames[16]])
    z = model.encode(x[:, None], temperature=0.2, hard=False, noise_ratio=0.3, u=u.cuda())[:, 0].float().contiguous()
    codes = model.encode(x[:, None], temperature=0.2, hard=True, noise_ratio=0.3, u=u.cuda())[:, 0].float().contiguous()
    assert torch.equal(out["latents"], z) and torch.equal(out["codes"], codes)
    sym = sfv.latent_symbols(model, x, frames, flags, u=u)
    assert torch.equal(sym["latents"], z) and torch.equal(sym["codes"], codes)
    for name, rows in (("soft", z), ("hard", codes)):
        got, seg = out[name], sfv.segment(rows, n_segments=3)
        assert np.array_equal(got["boundaries"], seg.boundaries) and got["boundaries"].shape == (2,)
        assert torch.equal(got["segments"].labels, seg.labels) and got["segments"].cost == seg.cost
        assert _same(got["segments"].costs, seg.costs)
        assert np.array_equal(got["frames"], np.array(frames)[seg.boundaries])
        assert _same_scores(got["boundary_agreement"], sfv.boundary_agreement(seg.boundaries, [7, 16], 2))
        ref = sfv.clustering_agreement(state, seg.labels, 3, 3)
        assert all(got["label_agreement"][n] == ref[n] for n in ("ari", "nmi", "v_measure", "fowlkes_mallows"))
        assert np.array_equal(got["label_agreement"]["contingency"], ref["contingency"])
    again = sfv.latent_segments(model, x, frames, flags, u=u, n_segments=4, tolerance=0, min_size=2)
    assert again["soft"]["boundaries"].shape == (3,) and again["n_segments"] == 4
    assert np.diff(np.concatenate([[0], again["soft"]["boundaries"], [F_]])).min() >= 2
    assert again["soft"]["label_agreement"]["contingency"].shape == (3, 4)
    assert _same_scores(again["hard"]["boundary_agreement"], sfv.boundary_agreement(again["hard"]["boundaries"], [7, 16], 0))
