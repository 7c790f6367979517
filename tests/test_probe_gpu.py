"""GPU: the linear probe kernels (csrc/probe.hip) element by element against tests/_probe_ref.py's longdouble
references and written-down f64 bounds, inside NaN-sentinel guard bands, and linear_probe / frame_probe end to end against
the scikit-learn fixture tests/golden/linear_probe*.npz (tools/make_probe_golden.py).  Nothing here reads the reference
or scikit-learn.

End-to-end gate: r2 and evs within 1e-10 max(1, |ref|), mse and mae within 1e-10 ref of scikit-learn's float64 values.
Two correct f64 implementations agree to ~5e-16 on these cases and the reference's own f32 run sits >= 1e-9 (relative)
away, so the gate separates an f64 evaluation from an f32 one by an order of magnitude."""
import os

import numpy as np
import pytest
import torch

import _probe_ref as R
import sfv_amd as sfv

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SENT = 0x7FF8DEADDEADBEEF               # a NaN no f64 arithmetic produces
GUARD = 4096
U8, F32 = 0, 1


class G64:
    """n f64 elements inside GUARD sentinels on each side"""

    def __init__(self, *shape):
        self.n = int(np.prod(shape))
        self.buf = torch.full((GUARD + self.n + GUARD,), SENT, dtype=torch.int64, device="cuda")
        self.t = self.buf[GUARD:GUARD + self.n].view(torch.float64).view(*shape)

    def check(self, what):
        bits = self.buf.cpu().numpy()
        inner = np.zeros(bits.shape, dtype=bool)
        inner[GUARD:GUARD + self.n] = True
        stray = np.nonzero((bits != SENT) & ~inner)[0]
        assert stray.size == 0, f"{what}: {stray.size} elements outside the output were written; first at {stray[0] - GUARD}"
        unwritten = np.nonzero((bits == SENT) & inner)[0]
        assert unwritten.size == 0, f"{what}: {unwritten.size} output elements never written; first at {unwritten[0] - GUARD}"
        return self.t.cpu().numpy()


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def _xty(code, Yd, rows, row0, B, out):
    N, P = Yd.shape[0], Yd[0].numel()
    n, M = B.shape
    nbytes = sfv._lib.query("rbvae_probe_xty_ws_bytes", n, M, P)
    ws = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device="cuda") if nbytes else None
    sfv._lib.call("rbvae_probe_xty", code, Yd, N, P, _dev(rows, torch.int32), n, int(row0), _dev(B), M, out, ws)


def _case_data(Ld, P, N, n_train, n_test, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == "u8":
        Y = rng.integers(0, 256, (N, P), dtype=np.uint8)
        Y[:, P // 2] = 93                                   # one constant target
    else:
        Y = rng.standard_normal((N, P)).astype(np.float32)
    X = rng.standard_normal((N, Ld))
    perm = rng.permutation(N)                               # unsorted row lists
    train, test = perm[:n_train], perm[n_train:n_train + n_test]
    B, mean_x = R.factor(X[train])
    return X, Y, train, test, B, mean_x


# (L, P, N, train rows, test rows, targets): P off 16 and off the 256 / 64 tiles, row counts off 4, both load paths
# (16-byte pieces when P is a multiple of 16 (u8) / 4 (f32), element loads otherwise), one split-K configuration
SHAPES = [
    (1, 37, 20, 7, 5, "u8"),
    (25, 336, 70, 50, 13, "u8"),
    (32, 768, 128, 102, 26, "u8"),
    (100, 300, 160, 133, 27, "f32"),
    (128, 203, 180, 150, 30, "f32"),
    (32, 208, 700, 601, 99, "u8"),
]


@pytest.mark.parametrize("Ld,P,N,n_train,n_test,dtype", SHAPES)
def test_kernels_elementwise(Ld, P, N, n_train, n_test, dtype):
    X, Y, train, test, B, mean_x = _case_data(Ld, P, N, n_train, n_test, dtype, 100 + Ld + P)
    code, Yd, Yv = (U8 if dtype == "u8" else F32), _dev(Y), R.target_values(Y)
    M = Ld + 1
    slabs = sfv._lib.query("rbvae_probe_xty_slabs", n_train, M, P)
    assert (slabs > 1) == (n_train == 601), f"{slabs} slabs for {n_train} rows"

    # pass 1
    C = G64(M, P)
    _xty(code, Yd, train, train[0], B, C.t)
    Ch = C.check("C")
    ref, bnd = R.xty_ref(B, Yv, train, train[0])
    w = R.within(Ch, ref, bnd, f"C (L={Ld}, P={P}, {n_train} rows, {dtype}, {slabs} slabs)")
    print(f"C: worst |err|/bound {w:.3g}")
    if dtype == "u8":
        assert np.all(Ch[:, P // 2] == 0.0), "a constant target must give C == 0 exactly"
    C2 = G64(M, P)
    _xty(code, Yd, train, train[0], B, C2.t)
    assert np.array_equal(C2.check("C again").view(np.int64), Ch.view(np.int64)), "two runs differ"

    # intercept from the device's C
    ic = G64(P)
    sfv._lib.call("rbvae_probe_intercept", code, Yd, N, P, int(train[0]), C.t, _dev(mean_x), Ld, ic.t)
    ich = ic.check("intercept")
    ref, bnd = R.intercept_ref(Ch, mean_x, Yv[train[0]])
    print(f"intercept: worst |err|/bound {R.within(ich, ref, bnd, 'intercept'):.3g}")

    # pass 2 from the device's W and intercept
    sums = G64(5, P)
    args = (code, Yd, N, P, _dev(test, torch.int32), n_test, int(test[0]), _dev(X[test]), C.t, ic.t, Ld)
    sfv._lib.call("rbvae_probe_residual_sums", *args, sums.t)
    sh = sums.check("sums")
    ref, bnd = R.residual_ref(X[test], Ch[:Ld], ich, Yv, test, test[0])
    for j, nm in enumerate(("sum e", "sum e^2", "sum |e|", "sum d", "sum d^2")):
        print(f"{nm}: worst |err|/bound {R.within(sh[j], ref[j], bnd[j], nm):.3g}")
    if dtype == "u8":
        assert sh[3, P // 2] == 0.0 and sh[4, P // 2] == 0.0, "a constant target must give SStot == 0 exactly"
    sums2 = G64(5, P)
    sfv._lib.call("rbvae_probe_residual_sums", *args, sums2.t)
    assert np.array_equal(sums2.check("sums again").view(np.int64), sh.view(np.int64)), "two runs differ"

    # finish: guards, and the scores of the device's sums
    r2, evs, met = G64(P), G64(P), G64(4)
    part = torch.empty(sfv._lib.query("rbvae_probe_finish_parts", P) * 5, dtype=torch.float64, device="cuda")
    ncon = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    sfv._lib.call("rbvae_probe_finish", sums.t, P, n_test, r2.t, evs.t, part, met.t, ncon[1:2])
    r2h, evh, mh = r2.check("r2"), evs.check("evs"), met.check("metrics")
    assert ncon.tolist()[0] == -7 and ncon.tolist()[2] == -7
    rr, ee, sstot = R.scores(sh[0], sh[1], sh[3], sh[4], float(n_test))      # the same f64 expressions
    assert np.array_equal(r2h, rr) and np.array_equal(evh, ee)
    assert ncon.tolist()[1] == int((sstot == 0).sum()) == (1 if dtype == "u8" else 0)
    # means of P (r2, evs) or m P (mse, mae) terms, any order
    LDt = R.LD
    for got, terms, cnt in ((mh[0], rr, P), (mh[3], ee, P), (mh[1], sh[1] / n_test, P), (mh[2], sh[2] / n_test, P)):
        ref = float(terms.astype(LDt).sum() / cnt)
        assert abs(got - ref) <= 2 * (P + 2) * R.U * float(np.abs(terms).sum()) / cnt + R.TINY


def test_lane_map_exact():
    """M = 16, 4 rows, 16 targets of distinct integers: one MFMA per tile, every sum exact in f64, so any permutation of
    the operand or result lanes shows"""
    k, m, p = np.arange(4)[:, None], np.arange(16)[None, :], np.arange(16)[None, :]
    B = (1 + 16 * k + m).astype(np.float64)                 # 1..64
    Y = np.zeros((5, 16), dtype=np.float32)
    Y[:4] = 1000 + 37 * 16 * k + 41 * p                     # row 4 stays zero: the shift row
    C = G64(16, 16)
    _xty(F32, _dev(Y), np.arange(4), 4, B, C.t)
    assert np.array_equal(C.check("C"), B.T @ Y[:4].astype(np.float64))


@pytest.mark.parametrize("dtype", ["u8", "f32"])
def test_out_of_range_rows_contribute_nothing(dtype):
    Ld, P, N = 7, 80, 30
    X, Y, train, test, B, mean_x = _case_data(Ld, P, N, 18, 9, dtype, 9)
    code, Yd = (U8 if dtype == "u8" else F32), _dev(Y)
    C = G64(Ld + 1, P)
    _xty(code, Yd, train, train[0], B, C.t)
    # the same call with two more rows whose indices are outside [0, N): their factor rows must not matter
    rows2 = np.concatenate([train[:5], [N], train[5:], [-3]])
    B2 = np.concatenate([B[:5], np.full((1, Ld + 1), 1e6), B[5:], np.full((1, Ld + 1), -1e6)])
    C2 = G64(Ld + 1, P)
    _xty(code, Yd, rows2, train[0], B2, C2.t)
    ref, bnd = R.xty_ref(B, R.target_values(Y), train, train[0])
    R.within(C2.check("C with bad rows"), ref, bnd, "C with out-of-range rows")
    # inserted at a multiple of 4 the k-steps of the good rows keep their order: appended only, bit-identical
    rows3, B3 = np.concatenate([train, [N + 5, -1]]), np.concatenate([B, np.full((2, Ld + 1), 3e5)])
    C3 = G64(Ld + 1, P)
    _xty(code, Yd, rows3, train[0], B3, C3.t)
    assert np.array_equal(C3.check("C with appended bad rows").view(np.int64), C.check("C").view(np.int64))

    ic = torch.empty(P, dtype=torch.float64, device="cuda")
    sfv._lib.call("rbvae_probe_intercept", code, Yd, N, P, int(train[0]), C.t, _dev(mean_x), Ld, ic)
    s1, s2 = G64(5, P), G64(5, P)
    sfv._lib.call("rbvae_probe_residual_sums", code, Yd, N, P, _dev(test, torch.int32), len(test), int(test[0]),
                  _dev(X[test]), C.t, ic, Ld, s1.t)
    t2 = np.concatenate([test, [N, -1, 2 ** 31 - 1, N + 1]])        # appended: the good rows keep their wave and order
    x2 = np.concatenate([X[test], np.full((4, Ld), 1e9)])
    sfv._lib.call("rbvae_probe_residual_sums", code, Yd, N, P, _dev(t2, torch.int32), len(t2), int(test[0]), _dev(x2),
                  C.t, ic, Ld, s2.t)
    assert np.array_equal(s2.check("sums with bad rows").view(np.int64), s1.check("sums").view(np.int64))


def test_invalid_arguments():
    Y = torch.zeros((4, 8), dtype=torch.uint8, device="cuda")
    rows = torch.arange(3, dtype=torch.int32, device="cuda")
    d = torch.zeros(4096, dtype=torch.float64, device="cuda")
    call = sfv._lib.call
    for M in (1, 130):                                      # L < 1, L > 128
        with pytest.raises(ValueError, match="M="):
            call("rbvae_probe_xty", U8, Y, 4, 8, rows, 3, 0, d, M, d, None)
    with pytest.raises(ValueError, match="P="):
        call("rbvae_probe_xty", U8, Y, 4, 0, rows, 3, 0, d, 3, d, None)
    with pytest.raises(ValueError, match="empty row list"):
        call("rbvae_probe_xty", U8, Y, 4, 8, rows, 0, 0, d, 3, d, None)
    with pytest.raises(ValueError, match="null"):
        call("rbvae_probe_xty", U8, Y, 4, 8, None, 3, 0, d, 3, d, None)
    with pytest.raises(ValueError, match="shift row"):
        call("rbvae_probe_xty", U8, Y, 4, 8, rows, 3, 4, d, 3, d, None)
    with pytest.raises(ValueError, match="y_dtype"):
        call("rbvae_probe_xty", 2, Y, 4, 8, rows, 3, 0, d, 3, d, None)
    with pytest.raises(ValueError, match="L="):
        call("rbvae_probe_intercept", U8, Y, 4, 8, 0, d, d, 129, d)
    with pytest.raises(ValueError, match="L="):
        call("rbvae_probe_residual_sums", U8, Y, 4, 8, rows, 3, 0, d, d, d, 0, d)
    with pytest.raises(ValueError, match="empty row list"):
        call("rbvae_probe_residual_sums", U8, Y, 4, 8, rows, 0, 0, d, d, d, 2, d)
    with pytest.raises(ValueError, match="null"):
        call("rbvae_probe_finish", d, 8, 3, d, d, None, d, rows)
    with pytest.raises(ValueError, match="m="):
        call("rbvae_probe_finish", d, 8, 0, d, d, d, d, rows)


# ---- end to end against scikit-learn ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(os.path.join(GOLD, "linear_probe.npz")))
    g.update({k: v for k, v in np.load(os.path.join(GOLD, "linear_probe_coef.npz")).items() if "/" in k})
    return g


@pytest.mark.parametrize("name", R.CASES)
def test_linear_probe_against_sklearn(gold, name):
    X, Y = gold[f"{name}/X"], gold[f"{name}/Y"]
    kept = R.assert_rank_gap(X[gold[f"{name}/train"]], name)            # the cut does not depend on the host LAPACK
    assert kept == int(gold[f"{name}/rank"])
    res = sfv.linear_probe(torch.from_numpy(X), torch.from_numpy(Y).cuda())
    assert np.array_equal(res.train_idx, gold[f"{name}/train"]) and np.array_equal(res.test_idx, gold[f"{name}/test"])
    assert (res.n_train, res.n_test, res.n_constant_targets) == (len(res.train_idx), len(res.test_idx), 0)
    ref = gold[f"{name}/metrics_f64"]
    got = np.array([res.r2, res.mse, res.mae, res.evs])
    d = np.abs(got - ref)
    print(f"{name}: |device - sklearn f64| r2 {d[0]:.3g} mse {d[1]:.3g} (rel {d[1] / ref[1]:.3g}) mae {d[2]:.3g} "
          f"(rel {d[2] / ref[2]:.3g}) evs {d[3]:.3g}; sklearn f32 - f64 {gold[f'{name}/metrics_f32'] - ref}")
    assert d[0] <= 1e-10 * max(1.0, abs(ref[0])) and d[3] <= 1e-10 * max(1.0, abs(ref[3]))
    assert d[1] <= 1e-10 * ref[1] and d[2] <= 1e-10 * ref[2]
    # coef_ / intercept_ in the reference's CHW flatten order (bound: tests/test_probe_cpu.py)
    P, Ld = Y[0].size, X.shape[1]
    assert tuple(res.coef.shape) == (P, Ld) and tuple(res.intercept.shape) == (P,)
    lim = 8 * max(res.n_train, Ld) * 1e3 * R.U * (np.abs(gold[f"{name}/coef"]).max() + np.abs(gold[f"{name}/intercept"]).max())
    assert np.abs(res.coef.cpu().numpy() - gold[f"{name}/coef"]).max() <= lim
    assert np.abs(res.intercept.cpu().numpy() - gold[f"{name}/intercept"]).max() <= lim
    assert abs(float(res.r2_per_target.mean()) - res.r2) <= 1e-12 * max(1.0, abs(res.r2))
    # the same targets as f32 [N, P] rows in CHW order: the f32 entry, same values
    Yf = torch.from_numpy(R.chw((Y.astype(np.float32) / np.float32(255.0)).reshape(len(Y), -1), Y.shape[1:])).cuda()
    res32 = sfv.linear_probe(X, Yf.contiguous())
    got32 = np.array([res32.r2, res32.mse, res32.mae, res32.evs])
    assert np.all(np.abs(got32 - ref) <= 1e-10 * np.array([max(1.0, abs(ref[0])), ref[1], ref[2], max(1.0, abs(ref[3]))]))


def test_constant_columns_score_exactly_one(gold):
    name = R.CONST_CASE
    X, Y = gold[f"{name}/X"], gold[f"{name}/Y"]
    R.assert_rank_gap(X[gold[f"{name}/train"]], name)
    res = sfv.linear_probe(X, torch.from_numpy(Y).cuda())
    const = gold[f"{name}/constant_targets"]
    assert res.n_constant_targets == len(const) == 5
    r2, evs = res.r2_per_target.cpu().numpy(), res.evs_per_target.cpu().numpy()
    assert np.all(r2[const] == 1.0) and np.all(evs[const] == 1.0)
    assert np.all(res.coef.cpu().numpy()[const] == 0.0)
    assert np.array_equal(res.intercept.cpu().numpy()[const], R.chw(R.target_values(Y), Y.shape[1:])[0, const])
    rest, ref = np.delete(np.stack([r2, evs]), const, axis=1), gold[f"{name}/per_target_f64"]
    assert np.all(np.abs(rest - ref) <= 1e-10 * np.maximum(1.0, np.abs(ref)))


def test_explicit_split_and_bad_inputs():
    rng = np.random.default_rng(3)
    X = rng.standard_normal((30, 4))
    Y = torch.from_numpy(rng.integers(0, 256, (30, 6, 5, 3), dtype=np.uint8)).cuda()
    a = sfv.linear_probe(X, Y)
    b = sfv.linear_probe(X, Y, train_idx=a.train_idx, test_idx=a.test_idx)
    assert (a.r2, a.mse, a.mae, a.evs) == (b.r2, b.mse, b.mae, b.evs)
    with pytest.raises(ValueError, match="GPU"):
        sfv.linear_probe(X, Y.cpu())
    with pytest.raises(ValueError):
        sfv.linear_probe(X[:29], Y)
    with pytest.raises(ValueError):
        sfv.linear_probe(rng.standard_normal((30, 129)), Y)
    with pytest.raises(ValueError):
        sfv.linear_probe(X, Y, train_idx=[0, 1, 30], test_idx=[2])
    with pytest.raises(ValueError):
        sfv.linear_probe(X, Y.double())


# ---- frame_probe -----------------------------------------------------------------------------------------------------

F_, H_, W_, RES, LD, BATCH = 40, 50, 70, 64, 16, 16


@pytest.fixture(scope="module")
def frames_setup():
    torch.manual_seed(0)
    model = sfv.Seq2SeqBinaryVAE(3, 3, LD, LD, variant="contrastive", input_hw=(RES, RES), compute_dtype="f32").cuda().eval()
    rng = np.random.default_rng(4)
    yy, xx = np.mgrid[0:H_, 0:W_]
    a = np.empty((F_, H_, W_, 3), dtype=np.uint8)
    for f in range(F_):
        base = np.stack([(xx * 3 + 5 * f) % 256, (yy * 4 + 3 * f) % 256, np.where((xx // 10 + yy // 10 + f) % 2 == 0, 210, 30)], -1)
        a[f] = np.clip(base + rng.integers(-9, 10, base.shape), 0, 255)
    return model, torch.from_numpy(a).cuda()


@pytest.mark.parametrize("embedding", ["h", "z"])
def test_frame_probe_equals_its_parts(frames_setup, embedding):
    model, frames = frames_setup
    u = torch.rand(F_, LD, generator=torch.Generator().manual_seed(11))
    res = sfv.frame_probe(model, frames, resolution=RES, temperature=0.5, embedding=embedding, batch=BATCH, u=u)
    targets = sfv.resize_u8(frames, (RES, RES), "bilinear")
    emb = []
    with torch.no_grad():
        for s in range(0, F_, BATCH):
            x = sfv.u8_to_input(targets[s:s + BATCH], "totensor")[:, None]
            ub = u[s:s + BATCH].cuda()
            if embedding == "h":
                emb.append(model(x, temperature=0.5, u=ub)[1].reshape(-1, LD))
            else:
                emb.append(model.encode(x, temperature=0.5, hard=True, u=ub)[:, 0])
    ref = sfv.linear_probe(torch.cat(emb), targets)
    assert (res.r2, res.mse, res.mae, res.evs) == (ref.r2, ref.mse, ref.mae, ref.evs)
    assert res.n_constant_targets == ref.n_constant_targets and (res.n_train, res.n_test) == (32, 8)
    assert torch.equal(res.coef, ref.coef) and torch.equal(res.intercept, ref.intercept)
    assert torch.equal(res.r2_per_target, ref.r2_per_target)
    assert tuple(res.coef.shape) == (3 * RES * RES, LD) and np.isfinite([res.r2, res.mse, res.mae, res.evs]).all()
    assert not model.training


def test_frame_probe_rejects_cpu_frames(frames_setup):
    model, frames = frames_setup
    with pytest.raises(ValueError, match="GPU"):
        sfv.frame_probe(model, frames.cpu(), resolution=RES)
    with pytest.raises(ValueError, match="embedding"):
        sfv.frame_probe(model, frames, resolution=RES, embedding="q")
