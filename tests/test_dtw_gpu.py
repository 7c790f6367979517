"""GPU: dynamic time warping on the device (csrc/dtw.hip, alignment.py) against tests/_dtw_ref.py.  Every comparison is exact:
the contract fixes every rounding, the tie order and the end, so the table, the last row, the packed directions, the path, the
cost and the ends are compared bit for bit, inside sentinel guard bands, with and without the stored table, twice.  The shapes
stand on the library's tile edges (rbvae_dtw_tile_rows / _cols): one tile less and more by one, several tiles with ragged last
tiles, and tall and wide tables; test_dtw_cpu.py shows that each named defect of the restatement changes the result on these
same inputs.

Measured on one MI355X: every table, last row, byte of directions, path, cost and end equal to the restatement's bit for bit on
every case, the euclidean ones included (the device's sqrt agreed with np.sqrt in every cell), and two runs bit-equal.  The 144
tests take 3.6 s together; no case takes more than 0.4 s.
"""
import numpy as np
import pytest
import torch

import _dtw_ref as R
import sfv_amd as sfv

pytestmark = pytest.mark.gpu

q = sfv._lib.query
TI, TJ = q("rbvae_dtw_tile_rows"), q("rbvae_dtw_tile_cols")
TILE = (TI, TJ)
MET = {"sqeuclidean": 0, "euclidean": 1, "hamming": 2}
GUARD = 4096
SENT = {torch.float64: (torch.int64, 0x7FF8DEADDEADBEEF), torch.int32: (torch.int32, -0x21524111), torch.uint8: (torch.uint8, 0xA5)}


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


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()      # a copy: the shared inputs are read-only


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _same_scores(a, b):
    """two boundary_agreement dicts, NaN equal to NaN"""
    return a.keys() == b.keys() and all(a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]) for k in a)


def _raw(X, Y, metric, window=None, sub=False, table=True):
    """the three entries called directly on guarded buffers -> what they wrote"""
    (N, Ld), M = X.shape, Y.shape[0]
    w = -1 if window is None else window
    what = f"({N}, {M}, {Ld}, {metric}, {window}, {sub})"
    dirs = Guarded(torch.uint8, q("rbvae_dtw_dirs_bytes", N, M))
    last = Guarded(torch.float64, M)
    tab = Guarded(torch.float64, N, M) if table else None
    ws = Guarded(torch.float64, q("rbvae_dtw_ws_bytes", N, M) // 8)
    Xd, Yd = _dev(X), _dev(Y)
    if metric == "hamming":
        sfv._lib.call("rbvae_dtw_fill_bits", sfv.pack_codes(Xd), N, sfv.pack_codes(Yd), M, Ld, w, int(sub), dirs.t, last.t,
                      tab.t if table else None, ws.t)
    else:
        sfv._lib.call("rbvae_dtw_fill", Xd, N, Yd, M, Ld, MET[metric], w, int(sub), dirs.t, last.t, tab.t if table else None, ws.t)
    path, state, cost = Guarded(torch.int32, N + M - 1, 2), Guarded(torch.int32, 3), Guarded(torch.float64, 1)
    sfv._lib.call("rbvae_dtw_trace", dirs.t, last.t, N, M, int(sub), path.t, state.t, cost.t)
    ws.check("workspace " + what, full=False)
    n, start, end = state.check("state " + what).tolist()
    p = path.check("path " + what, full=False)
    assert 1 <= n <= N + M - 1, f"{what}: len = {n}"
    return {"D": tab.check("table " + what) if table else None, "last_row": last.check("last_row " + what),
            "packed": dirs.check("dirs " + what, full=False).reshape(N, (M + 3) // 4), "path": p[:n].astype(np.int64),
            "cost": float(cost.check("cost " + what)[0]), "start": start, "end": end}


def _explain(got, ref, what):
    if got["D"] is not None and not _same(got["D"], ref["D"]):
        bad = np.argwhere(_bits(got["D"]) != _bits(ref["D"]))
        i, j = bad[0]
        return (f"{what}: {len(bad)} cells of D differ; first ({i}, {j}): device {got['D'][i, j]!r}, restatement "
                f"{ref['D'][i, j]!r}")
    if not np.array_equal(got["packed"], ref["packed"]):
        bad = np.argwhere(got["packed"] != ref["packed"])
        return f"{what}: {len(bad)} bytes of dirs differ; first row {bad[0][0]}, byte {bad[0][1]}"
    return f"{what}: last_row, path, cost or ends differ"


def _agrees(got, ref, what):
    ok = (got["D"] is None or _same(got["D"], ref["D"])) and _same(got["last_row"], ref["last_row"])
    ok = ok and np.array_equal(got["packed"], ref["packed"]) and np.array_equal(got["path"], ref["path"])
    ok = ok and _same(np.array([got["cost"]]), np.array([ref["cost"]])) and (got["start"], got["end"]) == (ref["start"], ref["end"])
    assert ok, _explain(got, ref, what)


def _result_agrees(res, ref, N, M, table, what):
    assert isinstance(res, sfv.DTWResult) and res.path.dtype == np.int64 and res.path.shape == (res.path_len, 2)
    got = {"D": res.table.cpu().numpy() if table else None, "last_row": res.last_row.cpu().numpy(), "packed": ref["packed"],
           "path": res.path, "cost": res.cost, "start": res.start, "end": res.end}
    assert (res.table is None) == (not table) and res.last_row.is_cuda and res.last_row.shape == (M,)
    _agrees(got, ref, what)
    assert res.normalized_cost == res.cost / res.path_len


def _check(X, Y, metric, window=None, sub=False):
    """the entries and alignment.dtw against the restatement, with and without the stored table, twice"""
    N, M = len(X), len(Y)
    what = f"({N}, {M}, {X.shape[1]}, {metric}, {window}, {sub})"
    ref = R.dtw(X, Y, metric, window, sub, TILE)
    got = _raw(X, Y, metric, window, sub)
    _agrees(got, ref, what)
    _agrees(_raw(X, Y, metric, window, sub, table=False), ref, what + " without the table")
    again = _raw(X, Y, metric, window, sub)
    assert _same(again["D"], got["D"]) and np.array_equal(again["packed"], got["packed"]), what + ": two runs differ"
    Xd, Yd = _dev(X), _dev(Y)
    for table in (True, False):
        res = sfv.dtw(Xd, Yd, metric=metric, window=window, subsequence=sub, return_table=table)
        _result_agrees(res, ref, N, M, table, what)
    return got, ref


# ---- the whole table ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,L,N,M", R.global_cases(TI, TJ))
def test_table_dirs_and_path(kind, L, N, M):
    X, Y = R.make(kind, N, M, L)
    for metric in R.metrics_of(kind):
        got, ref = _check(X, Y, metric)
        assert (got["start"], got["end"]) == (0, M - 1) and got["cost"] == got["D"][N - 1, M - 1]
        dirs = R.unpack_dirs(got["packed"], M)
        assert dirs[0, 0] == 3 and (dirs == 3).sum() == 1


def test_fill_and_trace_are_the_two_halves():
    X, Y = R.make("repeat", 2 * TI + 5, 3 * TJ + 3, 50)
    Xd, Yd = _dev(X), _dev(Y)
    t = sfv.dtw_fill(Xd, Yd, metric="euclidean", return_table=True)
    ref = R.dtw(X, Y, "euclidean", tile=TILE)
    assert isinstance(t, sfv.DTWTable) and (t.N, t.M, t.subsequence) == (len(X), len(Y), False)
    assert t.dirs.dtype == torch.uint8 and np.array_equal(t.dirs.cpu().numpy(), ref["packed"])
    assert _same(t.table.cpu().numpy(), ref["D"]) and _same(t.last_row.cpu().numpy(), ref["last_row"])
    _result_agrees(sfv.dtw_trace(t), ref, len(X), len(Y), True, "dtw_trace")
    assert sfv.dtw_fill(Xd, Yd).table is None


# ---- the band -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,L,metric,N,M,w", R.band_cases(TI, TJ))
def test_band(kind, L, metric, N, M, w):
    X, Y = R.make(kind, N, M, L)
    if w < abs(N - M):                                      # no path inside the band: refused
        with pytest.raises(ValueError, match=f"window={w}"):
            sfv.dtw(_dev(X), _dev(Y), metric=metric, window=w)
        return
    got, ref = _check(X, Y, metric, window=w)
    i, j = np.indices((N, M))
    out = np.abs(i - j) > w
    dirs = R.unpack_dirs(got["packed"], M)
    assert np.all(np.isposinf(got["D"][out])) and np.all(dirs[out] == 3)
    assert np.all(np.isfinite(got["D"][~out])) and (dirs[~out] == 3).sum() == 1
    assert np.all(np.abs(got["path"][:, 0] - got["path"][:, 1]) <= w)


def test_band_cases_leave_whole_tiles_outside():
    """the premise of test_band: on the shapes with tiles off the diagonal the narrowest band skips whole tiles, whose
    neighbours must still read +inf on the shared edges, and the widest listed band still skips one"""
    for N, M in R.multi_tile_shapes(TI, TJ)[:2]:
        ws = [w for w in R.band_windows(N, M, TI, TJ) if w >= abs(N - M)]
        assert R.tiles_outside(N, M, ws[0], TI, TJ) >= 1 and R.tiles_outside(N, M, ws[-1], TI, TJ) >= 1
    assert R.tiles_outside(2 * TI + 5, 3 * TJ + 3, abs(2 * TI + 5 - 3 * TJ - 3), TI, TJ) >= 3


@pytest.mark.parametrize("N,M", R.multi_tile_shapes(TI, TJ))
def test_a_band_as_wide_as_the_table_is_none(N, M):
    X, Y = R.make("repeat", N, M, 50)
    free = _raw(X, Y, "sqeuclidean")
    for w in (max(N, M), max(N, M) + 7, 1 << 30):
        _agrees(_raw(X, Y, "sqeuclidean", window=w), free, f"window {w}")
    res = sfv.dtw(_dev(X), _dev(Y), window=10 ** 12)
    assert np.array_equal(res.path, free["path"]) and res.cost == free["cost"]


# ---- subsequence --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,metric,X,Y", R.subsequence_cases(TI, TJ), ids=[c[0] for c in R.subsequence_cases(TI, TJ)])
def test_subsequence(name, metric, X, Y):
    got, ref = _check(X, Y, metric, sub=True)
    N, M = len(X), len(Y)
    dirs = R.unpack_dirs(got["packed"], M)
    assert np.all(dirs[0] == 3) and (N == 1 or np.all(dirs[1:] != 3))
    assert _same(got["D"][0], R.cost_matrix(X, Y, metric)[0])                   # row 0 does not accumulate
    assert got["path"][0, 0] == 0 and got["path"][0, 1] == got["start"] and got["path"][-1].tolist() == [N - 1, got["end"]]


def test_subsequence_finds_the_clip():
    for kind, L, metric in (("code", 50, "hamming"), ("soft", 50, "sqeuclidean"), ("soft", 128, "euclidean")):
        X, Y, pos = R.subsequence_case(kind, L, TI, TJ, 0)
        res = sfv.dtw(_dev(X), _dev(Y), metric=metric, subsequence=True)
        assert res.cost == 0.0 and (res.start, res.end) == (pos, pos + len(X) - 1) and res.path_len == len(X)
        assert np.array_equal(res.path, np.stack([np.arange(len(X)), pos + np.arange(len(X))], 1))
        labels = sfv.transfer_labels(res.path, np.arange(len(X)) // 8, len(Y))
        assert np.all(labels[:pos] == -1) and np.all(labels[pos + len(X):] == -1)
        assert np.array_equal(labels[pos:pos + len(X)], np.arange(len(X)) // 8)
    X, Y, (a, b) = R.twice_case(50, TI, TJ)                                     # two ends cost 0: the lower j
    res = sfv.dtw(_dev(X), _dev(Y), metric="hamming", subsequence=True)
    last = res.last_row.cpu().numpy()
    assert last[a + len(X) - 1] == 0.0 and last[b + len(X) - 1] == 0.0 and a < b
    assert res.cost == 0.0 and (res.start, res.end) == (a, a + len(X) - 1)


# ---- refused without a launch -------------------------------------------------------------------------------------------------------------

def test_refused_arguments_write_nothing():
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")           # noqa: E731
    zi = lambda *s: torch.zeros(s, dtype=torch.int32, device="cuda")            # noqa: E731
    dirs, last, tab = Guarded(torch.uint8, 300 * 75), Guarded(torch.float64, 300), Guarded(torch.float64, 300, 300)
    ws, path = Guarded(torch.float64, 1024), Guarded(torch.int32, 599, 2)
    state, cost = Guarded(torch.int32, 3), Guarded(torch.float64, 1)
    X, Y, B = z(300, 129), z(300, 129), zi(300, 4)
    err = sfv._lib.lib().rbvae_last_error
    # (N, M, L, metric, window, subsequence) and what the message names
    for N, M, Ld, met, w, sub, match in ((0, 5, 3, 0, -1, 0, "N=0,"), (5, 0, 3, 0, -1, 0, "M=0,"), (16385, 5, 3, 0, -1, 0, "N=16385"),
                                         (5, 16385, 3, 0, -1, 0, "M=16385"), (300, 300, 0, 0, -1, 0, "L=0"),
                                         (300, 300, 129, 0, -1, 0, "L=129"), (300, 300, 3, 3, -1, 0, "metric=3"),
                                         (300, 290, 3, 0, 9, 0, "window=9"), (290, 300, 3, 1, 9, 0, "window=9"),
                                         (30, 300, 3, 0, 280, 1, "subsequence=1"), (300, 300, 3, 0, -2, 0, "window=-2")):
        assert q("rbvae_dtw_ok", N, M, Ld, met, w, sub) == 0
        with pytest.raises(RuntimeError, match=match):
            sfv._lib.call("rbvae_dtw_fill", X, N, Y, M, Ld, met, w, sub, dirs.t, last.t, tab.t, ws.t)
        assert match.encode() in err()
        if met != 3:
            with pytest.raises(RuntimeError, match=match):
                sfv._lib.call("rbvae_dtw_fill_bits", B, N, B, M, Ld, w, sub, dirs.t, last.t, tab.t, ws.t)
    with pytest.raises(RuntimeError, match="fill_bits"):                        # packed codes have their own entry
        sfv._lib.call("rbvae_dtw_fill", X, 300, Y, 300, 3, 2, -1, 0, dirs.t, last.t, tab.t, ws.t)
    for N, M, match in ((0, 5, "N=0,"), (5, 16385, "M=16385")):
        with pytest.raises(RuntimeError, match=match):
            sfv._lib.call("rbvae_dtw_trace", dirs.t, last.t, N, M, 0, path.t, state.t, cost.t)
    with pytest.raises(RuntimeError, match="subsequence=2"):
        sfv._lib.call("rbvae_dtw_trace", dirs.t, last.t, 300, 300, 2, path.t, state.t, cost.t)
    for args in ((None, 300, Y), (X, 300, None)):
        with pytest.raises(ValueError, match="null"):
            sfv._lib.call("rbvae_dtw_fill", args[0], args[1], args[2], 300, 3, 0, -1, 0, dirs.t, last.t, tab.t, ws.t)
    for bad in range(4):
        a = [dirs.t, last.t, tab.t, ws.t]
        if bad == 2:
            continue                                        # table may be NULL
        a[bad] = None
        with pytest.raises(ValueError, match="null"):
            sfv._lib.call("rbvae_dtw_fill_bits", B, 300, B, 300, 3, -1, 0, *a)
    with pytest.raises(ValueError, match="null"):
        sfv._lib.call("rbvae_dtw_trace", dirs.t, None, 300, 300, 0, path.t, state.t, cost.t)
    with pytest.raises(ValueError, match="null"):
        sfv._lib.call("rbvae_dtw_trace", dirs.t, last.t, 300, 300, 0, path.t, state.t, None)
    for g, what in ((dirs, "dirs"), (last, "last_row"), (tab, "table"), (ws, "workspace"), (path, "path"), (state, "state"),
                    (cost, "cost")):
        g.check(what, untouched=True)
    bad = z(8, 3)
    bad[2, 1] = float("nan")
    inf = z(8, 3)
    inf[0, 0] = float("inf")
    for call, match in ((lambda: sfv.dtw(z(8, 3).cpu(), z(9, 3)), "GPU"), (lambda: sfv.dtw(z(8, 3), z(9, 3).cpu()), "GPU"),
                        (lambda: sfv.dtw(bad, z(9, 3)), "NaN"), (lambda: sfv.dtw(z(9, 3), bad, metric="hamming"), "NaN"),
                        (lambda: sfv.dtw(z(9, 3), inf), "infinite"), (lambda: sfv.dtw(z(8, 3).double(), z(9, 3)), "float32"),
                        (lambda: sfv.dtw(z(8, 3), z(9, 3).int()), "float32"), (lambda: sfv.dtw(z(8, 6)[:, ::2], z(9, 3)), "contiguous"),
                        (lambda: sfv.dtw(z(8, 3), z(3, 9).t()), "contiguous"), (lambda: sfv.dtw(z(8, 3), z(9, 4)), "L=3.*L=4"),
                        (lambda: sfv.dtw(z(8, 3), z(12, 3), window=3), "window=3"), (lambda: sfv.dtw(z(8, 3), z(9, 3), window=-1), "window"),
                        (lambda: sfv.dtw(z(8, 3), z(12, 3), window=5, subsequence=True), "subsequence=True"),
                        (lambda: sfv.dtw(z(8, 129), z(9, 129)), "L=129"), (lambda: sfv.dtw(z(8, 3), z(9, 3), metric="cosine"), "metric"),
                        (lambda: sfv.dtw(z(8), z(9, 3)), "2-D"), (lambda: sfv.dtw_fill(np.zeros((8, 3), np.float32), z(9, 3)), "torch tensor"),
                        (lambda: sfv.latent_alignment(None, z(2, 3, 8, 8), z(2, 3, 8, 8), [0], [1], [0, 1], [1]), "frame indices")):
        with pytest.raises(ValueError, match=match):
            call()


# ---- latent_alignment -----------------------------------------------------------------------------------------------------------------------

def test_latent_alignment():
    Fa, hw, LD = 24, (16, 24), 32
    torch.manual_seed(0)
    model = sfv.Seq2SeqBinaryVAE(4, 4, LD, LD, variant="percep", input_hw=hw, compute_dtype="f32").cuda().eval()
    g = torch.Generator().manual_seed(1)
    base = torch.randn(3, 4, *hw, generator=g)
    frames_a = list(range(100, 100 + 2 * Fa, 2))
    flags_a = [frames_a[7], frames_a[15] + 1]               # states of 7, 9 and 8 frames
    state_a = np.array([sfv.assign_label(f, flags_a) for f in frames_a])
    x_a = (base[state_a] + 0.05 * torch.randn(Fa, 4, *hw, generator=g)).cuda()
    # B: A's frames resampled at a varying speed -- slow, then fast, then slow
    pick = np.array([0, 0, 1, 1, 2, 3, 3, 4, 5, 6, 8, 10, 12, 14, 16, 17, 17, 18, 19, 19, 20, 21, 22, 22, 23, 23, 23])
    Fb = len(pick)
    x_b = x_a[torch.from_numpy(pick).cuda()].contiguous()
    frames_b = list(range(500, 500 + Fb))
    state_b = state_a[pick]
    flags_b = [frames_b[int(np.nonzero(state_b == 1)[0][0])], frames_b[int(np.nonzero(state_b == 2)[0][0])]]
    assert np.array_equal([sfv.assign_label(f, flags_b) for f in frames_b], state_b)
    u_a = torch.rand(Fa, LD, generator=torch.Generator().manual_seed(2))
    u_b = torch.rand(Fb, LD, generator=torch.Generator().manual_seed(3))
    out = sfv.latent_alignment(model, x_a, x_b, frames_a, flags_a, frames_b, flags_b, u_a=u_a, u_b=u_b)
    assert not model.training and np.array_equal(out["labels_a"], state_a) and np.array_equal(out["labels_b"], state_b)
    enc = lambda x, u, hard: model.encode(x[:, None], temperature=0.2, hard=hard, noise_ratio=0.3,  # noqa: E731
                                          u=u.cuda())[:, 0].float().contiguous()
    za, zb, ca, cb = enc(x_a, u_a, False), enc(x_b, u_b, False), enc(x_a, u_a, True), enc(x_b, u_b, True)
    assert torch.equal(out["latents_a"], za) and torch.equal(out["latents_b"], zb)
    assert torch.equal(out["codes_a"], ca) and torch.equal(out["codes_b"], cb)
    true_b = np.nonzero(state_b[1:] != state_b[:-1])[0] + 1
    assert np.array_equal(out["true_boundaries_b"], true_b)
    for name, a, b, metric in (("soft", za, zb, "sqeuclidean"), ("hard", ca, cb, "hamming")):
        got = out[name]
        ref = R.dtw(a.cpu().numpy(), b.cpu().numpy(), metric, tile=TILE)
        assert np.array_equal(got["dtw"].path, ref["path"]) and got["dtw"].cost == ref["cost"]
        assert (got["dtw"].start, got["dtw"].end) == (0, Fb - 1) and got["dtw"].table is None
        labels = sfv.transfer_labels(ref["path"], state_a, Fb)
        assert got["labels"].shape == (Fb,) and got["labels"].dtype == np.int64 and np.array_equal(got["labels"], labels)
        assert got["accuracy"] == float((labels == state_b).mean())
        wm = sfv.warp_map(ref["path"], Fa, Fb)
        assert all(np.array_equal(got["warp"][k], wm[k]) for k in wm) and got["warp"]["first_i"].shape == (Fb,)
        bounds = np.nonzero(labels[1:] != labels[:-1])[0] + 1
        assert np.array_equal(got["boundaries"], bounds)
        assert _same_scores(got["boundary_agreement"], sfv.boundary_agreement(bounds, true_b, 2))
        agree = sfv.clustering_agreement(state_b, torch.from_numpy(labels).cuda(), 3, 3)
        assert got["label_agreement"]["ari"] == agree["ari"]
        assert np.array_equal(got["label_agreement"]["contingency"], agree["contingency"])
    # given latents are used as they are; a band is passed on; without uniforms the two calls draw their own
    again = sfv.latent_alignment(model, x_a, x_b, frames_a, flags_a, frames_b, flags_b, latents_a=za, latents_b=zb, window=6,
                                 u_a=u_a, u_b=u_b)
    assert torch.equal(again["latents_a"], za) and torch.equal(again["codes_b"], cb)
    ref = R.dtw(za.cpu().numpy(), zb.cpu().numpy(), "sqeuclidean", window=6, tile=TILE)
    assert np.array_equal(again["soft"]["dtw"].path, ref["path"])
    torch.manual_seed(5)
    drawn = sfv.latent_alignment(model, x_a, x_a, frames_a, flags_a, frames_a, flags_a)
    assert not torch.equal(drawn["latents_a"], drawn["latents_b"])              # the same frames under independent uniforms
