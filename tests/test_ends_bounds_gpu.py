"""Element-wise bounds and guarded stores for the kernels at the 3/4-channel ends of the two CNNs (tests/_ends_cases.py
holds the cases, the restated dispatch, the float64 references and the error model; tests/_bounds.py the buffers):

  rbvae_conv_first_fused          conv_first_fused_k<CIN, 0, NQ>: every element against conv2d of the bf16-rounded frames
                                  (ReLU, bias, keyed dropout decided by the reference), col rows bit for bit, col = NULL
  rbvae_deconv_last_dgrad_fused   conv_first_fused_k<CIN, 1, NQ>: the gate over every bf16 pattern class, colsum_ws per block
  rbvae_wgrad_first               wgrad_first_k / wgrad_first_wide_k<CIN, MODE>: every K-slice slab against its own pixels
  rbvae_deconv_last_fused         deconv_last_fused_k<ONE>: x_recon through the sigmoid bound (incl. saturated cases), dpre,
                                  the squared-error and dpre column sums of every workgroup
  rbvae_conv_in                   conv_in_k<CIN, NQ>: output, tile statistics, rbvae_gn_finish_tiles(.., 8, 16)
  rbvae_im2col(_frames), rbvae_col2im_sigmoid(_frames), rbvae_sigmoid_bwd_nhwc: the two-kernel path

Every output, workspace and slab sits inside NaN guard bands (assert_guards: no stray store, every declared element
written); every input inside NaN guard rows, NaN padding columns (ldo > Nout, ldy > Nout) and NaN between the frames of a
frame-mapped buffer.  Refusals go through the argument checks that return before a launch and leave the outputs untouched.

Worst |err| / bound per kernel, the maxima over the cases of the printed BOUNDS lines from the first device run (MI355X):

  conv_first_fused          out 0.996
  deconv_last_dgrad_fused   out 0.996   colsum 0.00271
  wgrad_first               wgrad_first_k 0.222   wgrad_first_wide_k 0.272
  deconv_last_fused         xr 0.467   dpre 0.725   dsum 0.121   sse 0.0889
  conv_in                   out 0.996   stats 0.0156   gn_finish 0.00487
  col2im_sigmoid            xr 0.633   dpre 0.771   dsum 0.134   sse 0.15   sse_mean 0.0522
  sigmoid_bwd_nhwc          0.615

(the col rows are compared bit for bit and print no ratio).  What is established without a device
(test_ends_bounds_cpu.py): the gates agree with the library, an f32 emulation of every operation passes every bound, and
every named defect is rejected -- the two-kernel arithmetic (Y rounded to bf16) lands about 2000 times outside the
deconv_last_fused bound.

rbvae_wgrad_first at the cfg-3 size (128 x 3 x 256 x 256, ksplit 512) stays with
test_kernels_gpu.py::test_wgrad_first_at_the_cfg3_frame_size: its float64 reference (2 097 152 pixel rows) alone costs more
than this whole file."""
import pytest
import torch

import _bounds as B
import _ends_cases as E

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
ids = lambda cases: [c["id"] for c in cases]


@pytest.fixture(scope="module")
def lib():
    import sfv_amd
    return sfv_amd._lib


def zero_page():
    return torch.zeros(256, dtype=torch.uint8, device="cuda")


def report(kind, c, dtype, res):
    if isinstance(res, dict):
        res = " ".join(f"{k} {v:.3g}" for k, v in res.items())
    else:
        res = f"{res:.3g}"
    print(f"\nBOUNDS {kind} {c} {dtype} worst |err|/bound = {res}")


def f32_row(t):
    """A [1][n] f32 vector (bias, gscale_dev) inside NaN guard rows, its row padded with NaN to 16 bytes."""
    t = t.reshape(1, -1).float()
    return B.poisoned(t, E.cdiv(t.shape[1], 4) * 4, F32)


def flat_in(t):
    """An f32 input of any length inside NaN guards (NaN values inside t, the gaps between mapped frames, stay)."""
    g = B.GuardedFlat(t.numel(), F32)
    g.view.copy_(t.reshape(-1).float())
    return g


def frames_in(x, fmap):
    buf, fm = E.frame_buffer(x, fmap)
    return flat_in(buf), fm


def bits16(t):
    return t.contiguous().view(torch.int16).cpu()


def untouched(*gs):
    for g in gs:
        ib, pat = B.SENTINEL[g.dtype]
        assert bool((g.buf.view(ib) == pat).all()), "a refused call wrote to its output"


# ---- conv_first_fused_k ------------------------------------------------------------------------------------------------

CF0 = [c for c in E.CF_CASES if c["mode"] == 0]
CF1 = [c for c in E.CF_CASES if c["mode"] == 1]


@pytest.mark.parametrize("c", CF0, ids=ids(CF0))
def test_conv_first_fused_bounded_and_guarded(lib, c):
    N, Cin, IH, IW, Nout, ldo = c["N"], c["Cin"], c["IH"], c["IW"], c["Nout"], c["ldo"]
    assert lib.query("rbvae_conv_first_fused_ok", 1, Cin, IH, IW, Nout, N) == E.cf_shape_ok("bf16", Cin, IH, IW, Nout, N) == 1
    inst = E.cf_instance(Cin, 0, Nout)
    d = E.cf_build(c)
    x, fm = frames_in(d["x"], c["fmap"])
    W = B.poisoned(d["Wp"], 64, BF)
    bias = f32_row(d["bias"]) if d["bias"] is not None else None
    sd = torch.tensor([c["seed_dev"]], dtype=torch.int64, device="cuda") if c["seed_dev"] is not None else None
    outs = []
    for with_col in (True, False):
        out = B.guarded(d["P"], ldo, Nout, BF)
        col = B.guarded(d["P"], 64, 64, BF) if with_col else None
        lib.call("rbvae_conv_first_fused", 1, x.view, *fm, W.view, bias and bias.view, zero_page(), col and col.view, out.view,
                 N, Cin, IH, IW, Nout, ldo, c["relu"], 1 if c["drop"] else 0, c["p"], c["scale"], c["seed"], sd)
        torch.cuda.synchronize()
        what = f"{c['id']} {inst} col={'yes' if with_col else 'NULL'}"
        B.assert_guards(out, f"{what} out")
        if col is not None:
            B.assert_guards(col, f"{what} col")
        outs.append((out, col))
    res = E.cf_check(c, d, dict(out=outs[0][0].out, col=bits16(outs[0][1].out)), what=c["id"])
    assert torch.equal(bits16(outs[0][0].out), bits16(outs[1][0].out)), f"{c['id']}: col = NULL changes the output"
    if c["drop"]:
        got_zero = (outs[0][0].out.float().cpu() == 0)
        assert bool(got_zero[~d["keep"]].all()), f"{c['id']}: a dropped element is not zero"
    report("conv_first_fused", f"<{Cin},0,{inst[3]}> {c['id']}", "bf16", res)


@pytest.mark.parametrize("c", CF1, ids=ids(CF1))
def test_deconv_last_dgrad_fused_bounded_and_guarded(lib, c):
    N, Cout, OH, OW, C1, ldo = c["N"], c["Cin"], c["IH"], c["IW"], c["Nout"], c["ldo"]
    nblk = lib.query("rbvae_deconv_last_dgrad_blocks", 1, Cout, OH, OW, C1, N)
    assert nblk == E.dgrad_blocks("bf16", Cout, OH, OW, C1, N) > 0
    inst = E.cf_instance(Cout, 1, C1)
    d = E.cf_build(c)
    dpre = flat_in(d["x_store"])
    W = B.poisoned(d["Wp"], 64, BF)
    gate = B.poisoned(d["gate"], ldo, BF)
    assert torch.equal(bits16(gate.out), d["gate"].view(torch.int16)), "gate patterns must reach the device bit for bit"
    outs = []
    for full in (True, False):
        out = B.guarded(d["P"], ldo, C1, BF)
        col = B.guarded(d["P"], 64, 64, BF) if full else None
        ws = B.guarded(nblk, C1, C1, F32) if full else None
        lib.call("rbvae_deconv_last_dgrad_fused", 1, dpre.view, W.view, zero_page(), col and col.view, gate.view, out.view, N,
                 Cout, OH, OW, C1, ldo, c["scale"], ws and ws.view)
        torch.cuda.synchronize()
        what = f"{c['id']} {inst} {'col + colsum' if full else 'col = colsum = NULL'}"
        B.assert_guards(out, f"{what} out")
        if full:
            B.assert_guards(col, f"{what} col")
            B.assert_guards(ws, f"{what} colsum_ws")
        outs.append((out, col, ws))
    res = E.cf_check(c, d, dict(out=outs[0][0].out, col=bits16(outs[0][1].out), colsum=outs[0][2].out), what=c["id"])
    assert torch.equal(bits16(outs[0][0].out), bits16(outs[1][0].out)), f"{c['id']}: colsum_ws = NULL changes the output"
    report("deconv_last_dgrad_fused", f"<{Cout},1,{inst[3]}> {c['id']}", "bf16", res)


# ---- rbvae_wgrad_first -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", E.WF_CASES, ids=ids(E.WF_CASES))
def test_wgrad_first_slabs_bounded_and_guarded(lib, c):
    N, Cin, IH, IW, Nout, ks, mode = c["N"], c["Cin"], c["IH"], c["IW"], c["Nout"], c["ks"], c["mode"]
    nblk = lib.query("rbvae_wgrad_first_blocks", 1, Cin, IH, IW, Nout, N)
    assert nblk == E.wgrad_first_blocks("bf16", Cin, IH, IW, Nout, N) and 1 <= ks <= nblk
    d = E.wf_build(c)
    if mode == 0:
        x, fm = frames_in(d["x"], c["fmap"])
    else:
        x, fm = flat_in(d["x_store"]), (0, 0, 0, 0, 0)
    dy = B.poisoned(d["dy"], c["ldy"], BF)
    slabs = B.guarded(ks * Nout, 64, 64, F32, guard_rows=Nout)                   # a whole guard slab on each side
    lib.call("rbvae_wgrad_first", 1, mode, x.view, *fm, dy.view, slabs.view, zero_page(), N, Cin, IH, IW, Nout, c["ldy"], ks)
    torch.cuda.synchronize()
    inst = E.wf_instance(Cin, mode, Nout)
    B.assert_guards(slabs, f"{c['id']} {inst} slabs")
    worst = E.wf_check(c, d, slabs.out, what=f"{c['id']} {inst}")
    report("wgrad_first", f"{inst[0]}<{Cin},{mode}> {c['id']}", "bf16", worst)


# ---- rbvae_deconv_last_fused -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", E.DL_CASES, ids=ids(E.DL_CASES))
def test_deconv_last_fused_bounded_and_guarded(lib, c):
    N, IH, IW, C1, Cout, NYP = c["N"], c["IH"], c["IW"], c["C1"], c["Cout"], c["NYP"]
    OH, OW = 2 * IH, 2 * IW
    parts = lib.query("rbvae_deconv_last_fused_parts", 1, N, IH, IW, C1, Cout)
    d = E.dl_build(c)
    assert parts == E.dl_parts("bf16", N, IH, IW, C1, Cout) == d["parts"]
    D2 = B.poisoned(B.rows(d["a"]), C1, BF)
    V = B.poisoned(d["Vp"], C1, BF)
    bias = f32_row(d["bias"]) if d["bias"] is not None else None
    xr = B.GuardedFlat(N * Cout * OH * OW, F32)
    tgt, fm, ws, dpre = None, (0, 0, 0, 0, Cout * OH * OW), None, None
    if d["target"] is not None:
        tgt, fm = frames_in(d["target"], None if c["target"] == "plain" else c["target"])
        ws = B.GuardedFlat(5 * parts if c["dpre"] else parts, F32)      # dpre = NULL: the 4 parts tail stays sentinel (guard)
        dpre = B.GuardedFlat(N * OH * OW * Cout, F32) if c["dpre"] else None
    lib.call("rbvae_deconv_last_fused", 1, D2.view, V.view, NYP, bias and bias.view, zero_page(), N, IH, IW, C1, Cout, xr.view,
             tgt and tgt.view, *fm, ws and ws.view, dpre and dpre.view, c["gscale"])
    torch.cuda.synchronize()
    what = f"{c['id']} deconv_last_fused_k<{E.dl_instance(C1)[1]}>"
    got = dict(xr=xr.out.reshape(N, Cout, OH, OW))
    for g, nm in ((xr, "xr"), (ws, "ws"), (dpre, "dpre")):
        if g is not None:
            B.assert_guards(g, f"{what} {nm}")
    if ws is not None:
        got["sse"] = ws.out[:parts]
    if dpre is not None:
        got["dpre"] = dpre.out.reshape(N, OH, OW, Cout)
        got["dsum"] = ws.out[parts:].reshape(parts, 4)
    res = E.dl_check(c, d, got, what=what)
    report("deconv_last_fused", f"<{'ONE' if C1 == 64 else 'pipelined'}> {c['id']}", "bf16", res)


# ---- rbvae_conv_in -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", E.CI_CASES, ids=ids(E.CI_CASES))
def test_conv_in_bounded_and_guarded(lib, c):
    N, Cin, H, W, Nout, cg, ldo = c["N"], c["Cin"], c["H"], c["W"], c["Nout"], c["cg"], c["ldo"]
    assert lib.query("rbvae_conv_in_ok", 1, Cin, H, W, Nout, N, cg) == E.conv_in_ok("bf16", Cin, H, W, Nout, N, cg) == 1
    nst = lib.query("rbvae_conv_in_stats_floats", N, H, W, Nout, cg)
    assert nst == E.conv_in_stats_floats(N, H, W, Nout, cg)
    d = E.ci_build(c)
    x = flat_in(d["x"])
    Wp = B.poisoned(d["Wp"], 64, BF)
    bias = f32_row(d["bias"]) if d["bias"] is not None else None
    inst = E.ci_instance(Cin, Nout)
    outs = []
    for with_stats in (True, False):
        out = B.guarded(N * H * W, ldo, Nout, BF)
        stats = B.GuardedFlat(nst, F32) if with_stats else None
        lib.call("rbvae_conv_in", 1, x.view, Wp.view, bias and bias.view, zero_page(), out.view, stats and stats.view, cg, N, Cin,
                 H, W, Nout, ldo)
        torch.cuda.synchronize()
        B.assert_guards(out, f"{c['id']} {inst} out")
        if stats is not None:
            B.assert_guards(stats, f"{c['id']} {inst} stats")
        outs.append((out, stats))
    out, stats = outs[0]
    res = E.ci_check(c, d, dict(out=out.out, stats=stats.out), what=f"{c['id']} {inst}")
    assert torch.equal(bits16(out.out), bits16(outs[1][0].out)), f"{c['id']}: stats_part = NULL changes the output"
    # rbvae_gn_finish_tiles(.., 8, 16) over the partials: per (image, group) mean / rstd
    G, eps = Nout // cg, 1e-6
    g = torch.Generator().manual_seed(len(c["id"]))
    gamma, beta = torch.randn(Nout, generator=g), torch.randn(Nout, generator=g)
    sc, sh = B.guarded(N, Nout, Nout, F32), B.guarded(N, Nout, Nout, F32)
    mo, ro = B.GuardedFlat(N * G, F32), B.GuardedFlat(N * G, F32)
    lib.call("rbvae_gn_finish_tiles", stats.view, f32_row(gamma).view, f32_row(beta).view, sc.view, sh.view, mo.view, ro.view, N,
             H, W, Nout, G, eps, 8, 16)
    torch.cuda.synchronize()
    for buf, nm in ((sc, "scale"), (sh, "shift"), (mo, "mean_out"), (ro, "rstd_out")):
        B.assert_guards(buf, f"{c['id']} gn_finish {nm}")
    mean, rstd, bmean, brstd = E.ci_gn_finish_ref(c, out.out.cpu(), eps)
    rm = (mo.out.cpu().double().reshape(N, G) - mean).abs() / bmean
    rr = (ro.out.cpu().double().reshape(N, G) - rstd).abs() / brstd
    assert bool((rm <= 1).all()), (c["id"], "gn_finish mean", float(rm.max()))
    assert bool((rr <= 1).all()), (c["id"], "gn_finish rstd", float(rr.max()))
    res["gn_finish"] = max(float(rm.max()), float(rr.max()))
    report("conv_in", f"<{Cin},{inst[2]}> cg{cg} {c['id']}", "bf16", res)


# ---- the two-kernel path: rbvae_im2col(_frames), rbvae_col2im_sigmoid(_frames), rbvae_sigmoid_bwd_nhwc ---------------------

@pytest.mark.parametrize("c", E.IM_CASES, ids=ids(E.IM_CASES))
def test_im2col_bit_for_bit_and_guarded(lib, c):
    N, C, H, W, Kpad, tdt = c["N"], c["C"], c["H"], c["W"], c["Kpad"], E.TDT[c["dtype"]]
    d = E.im_build(c)
    sc, sh, sw = (H * W, W, 1) if c["layout"] == "nchw" else (1, W * C, C)
    x, fm = frames_in(d["x_store"], c["fmap"])
    col = B.guarded(N * d["OH"] * d["OW"], Kpad, Kpad, tdt)
    tail = (sc, sh, sw, N, C, H, W, d["OH"], d["OW"], 3, 3, c["stride"], 1, Kpad, col.view)
    if c["fmap"] is None:
        lib.call("rbvae_im2col", E.DTYPE_ID[c["dtype"]], x.view, fm[4], *tail)
    else:
        lib.call("rbvae_im2col_frames", E.DTYPE_ID[c["dtype"]], x.view, *fm, *tail)
    torch.cuda.synchronize()
    B.assert_guards(col, f"{c['id']} col")
    assert E.same_bits(col.out.cpu(), d["want"]), f"{c['id']} {E.im_kernel(c)}: col differs from the host gather"


@pytest.mark.parametrize("c", E.C2_CASES, ids=ids(E.C2_CASES))
def test_col2im_sigmoid_bounded_and_guarded(lib, c):
    N, IH, IW, Cout, ldy, tdt = c["N"], c["IH"], c["IW"], c["Cout"], c["ldy"], E.TDT[c["dtype"]]
    OH, OW, tot, nb, kern = E.c2_geom(c)
    assert lib.query("rbvae_col2im_nparts", tot) == nb
    has_dcol = lib.query("rbvae_col2im_has_dcol", N, IH, IW, ldy, OH, OW, Cout)
    assert has_dcol == E.col2im_has_dcol(N, IH, IW, ldy, OH, OW, Cout) == (1 if kern == "pix" else 0)
    d = E.c2_build(c)
    Y = B.poisoned(d["Y"], ldy, tdt)
    bias = f32_row(d["bias"]) if d["bias"] is not None else None
    xr = B.GuardedFlat(tot, F32)
    tgt, fm, ws, dpre, mse, gs = None, (0, 0, 0, 0, Cout * OH * OW), None, None, None, None
    if d["target"] is not None:
        tgt, fm = frames_in(d["target"], None if c["target"] == "plain" else c["target"])
        ws = B.GuardedFlat(5 * nb if (c["dpre"] and kern == "pix") else nb, F32)
        dpre = B.GuardedFlat(tot, F32) if c["dpre"] else None
        mse = B.GuardedFlat(1, F32) if c["sse_mean"] else None
        gs = f32_row(torch.tensor([d["gs"]])) if c["gs_dev"] else None
    head = (E.DTYPE_ID[c["dtype"]], Y.view, ldy, bias and bias.view, N, IH, IW, OH, OW, Cout, 3, 3, 1, xr.view, tgt and tgt.view)
    tail = (mse and mse.view, ws and ws.view, dpre and dpre.view, c["gscale"], gs and gs.view)
    if c["target"] in (None, "plain"):
        lib.call("rbvae_col2im_sigmoid", *head, *tail)
    else:
        lib.call("rbvae_col2im_sigmoid_frames", *head, *fm, *tail)
    torch.cuda.synchronize()
    what = f"{c['id']} col2im_sigmoid_{kern}"
    for g, nm in ((xr, "xr"), (ws, "ws"), (dpre, "dpre"), (mse, "sse_mean")):
        if g is not None:
            B.assert_guards(g, f"{what} {nm}")
    got = dict(xr=xr.out.reshape(N, Cout, OH, OW))
    if ws is not None:
        got["sse"] = ws.out[:nb]
    if dpre is not None:
        got["dpre"] = dpre.out.reshape(N, OH, OW, Cout)
        if kern == "pix":
            got["dsum"] = ws.out[nb:].reshape(nb, 4)
    if mse is not None:
        got["sse_mean"] = mse.out.cpu()[0]
    report("col2im_sigmoid", f"{kern} {c['id']}", c["dtype"], E.c2_check(c, d, got, what=what))


def test_sigmoid_bwd_nhwc_is_its_definition(lib):
    g0 = torch.Generator().manual_seed(31)
    for (N, C, H, W) in ((2, 3, 9, 17), (1, 4, 16, 32), (3, 1, 1, 1), (1, 5, 7, 300)):
        g, xr = torch.randn(N, C, H, W, generator=g0), torch.rand(N, C, H, W, generator=g0)
        out = B.GuardedFlat(N * C * H * W, F32)
        lib.call("rbvae_sigmoid_bwd_nhwc", flat_in(g).view, flat_in(xr).view, out.view, N, C, H, W)
        torch.cuda.synchronize()
        B.assert_guards(out, "sigmoid_bwd_nhwc dpre")
        report("sigmoid_bwd_nhwc", f"{N}x{C}x{H}x{W}", "f32", E.sb_check(g, xr, out.out.reshape(N, H, W, C)))


# ---- refusals: every gate and argument check returns before a launch and writes nothing ------------------------------------

def test_refusals_raise_and_write_nothing(lib):
    z = zero_page()
    N, Cin, IH, IW, Nout = 2, 3, 15, 17, 64
    OH, OW = E.s2_out(IH, IW)
    P = N * OH * OW
    x = flat_in(torch.zeros(N * Cin * IH * IW))
    W = B.poisoned(torch.zeros(320, 64), 64, BF)
    bias = f32_row(torch.zeros(320))
    out, col = B.guarded(P, 328, 320, BF), B.guarded(P, 64, 64, BF)
    gate = B.poisoned(torch.ones(P, 320), 328, BF)
    ws = B.guarded(8, 320, 320, F32)
    slabs = B.guarded(9 * 320, 64, 64, F32)
    off = lambda g, k: g.view.data_ptr() + k

    def cf_args(dtype=1, Cin=Cin, Nout=Nout, ldo=Nout, drop_mode=0, W_=None, out_=None, bias_=None):
        return (dtype, x.view, 0, 0, 0, 0, Cin * IH * IW, W_ or W.view, bias_ or bias.view, z, col.view, out_ or out.view, N, Cin, IH,
                IW, Nout, ldo, 1, drop_mode, 0.0, 1.0, 0, None)
    cf_bad = [dict(dtype=0), dict(Cin=5), dict(Cin=0), dict(Nout=12), dict(Nout=264, ldo=264), dict(ldo=Nout + 4), dict(ldo=Nout - 8),
              dict(drop_mode=2), dict(W_=off(W, 2)), dict(out_=off(out, 2)), dict(bias_=off(bias, 4))]
    for kw in cf_bad:
        if {"dtype", "Cin", "Nout"} & set(kw):
            assert lib.query("rbvae_conv_first_fused_ok", kw.get("dtype", 1), kw.get("Cin", Cin), IH, IW, kw.get("Nout", Nout), N) == 0
        with pytest.raises(ValueError):
            lib.call("rbvae_conv_first_fused", *cf_args(**kw))
    with pytest.raises(ValueError):                                             # null weights
        lib.call("rbvae_conv_first_fused", 1, x.view, 0, 0, 0, 0, Cin * IH * IW, None, bias.view, z, col.view, out.view, N, Cin, IH, IW,
                 Nout, Nout, 1, 0, 0.0, 1.0, 0, None)

    def dg_args(dtype=1, Cout=Cin, C1=Nout, ldo=Nout, gate_=None):
        return (dtype, x.view, W.view, z, col.view, gate_ or gate.view, out.view, N, Cout, IH, IW, C1, ldo, 1.0, ws.view)
    for kw in (dict(dtype=0), dict(Cout=5), dict(C1=264, ldo=264), dict(C1=20), dict(ldo=Nout + 4), dict(gate_=off(gate, 2))):
        if {"dtype", "Cout", "C1"} & set(kw):
            assert lib.query("rbvae_deconv_last_dgrad_blocks", kw.get("dtype", 1), kw.get("Cout", Cin), IH, IW, kw.get("C1", Nout), N) == 0
        with pytest.raises(ValueError):
            lib.call("rbvae_deconv_last_dgrad_fused", *dg_args(**kw))

    nblk = E.s2_blocks(N, IH, IW)
    dy = B.poisoned(torch.zeros(P, 320), 328, BF)

    def wf_args(dtype=1, mode=0, Cin=Cin, Nout=Nout, ldy=328, ks=2, dy_=None):
        return (dtype, mode, x.view, 0, 0, 0, 0, Cin * IH * IW, dy_ or dy.view, slabs.view, z, N, Cin, IH, IW, Nout, ldy, ks)
    for kw in (dict(dtype=0), dict(mode=2), dict(Cin=5), dict(Nout=72), dict(Nout=32), dict(ldy=332), dict(ldy=56), dict(ks=0),
               dict(ks=nblk + 1), dict(dy_=off(dy, 2))):
        if "Nout" in kw or "Cin" in kw or "dtype" in kw:
            assert lib.query("rbvae_wgrad_first_blocks", kw.get("dtype", 1), kw.get("Cin", Cin), IH, IW, kw.get("Nout", Nout), N) == 0
        with pytest.raises(ValueError):
            lib.call("rbvae_wgrad_first", *wf_args(**kw))
    untouched(out, col, ws, slabs)

    # rbvae_deconv_last_fused
    n, ih, iw, C1, Cout = 2, 9, 17, 128, 3
    oh, ow = 2 * ih, 2 * iw
    D2 = B.poisoned(torch.zeros(n * ih * iw, 128), 128, BF)
    V = B.poisoned(torch.zeros(48, 128), 128, BF)
    b4 = f32_row(torch.zeros(8))
    xr, dpre, wsl = B.GuardedFlat(n * 5 * oh * ow, F32), B.GuardedFlat(n * oh * ow * 5, F32), B.GuardedFlat(5 * 8, F32)
    tg = flat_in(torch.zeros(n * 5 * oh * ow))

    def dl_args(dtype=1, C1=C1, Cout=Cout, NYP=32, target=True, ws_=True, dpre_=None):
        return (dtype, D2.view, V.view, NYP, b4.view, z, n, ih, iw, C1, Cout, xr.view, tg.view if target else None, 0, 0, 0, 0,
                Cout * oh * ow, wsl.view if ws_ else None, dpre.view if dpre_ is None else dpre_, 0.5)
    for kw in (dict(dtype=0), dict(C1=96), dict(C1=32), dict(Cout=5), dict(Cout=0), dict(NYP=24), dict(NYP=56), dict(target=False),
               dict(ws_=False), dict(dpre_=off(dpre, 4))):
        if {"dtype", "C1", "Cout"} & set(kw):
            assert lib.query("rbvae_deconv_last_fused_parts", kw.get("dtype", 1), n, ih, iw, kw.get("C1", C1), kw.get("Cout", Cout)) == 0
        with pytest.raises(ValueError):
            lib.call("rbvae_deconv_last_fused", *dl_args(**kw))
    untouched(xr, dpre, wsl)

    # rbvae_conv_in
    H, Wd = 9, 17
    xi = flat_in(torch.zeros(n * 4 * H * Wd))
    oi, st = B.guarded(n * H * Wd, 328, 320, BF), B.GuardedFlat(2 * n * 4 * 80, F32)

    def ci_args(dtype=1, Cin=3, Nout=64, ldo=64, cg=8, st_=None):
        return (dtype, xi.view, W.view, bias.view, z, oi.view, st.view if st_ is None else st_, cg, n, Cin, H, Wd, Nout, ldo)
    for kw in (dict(dtype=0), dict(Cin=5), dict(Nout=264, ldo=264), dict(Nout=20), dict(cg=5), dict(cg=32), dict(Nout=72, cg=16, ldo=72),
               dict(ldo=68), dict(ldo=56), dict(st_=off(st, 4))):
        if {"dtype", "Cin", "Nout", "cg"} & set(kw):
            assert lib.query("rbvae_conv_in_ok", kw.get("dtype", 1), kw.get("Cin", 3), H, Wd, kw.get("Nout", 64), n, kw.get("cg", 8)) == 0
        with pytest.raises(ValueError):
            lib.call("rbvae_conv_in", *ci_args(**kw))
    untouched(oi, st)

    # rbvae_im2col(_frames) and rbvae_col2im_sigmoid
    ci_ = B.guarded(P, 64, 64, BF)
    im = lambda Kpad=64, col_=None: (1, x.view, Cin * IH * IW, IH * IW, IW, 1, N, Cin, IH, IW, OH, OW, 3, 3, 2, 1, Kpad, col_ or ci_.view)
    for args in (im(Kpad=20), im(Kpad=28), im(col_=off(ci_, 2))):
        with pytest.raises(ValueError):
            lib.call("rbvae_im2col", *args)
    with pytest.raises(ValueError):                                             # d1 not a multiple of d2
        lib.call("rbvae_im2col_frames", 1, x.view, 3, 2, 0, 0, Cin * IH * IW, IH * IW, IW, 1, N, Cin, IH, IW, OH, OW, 3, 3, 2, 1, 64, ci_.view)
    with pytest.raises(ValueError):
        lib.call("rbvae_im2col", 7, x.view, Cin * IH * IW, IH * IW, IW, 1, N, Cin, IH, IW, OH, OW, 3, 3, 2, 1, 64, ci_.view)
    Y = B.poisoned(torch.zeros(n * ih * iw, 32), 32, F32)
    mse = B.GuardedFlat(1, F32)

    def c2_args(dtype=0, ldy=32, target=True, mse_=True, ws_=True, dpre_=True):
        return (dtype, Y.view, ldy, b4.view, n, ih, iw, oh, ow, Cout, 3, 3, 1, xr.view, tg.view if target else None,
                mse.view if mse_ else None, wsl.view if ws_ else None, dpre.view if dpre_ else None, 0.5, None)
    for kw in (dict(dtype=7), dict(ldy=24), dict(ws_=False), dict(target=False), dict(target=False, mse_=False, ws_=False)):
        with pytest.raises(ValueError):
            lib.call("rbvae_col2im_sigmoid", *c2_args(**kw))
    untouched(ci_, xr, dpre, wsl, mse)
