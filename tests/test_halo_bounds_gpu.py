"""Element-wise bounds and guarded stores for the halo kernels (tests/_halo_cases.py holds the cases, the restated
dispatch and the float64 references; tests/_bounds.py the error model):

  rbvae_conv3x3_halo       conv_halo_k<float | bf16, 3, GN> and conv_halo_ws_k<GN>, GroupNorm (+ swish) staging with the
                           unrounded f64 operand and its u_in term, per-tile (mean, M2) statistics, rbvae_gn_finish_tiles
  rbvae_deconv3x3s2_halo   every deconv_halo_k<T, SC, WAVES> the dispatch reaches, forward and gradient forms, colsum rows
  rbvae_wgrad3x3s2_halo    each K-slice slab against its own pixels, empty slices exactly zero, XCD padding writes nothing
  rbvae_wgrad3x3s2_row     the same for wgrad_row_k<8> and <4>

Outputs, statistics, workspaces and slabs sit inside NaN guard bands (no stray store, every declared element written);
inputs inside NaN guard rows and NaN padding columns (lda > Kc, ldo > Nout)."""
import pytest
import torch

import _bounds as B
import _halo_cases as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import sfv_amd
    return sfv_amd._lib


def zero_page():
    return torch.zeros(256, dtype=torch.uint8, device="cuda")


def report(kind, c, dtype, worst):
    print(f"\nBOUNDS {kind} {c} {dtype} worst |err|/bound = {worst:.3g}")


def f32_row(t):
    """A [1][n] f32 vector inside NaN guard rows (bias, per-image scale / shift rows use poisoned directly)."""
    t = t.reshape(1, -1).float()
    return B.poisoned(t, t.shape[1], torch.float32)


def run_conv(lib, c, d, variant, ops, out, stats):
    l = lib.dbg_lib()
    old = l.rbvae_dbg_conv_halo_variant(variant)
    try:
        OH, OW = H.ch_geometry(c)[:2]
        lib.call("rbvae_conv3x3_halo", H.DTYPE_ID[c["dtype"]], ops["A"].view, ops["W"].view, out.view,
                 ops["bias"] and ops["bias"].view, ops["addend"] and ops["addend"].view, zero_page(),
                 ops["scale"] and ops["scale"].view, ops["shift"] and ops["shift"].view, c["swish"],
                 stats and stats.view, c["stats_cg"], c["N"], c["IH"], c["IW"], OH, OW, c["pad"][0], c["pad"][1], c["Kc"],
                 c["Nout"], c["lda"], c["ldo"])
        torch.cuda.synchronize()
    finally:
        l.rbvae_dbg_conv_halo_variant(old)


def conv_operands(c, d):
    tdt = H.TDT[c["dtype"]]
    return dict(A=B.poisoned(d["A"], c["lda"], tdt), W=B.poisoned(d["Wp"], 9 * c["Kc"], tdt),
                bias=f32_row(d["bias"]) if d["bias"] is not None else None,
                addend=B.poisoned(d["addend"], c["ldo"], tdt) if d["addend"] is not None else None,
                scale=B.poisoned(d["scale"], c["Kc"], torch.float32) if d["scale"] is not None else None,
                shift=B.poisoned(d["shift"], c["Kc"], torch.float32) if d["shift"] is not None else None)


@pytest.mark.parametrize("c", H.CH_CASES, ids=[c["id"] for c in H.CH_CASES])
def test_conv3x3_halo_bounded_and_guarded(lib, c):
    tdt, N, Nout, cg = H.TDT[c["dtype"]], c["N"], c["Nout"], c["stats_cg"]
    OH, OW, tr, tc, mtiles, total = H.ch_geometry(c)
    assert lib.query("rbvae_conv3x3_halo_ok", H.DTYPE_ID[c["dtype"]], c["IH"], c["IW"], OH, OW, c["Kc"], Nout)
    d = H.ch_build(c)
    ops = conv_operands(c, d)
    tile = H.ch_tile_of_rows(c)
    for variant in H.ch_variants(c):
        kern = H.ch_kernel(c, variant)
        what = f"{c['id']} {kern}"
        out = B.guarded(N * OH * OW, c["ldo"], Nout, tdt)
        stats = None
        if cg:
            nst = lib.query("rbvae_conv3x3_halo_stats_floats", N, OH, OW, Nout, cg)
            assert nst == 2 * mtiles * (Nout // cg)
            stats = B.GuardedFlat(nst, torch.float32)
        run_conv(lib, c, d, variant, ops, out, stats)
        B.assert_guards(out, f"{what} Out")
        worst = B.check(out.out, d["ref"], d["S"], out_dtype=tdt, K=d["K"], pre=d["pre"], nhw=d["nhw"], what=what,
                        S_in=d["S_in"], u_in=d["u_in"])
        report("conv3x3_halo", f"{kern}{'<GN>' if c['gn'] else ''} {c['id']}", c["dtype"], worst)
        if stats is None:
            continue
        B.assert_guards(stats, f"{what} stats")
        stored = out.out.cpu()
        wm, w2 = H.check_tile_stats(stats.out.reshape(-1, 2), stored, tile, mtiles, cg, what=f"{what} cg {cg}")
        report("conv3x3_halo_stats", f"{kern} cg{cg} {c['id']}", c["dtype"], max(wm, w2))
        if cg > 64:
            continue
        # rbvae_gn_finish_tiles(.., 16, 16) over the same partials: per (image, group) mean / rstd, then scale / shift
        G, eps = Nout // cg, 1e-6
        g = torch.Generator().manual_seed(len(c["id"]))
        gamma, beta = torch.randn(Nout, generator=g), torch.randn(Nout, generator=g)
        sc, sh = B.guarded(N, Nout, Nout, torch.float32), B.guarded(N, Nout, Nout, torch.float32)
        mo, ro = B.GuardedFlat(N * G, torch.float32), B.GuardedFlat(N * G, torch.float32)
        lib.call("rbvae_gn_finish_tiles", stats.view, f32_row(gamma).view, f32_row(beta).view, sc.view, sh.view, mo.view,
                 ro.view, N, OH, OW, Nout, G, eps, 16, 16)
        torch.cuda.synchronize()
        for buf, nm in ((sc, "scale"), (sh, "shift"), (mo, "mean_out"), (ro, "rstd_out")):
            B.assert_guards(buf, f"{what} gn_finish {nm}")
        mean, rstd, bmean, brstd = H.gn_finish_ref(stored, tile, c, cg, eps)
        gm, gr = mo.out.cpu().double().reshape(N, G), ro.out.cpu().double().reshape(N, G)
        rm, rr = (gm - mean).abs() / bmean, (gr - rstd).abs() / brstd
        assert bool((rm <= 1).all()), (what, "gn_finish mean", float(rm.max()))
        assert bool((rr <= 1).all()), (what, "gn_finish rstd", float(rr.max()))
        # scale = rstd gamma, shift = beta - mean scale (per image and channel)
        ga, be = gamma.double(), beta.double()
        rs_c, m_c = rstd.repeat_interleave(cg, 1), mean.repeat_interleave(cg, 1)
        bm_c, br_c = bmean.repeat_interleave(cg, 1), brstd.repeat_interleave(cg, 1)
        want_sc = rs_c * ga
        b_sc = ga.abs() * (br_c + B.U32 * rs_c) + B.TINY
        want_sh = be - m_c * want_sc
        b_sh = m_c.abs() * b_sc + want_sc.abs() * bm_c + 2 * B.U32 * (be.abs() + 2 * (m_c * want_sc).abs()) + B.TINY
        rsc = (sc.out.cpu().double() - want_sc).abs() / b_sc
        rsh = (sh.out.cpu().double() - want_sh).abs() / b_sh
        assert bool((rsc <= 1).all()), (what, "gn_finish scale", float(rsc.max()))
        assert bool((rsh <= 1).all()), (what, "gn_finish shift", float(rsh.max()))
        report("gn_finish_tiles", f"cg{cg} {c['id']}", c["dtype"],
               max(float(rm.max()), float(rr.max()), float(rsc.max()), float(rsh.max())))


def test_conv3x3_halo_default_dispatch_512_items_is_variant0_bit_for_bit(lib):
    """>= 512 work items: the product dispatch (variant 2) runs conv_halo_ws_k; its output and statistics are the same
    bits as variant 0, and both launches stay inside their buffers (an f64 reference at this size is ~1e10 MACs)."""
    c = H.CH_BIG
    assert H.ch_kernel(c, 2) == H.ch_kernel(c, 0) == "conv_halo_ws_k"
    N, Nout, cg = c["N"], c["Nout"], c["stats_cg"]
    OH, OW = H.ch_geometry(c)[:2]
    d = H.ch_build(c, reference=False)
    ops = conv_operands(c, d)
    res = []
    for variant in (2, 0):
        out = B.guarded(N * OH * OW, c["ldo"], Nout, torch.bfloat16)
        stats = B.GuardedFlat(lib.query("rbvae_conv3x3_halo_stats_floats", N, OH, OW, Nout, cg), torch.float32)
        run_conv(lib, c, d, variant, ops, out, stats)
        B.assert_guards(out, f"variant {variant} Out")
        B.assert_guards(stats, f"variant {variant} stats")
        res.append((out.out.contiguous().view(torch.int16).cpu(), stats.out.view(torch.int32).cpu()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


@pytest.mark.parametrize("c", H.DH_CASES, ids=[c["id"] for c in H.DH_CASES])
def test_deconv3x3s2_halo_bounded_and_guarded(lib, c):
    tdt, dt, N, TH, TW, Kc, Nout = H.TDT[c["dtype"]], H.DTYPE_ID[c["dtype"]], c["N"], c["TH"], c["TW"], c["Kc"], c["Nout"]
    bm = H.dh_tile_rows(c["dtype"], N, TH, TW, Kc, Nout)
    assert bm and lib.query("rbvae_deconv3x3s2_halo_tile_rows", dt, N, TH, TW, Kc, Nout) == bm
    inst = H.dh_instance(c)
    d = H.dh_build(c)
    A = B.poisoned(d["A"], c["lda"], tdt)
    Wp = B.poisoned(d["Wp"], 9 * Kc, tdt)
    out = B.guarded(d["rows"], c["ldo"], Nout, tdt)
    bias = f32_row(d["bias"]) if d["bias"] is not None else None
    gate = B.poisoned(d["gate"], c["ldo"], tdt) if d["gate"] is not None else None
    keep = d["keep"].to(torch.uint8).cuda() if d["keep"] is not None else None
    ws = None
    if c["form"] == "gradient":
        nrow = lib.query("rbvae_deconv3x3s2_halo_colsum_rows", dt, N, TH, TW, Kc, Nout)
        assert nrow == H.dh_colsum_rows(c)
        ws = B.guarded(nrow, Nout, Nout, torch.float32)
    lib.call("rbvae_deconv3x3s2_halo", dt, A.view, Wp.view, out.view, bias and bias.view, gate and gate.view, keep,
             zero_page(), N, TH, TW, Kc, Nout, c["lda"], c["ldo"], d["relu"], 2 if keep is not None else 0, 0.2,
             d["scale"], 0, None, ws and ws.view)
    torch.cuda.synchronize()
    what = f"{c['id']} deconv_halo_k<{inst[0]}, {inst[1]}, {inst[2]}>"
    B.assert_guards(out, f"{what} Out")
    worst = B.check(out.out, d["ref"], d["S"], out_dtype=tdt, K=d["K"], scale=d["scale"], nhw=d["nhw"], what=what)
    report("deconv3x3s2_halo", f"<{inst[1]},{inst[2]}> {c['form']} {c['id']}", c["dtype"], worst)
    if ws is not None:
        B.assert_guards(ws, f"{what} colsum_ws")
        want, bnd = H.dh_colsum_ref(c, out.out.cpu())
        r = (ws.out.cpu().double() - want).abs() / bnd
        assert bool((r <= 1).all()), (what, "colsum row", int(r.max(1).values.argmax()), float(r.max()))
        report("deconv3x3s2_halo_colsum", c["id"], c["dtype"], float(r.max()))


@pytest.mark.parametrize("c", H.WK_CASES, ids=[c["id"] for c in H.WK_CASES])
def test_wgrad3x3s2_halo_and_row_slabs_bounded_and_guarded(lib, c):
    kind, N, OH, OW, Ca, Cb, ks = c["kind"], c["N"], c["OH"], c["OW"], c["Ca"], c["Cb"], c["ks"]
    name = f"rbvae_wgrad3x3s2_{kind}"
    assert lib.query(name + "_ok", 1, N, OH, OW, Ca, Cb)
    nblk = lib.query(name + "_blocks", N, OH, OW)
    assert nblk == (H.wh_blocks(N, OH, OW) if kind == "halo" else H.wr_blocks(N, OH, OW))
    d = H.wk_build(c)
    Sg = B.poisoned(d["S"], c["lds"], torch.bfloat16)
    Gg = B.poisoned(d["G"], c["ldg"], torch.bfloat16)
    slab = Ca * 9
    slabs = B.guarded(ks * slab, Cb, Cb, torch.float32, guard_rows=slab)      # a whole guard slab on each side
    lib.call(name, 1, Sg.view, Gg.view, slabs.view, zero_page(), N, OH, OW, Ca, Cb, c["lds"], c["ldg"], ks)
    torch.cuda.synchronize()
    kern = "wgrad_halo_k" if kind == "halo" else f"wgrad_row_k<{H.wr_width(OW)}>"
    B.assert_guards(slabs, f"{c['id']} {kern} slabs")
    worst = H.check_slabs(slabs.out.reshape(ks, Ca, 9 * Cb), d, c, what=f"{c['id']} {kern}")
    report("wgrad3x3s2", f"{kern} {c['id']}", "bf16", worst)
