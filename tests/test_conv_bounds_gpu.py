"""Element-wise bounds and guarded stores for the conv / GEMM kernels: every gather_gemm and wgrad_gemm template instance
the build dispatches to (tests/_conv_cases.py restates the dispatch), rbvae_fc_gemm and rbvae_conv3x3s2_halo.

Each case compares the kernel with a float64 reference of the same operands element by element under the error model
of tests/_bounds.py, with outputs inside NaN guard bands (no stray store, every declared element written), inputs inside
NaN guard rows and NaN padding columns (no read the ABI does not allow), and workspaces sized by the kernel's own query
and prefilled with NaN."""
import ctypes

import pytest
import torch

import _bounds as B
import _conv_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import sfv_amd
    return sfv_amd._lib


def zero_page():
    return torch.zeros(256, dtype=torch.uint8, device="cuda")


def report(kind, c, dtype, worst):
    print(f"\nBOUNDS {kind} {c} {dtype} worst |err|/bound = {worst:.3g}")


@pytest.mark.parametrize("c", C.GG_CASES, ids=[c["id"] for c in C.GG_CASES])
def test_gather_gemm_bounded_and_guarded(lib, c):
    tdt, Kc, Nout, e = C.TDT[c["dtype"]], c["Kc"], c["Nout"], c["epi"]
    assert C.gg_case_instance(c)[0] == c["inst"]
    d = C.gg_build(c)
    A = B.poisoned(d["A"], c["lda"], tdt)
    Wp = B.poisoned(d["Wp"], d["Wp"].shape[1], tdt)
    out = B.guarded(d["rows"], c["ldo"], Nout, tdt)
    gate = B.poisoned(d["gate"], c["ldo"], tdt) if d["gate"] is not None else None
    addend = B.poisoned(d["addend"], c["ldo"], tdt) if d["addend"] is not None else None
    keep = d["keep"].to(torch.uint8).cuda() if d["keep"] is not None else None
    bias = d["bias"].cuda() if d["bias"] is not None else None
    mt = C.cdiv(d["Mc"], 128)
    ws = B.guarded(d["ncls"] * mt, Nout, Nout, torch.float32) if e.get("colsum") else None
    desc = (ctypes.c_int * len(d["desc"]))(*d["desc"])
    lib.call("rbvae_gather_gemm", C.DTYPE_ID[c["dtype"]], A.view, Wp.view, out.view, bias, gate and gate.view, keep,
             addend and addend.view, zero_page(), *d["geom"], Kc, Nout, c["lda"], c["ldo"], d["taps"], d["ncls"],
             ctypes.addressof(desc), int(bool(e.get("relu"))), 2 if keep is not None else 0, 0.2, d["scale"], 0, None,
             ws and ws.view)
    torch.cuda.synchronize()
    B.assert_guards(out, f"{c['id']} Out")
    worst = B.check(out.out, d["ref"], d["S"], out_dtype=tdt, K=d["K"], scale=d["scale"], pre=d["pre"], nhw=d["nhw"],
                    what=c["id"])
    report("gather_gemm", c["inst"], c["dtype"], worst)
    if ws is not None:
        # each per-tile row against the f64 sum of the kernel's own stored rows of that tile: pins the layout
        B.assert_guards(ws, f"{c['id']} colsum_ws")
        stored = out.out.double().cpu()
        orow = C.gg_out_rows(c)                                               # [ncls][Mc]
        tile = (torch.arange(d["ncls"])[:, None] * mt + torch.arange(d["Mc"])[None, :] // 128).reshape(-1)
        vals = stored[orow.reshape(-1)]
        want = torch.zeros(d["ncls"] * mt, Nout, dtype=torch.float64).index_add_(0, tile, vals)
        absw = torch.zeros_like(want).index_add_(0, tile, vals.abs())
        err = (ws.out.double().cpu() - want).abs()
        bnd = 127 * 2.0 ** -24 * absw + B.TINY
        assert bool((err <= bnd).all()), (c["id"], "colsum", float((err / bnd).max()))


@pytest.mark.parametrize("c", C.WG_CASES, ids=[c["id"] for c in C.WG_CASES])
def test_wgrad_gemm_bounded_and_guarded(lib, c):
    tdt, Co, Ci, ks = C.TDT[c["dtype"]], c["Co"], c["Ci"], c["ks"]
    assert C.wg_case_instance(c)[0] == c["inst"]
    d = C.wg_build(c)
    P, taps = d["P"], d["taps"]
    Dy = B.poisoned(d["Dy"], c["ldy"], tdt)
    In = B.poisoned(d["In"], c["ldi"], tdt)
    slab = Co * taps
    slabs = B.guarded(ks * slab, Ci, Ci, torch.float32, guard_rows=slab)     # a whole guard slab on each side
    idx = None
    if d["conv"] is not None:
        N, H, W, Ho, Wo = d["conv"]
        idx = torch.empty(9 * P, dtype=torch.int32, device="cuda")
        lib.call("rbvae_conv_gather_index", idx, N, H, W, Ho, Wo, 3, 3, 2, 1)
    lib.call("rbvae_wgrad_gemm", C.DTYPE_ID[c["dtype"]], Dy.view, In.view, slabs.view, idx, zero_page(), P,
             d["in_rows"], Co, Ci, c["ldy"], c["ldi"], taps, ks)
    torch.cuda.synchronize()
    B.assert_guards(slabs, f"{c['id']} slabs")
    got = slabs.out.double().cpu().reshape(ks, slab, Ci).sum(0).reshape(Co, taps * Ci)
    pper = C.cdiv(C.cdiv(P, ks), 64) * 64
    worst = B.check(got, d["ref"], d["S"], out_dtype=torch.float32, K=min(P, pper), what=c["id"])
    report("wgrad_gemm", c["inst"], c["dtype"], worst)


@pytest.mark.parametrize("M,N,lda,K,with_bias", [(37, 1024, 72, 64, True), (300, 2064, 64, 64, False),
                                                 (70, 1040, 136, 128, True), (200, 32768, 72, 64, False),
                                                 (513, 8192, 64, 64, True)])
def test_fc_gemm_bounded_and_guarded(lib, M, N, lda, K, with_bias):
    """rbvae_fc_gemm (both tile shapes: N % 128 == 0 with >= 256 workgroups takes the wide one) with its per-128-row
    column sums."""
    ldo = N + 8 if lib.query("rbvae_fc_gemm_ok", 1, M, K, N, lda, N + 8) else N
    assert lib.query("rbvae_fc_gemm_ok", 1, M, K, N, lda, ldo)
    g = torch.Generator().manual_seed(M + N)
    A = torch.randn(M, K, generator=g).bfloat16()
    W = (torch.randn(N, K, generator=g) / K ** 0.5).bfloat16()
    ref, S = B.ref_and_scale("linear", A, W)
    bias = torch.randn(N, generator=g) if with_bias else None
    if bias is not None:
        ref, S = ref + bias.double(), S + bias.double().abs()
    Ag = B.poisoned(A, lda, torch.bfloat16)
    Wg = B.poisoned(W, K, torch.bfloat16)
    out = B.guarded(M, ldo, N, torch.bfloat16)
    mt = C.cdiv(M, 128)
    ws = B.guarded(mt, N, N, torch.float32)
    lib.call("rbvae_fc_gemm", 1, Ag.view, Wg.view, out.view, bias.cuda() if bias is not None else None, ws.view,
             M, K, N, lda, ldo)
    torch.cuda.synchronize()
    B.assert_guards(out, "fc_gemm Out")
    B.assert_guards(ws, "fc_gemm colsum_ws")
    worst = B.check(out.out, ref, S, out_dtype=torch.bfloat16, K=K, what=f"fc_gemm {M}x{N}x{K}")
    report("fc_gemm", f"M{M}N{N}K{K}", "bf16", worst)
    stored = out.out.double().cpu()
    tile = torch.arange(M) // 128
    want = torch.zeros(mt, N, dtype=torch.float64).index_add_(0, tile, stored)
    absw = torch.zeros_like(want).index_add_(0, tile, stored.abs())
    assert bool(((ws.out.double().cpu() - want).abs() <= 127 * 2.0 ** -24 * absw + B.TINY).all())


@pytest.mark.parametrize("N,Kc,Nout,IH,IW", [(2, 32, 128, 16, 32), (2, 256, 256, 44, 80), (5, 96, 128, 8, 8),
                                             (1, 128, 256, 34, 66), (1, 64, 128, 2, 2)])
@pytest.mark.parametrize("form", ["forward", "gradient"])
def test_conv3x3s2_halo_bounded_and_guarded(lib, N, Kc, Nout, IH, IW, form):
    """rbvae_conv3x3s2_halo, both workgroup widths, padded lda / ldo, tiles hanging over the last rows / columns: the
    forward form (bias, ReLU, scale) and the gradient form (gate, scale, per-tile column sums of the stored values, the
    workspace sized by rbvae_conv3x3s2_halo_colsum_rows)."""
    assert lib.query("rbvae_conv3x3s2_halo_ok", 1, N, IH, IW, Kc, Nout)
    OH, OW = IH // 2, IW // 2
    lda, ldo = Kc + 32, Nout + 8
    g = torch.Generator().manual_seed(N * IH * IW + Kc)
    x = torch.randn(N, Kc, IH, IW, generator=g).bfloat16()
    w = (torch.randn(Nout, Kc, 3, 3, generator=g) / (9 * Kc) ** 0.5).bfloat16()
    ref, S = B.ref_and_scale("conv2d", x, w, stride=2)
    ref, S = B.rows(ref), B.rows(S)
    A = B.poisoned(B.rows(x), lda, torch.bfloat16)
    Wp = B.poisoned(w.permute(0, 2, 3, 1).reshape(Nout, -1), 9 * Kc, torch.bfloat16)
    out = B.guarded(N * OH * OW, ldo, Nout, torch.bfloat16)
    bias = gate = ws = None
    if form == "forward":
        bias, relu, scale = torch.randn(Nout, generator=g) * 0.5, 1, 1.25
        ref, S = (ref + bias.double()).clamp_min(0) * scale, S + bias.double().abs()
    else:
        relu, scale = 0, 0.5
        gv = torch.randn(N * OH * OW, Nout, generator=g).bfloat16()
        gate = B.poisoned(gv, ldo, torch.bfloat16)
        ref = ref * scale * (gv > 0)
        ws = B.guarded(lib.query("rbvae_conv3x3s2_halo_colsum_rows", N, IH, IW), Nout, Nout, torch.float32)
    lib.call("rbvae_conv3x3s2_halo", 1, A.view, Wp.view, out.view, bias.cuda() if bias is not None else None,
             gate and gate.view, None, N, IH, IW, Kc, Nout, lda, ldo, relu, 0, 0.0, scale, 0, None, ws and ws.view)
    torch.cuda.synchronize()
    B.assert_guards(out, "conv3x3s2_halo Out")
    worst = B.check(out.out, ref, S, out_dtype=torch.bfloat16, K=9 * Kc, scale=scale, nhw=(N, OH, OW),
                    what=f"conv3x3s2_halo {form} {N}x{Kc}x{Nout}x{IH}x{IW}")
    report("conv3x3s2_halo", form, "bf16", worst)
    if ws is not None:
        # per 8 x 16 output-pixel tile (image-major, then tile row, then tile column): the f64 sum of its stored rows
        B.assert_guards(ws, "conv3x3s2_halo colsum_ws")
        p = torch.arange(N * OH * OW)
        n, r, c = p // (OH * OW), p // OW % OH, p % OW
        tile = (n * C.cdiv(OH, 8) + r // 8) * C.cdiv(OW, 16) + c // 16
        stored = out.out.double().cpu()
        want = torch.zeros(ws.rows, Nout, dtype=torch.float64).index_add_(0, tile, stored)
        absw = torch.zeros_like(want).index_add_(0, tile, stored.abs())
        assert bool(((ws.out.double().cpu() - want).abs() <= 127 * 2.0 ** -24 * absw + B.TINY).all())
