"""The halo-kernel cases of test_halo_bounds_gpu.py: case tables, the host restatement of each kernel's dispatch (which
template instance a case reaches, how its tiles and K-slices are laid out), and the float64 operands and references
(CPU only: the GPU tests upload what is built here, test_halo_bounds_cpu.py checks the tables without a GPU).

  conv_halo.hip / conv_halo_ws.hip   rbvae_conv3x3_halo: 16 x 16 pixel x 128 channel tiles, GroupNorm staging,
                                     (mean, M2) statistics per tile and group, rbvae_gn_finish_tiles
  deconv_halo.hip                    rbvae_deconv3x3s2_halo: strip-linear tiles, four parity classes, column sums
  wgrad_halo.hip / wgrad_row.hip     rbvae_wgrad3x3s2_halo / _row: per-K-slice weight-gradient slabs"""
import torch

import _bounds as B
from _conv_cases import DTYPE_ID, KE, TDT, cdiv

# ---- rbvae_conv3x3_halo ---------------------------------------------------------------------------------------------

CH_T, CH_BN, CW_MAXN = 16, 128, 512


def ch_geometry(c):
    """(OH, OW, tiles_r, tiles_c, mtiles, total work items) of a conv case."""
    (ph, pw), N = c["pad"], c["N"]
    OH, OW = c["IH"] + 2 * ph - 2, c["IW"] + 2 * pw - 2
    tr, tc = cdiv(OH, CH_T), cdiv(OW, CH_T)
    return OH, OW, tr, tc, N * tr * tc, N * tr * tc * (c["Nout"] // CH_BN)


def ch_ws_covers(c):
    """ch_ws_covers (csrc/conv_halo_ws.hip): 32-bit buffer offsets, Nout <= 512, statistics groups within 64 lanes."""
    OH, OW = ch_geometry(c)[:2]
    lim, N, Kc, cg = 1 << 31, c["N"], c["Kc"], c["stats_cg"]
    return (N * c["IH"] * c["IW"] * c["lda"] * 2 < lim and c["Nout"] * 9 * Kc * 2 < lim and N * Kc * 4 < lim and
            N * OH * OW * c["ldo"] * 2 < lim and Kc % 64 == 0 and c["Nout"] <= CW_MAXN and
            (not cg or (cg <= 64 and 64 % cg == 0)))


def ch_kernel(c, variant):
    """The kernel rbvae_conv3x3_halo launches (conv_halo.hip:628-634) under rbvae_dbg_conv_halo_variant(variant):
    f32 always conv_halo_k<float, 3, GN>; bf16 the persistent conv_halo_ws_k<GN> for variant 0, or variant 2 with
    >= 512 work items, wherever ch_ws_covers, else conv_halo_k<bf16, 3, GN>."""
    if c["dtype"] == "f32":
        return "conv_halo_k"
    total = ch_geometry(c)[5]
    if (variant == 0 or (variant == 2 and total >= 512)) and ch_ws_covers(c):
        return "conv_halo_ws_k"
    return "conv_halo_k"


def ch_variants(c):
    """The dbg variants a case runs under: 1 (one tile per workgroup) always, 0 (persistent) for bf16 where covered."""
    return [1, 0] if c["dtype"] == "bf16" and ch_ws_covers(c) else [1]


def ch(id, dtype, N, IH, IW, Kc, Nout, pad=(1, 1), lda=0, ldo=0, bias=0, addend=0, gn=0, swish=0, stats_cg=0):
    return dict(id=id, dtype=dtype, N=N, IH=IH, IW=IW, Kc=Kc, Nout=Nout, pad=pad, lda=Kc + lda, ldo=Nout + ldo, bias=bias,
                addend=addend, gn=gn, swish=swish, stats_cg=stats_cg)


CH_CASES = [
    # f32: Kc % 32, 1 / 2 / 4 / 8 slices
    ch("f32_s1_n128_stats16", "f32", 2, 16, 16, 32, 128, lda=32, ldo=8, bias=1, stats_cg=16),
    ch("f32_s2_n256_ragged_add", "f32", 1, 17, 33, 64, 256, ldo=4, bias=1, addend=1),
    ch("f32_s4_gn_swish_stats32", "f32", 3, 22, 40, 128, 128, lda=4, bias=1, gn=1, swish=1, stats_cg=32),
    ch("f32_s8_min_pad00_gn", "f32", 2, 10, 18, 256, 128, pad=(0, 0), addend=1, gn=1),
    ch("f32_s1_n512_pad22_gn_swish", "f32", 2, 12, 20, 32, 512, pad=(2, 2), ldo=4, bias=1, addend=1, gn=1, swish=1),
    ch("f32_s2_pad10_gn_stats64", "f32", 1, 19, 21, 64, 256, pad=(1, 0), gn=1, stats_cg=64),
    ch("f32_s1_pad01_stats128", "f32", 2, 10, 16, 32, 128, pad=(0, 1), bias=1, stats_cg=128),
    # bf16: Kc % 64, 1 / 2 / 4 / 8 slices
    ch("bf16_s1_n128_stats16", "bf16", 2, 16, 16, 64, 128, lda=64, ldo=8, bias=1, stats_cg=16),
    ch("bf16_s2_n256_gn_swish_stats32", "bf16", 3, 22, 40, 128, 256, ldo=8, bias=1, addend=1, gn=1, swish=1, stats_cg=32),
    ch("bf16_s8_n512_gn_stats64", "bf16", 1, 16, 24, 512, 512, bias=1, gn=1, stats_cg=64),
    ch("bf16_s4_ragged_add", "bf16", 2, 17, 33, 256, 128, lda=8, addend=1),
    ch("bf16_s2_min_pad00_gn_swish", "bf16", 2, 10, 18, 128, 256, pad=(0, 0), addend=1, gn=1, swish=1),
    ch("bf16_s1_pad22_gn", "bf16", 2, 12, 20, 64, 128, pad=(2, 2), ldo=8, bias=1, gn=1),
    ch("bf16_s4_pad10_stats64", "bf16", 1, 19, 21, 256, 256, pad=(1, 0), bias=1, stats_cg=64),
    ch("bf16_s1_pad01_gn_swish_stats16", "bf16", 2, 10, 17, 64, 128, pad=(0, 1), lda=64, addend=1, gn=1, swish=1,
       stats_cg=16),
    ch("bf16_s2_gn_swish_stats128", "bf16", 2, 20, 20, 128, 256, bias=1, gn=1, swish=1, stats_cg=128),
]

# >= 512 work items: the default dispatch (variant 2) takes conv_halo_ws_k; compared bit for bit with variant 0
CH_BIG = ch("bf16_big_512_items", "bf16", 8, 128, 128, 64, 128, ldo=8, bias=1, addend=1, gn=1, swish=1, stats_cg=32)


def ch_build(c, reference=True):
    """Operands (storage-rounded, CPU) and the float64 reference of a conv case: x [N][Kc][IH][IW], A rows, Wp
    [Nout][9 Kc], bias, addend rows, gn scale / shift [N][Kc]; ref / S / S_in / pre as [N OH OW][Nout] rows, u_in
    (reference=False: the operands alone)."""
    tdt, N, Kc, Nout = TDT[c["dtype"]], c["N"], c["Kc"], c["Nout"]
    OH, OW = ch_geometry(c)[:2]
    g = torch.Generator().manual_seed(sum(map(ord, c["id"])))
    x = torch.randn(N, Kc, c["IH"], c["IW"], generator=g).to(tdt)
    w = (torch.randn(Nout, Kc, 3, 3, generator=g) / (9 * Kc) ** 0.5).to(tdt)
    out = dict(x=x, A=B.rows(x), Wp=w.permute(0, 2, 3, 1).reshape(Nout, 9 * Kc).contiguous(), w=w, nhw=(N, OH, OW),
               bias=None, addend=None, scale=None, shift=None, pre=None, S_in=None, u_in=0.0, K=9 * Kc)
    a = x.double()
    if c["gn"]:
        # different per image and channel: a swapped image or channel group shows up
        out["scale"] = torch.rand(N, Kc, generator=g) + 0.5
        out["shift"] = torch.randn(N, Kc, generator=g) * 0.75
        a, tmax = B.staged_operand(x, out["scale"], out["shift"], c["swish"])
        out["u_in"] = B.staged_u_in(tdt, c["swish"], tmax)
    if reference:
        ref, S = B.ref_and_scale("conv2d", a, w, stride=1, padding=c["pad"])
        assert ref.shape == (N, Nout, OH, OW)
        ref, S = B.rows(ref), B.rows(S)
    else:
        ref = S = torch.zeros(N * OH * OW, Nout, dtype=torch.float64)
    if c["gn"]:
        out["S_in"] = S.clone()
    if c["bias"]:
        out["bias"] = torch.randn(Nout, generator=g) * 0.5
        ref, S = ref + out["bias"].double(), S + out["bias"].double().abs()
    if c["addend"]:
        # added to the tile already rounded to the storage type (conv_halo.hip store phase): a second rounding
        out["addend"] = torch.randn(N * OH * OW, Nout, generator=g).to(tdt)
        out["pre"] = ref
        ref = ref + out["addend"].double()
    out["ref"], out["S"] = ref, S
    return out


def ch_tile_of_rows(c):
    """Statistics tile (mtile = (n tiles_r + tr) tiles_c + tc) of every output row."""
    OH, OW, tr, tc = ch_geometry(c)[:4]
    p = torch.arange(c["N"] * OH * OW)
    n, y, x = p // (OH * OW), p // OW % OH, p % OW
    return (n * tr + y // CH_T) * tc + x // CH_T


def stats_slot(mtile, group, Nout, cg):
    """float2 index of (tile, group) in stats_part: mtile * (Nout / cg) + group (conv_halo.hip epilogue)."""
    return mtile * (Nout // cg) + group


def tile_stats_ref(stored, tile, ntiles, cg):
    """float64 (mean, M2), count, sum |x| and max |x| per (tile, group) of the stored rows [rows][Nout] over each tile's
    valid pixels: [ntiles][Nout / cg] each, in stats_slot order."""
    v = stored.double()
    rows, Nout = v.shape
    G = Nout // cg
    npix = torch.zeros(ntiles, dtype=torch.float64).index_add_(0, tile, torch.ones(rows, dtype=torch.float64))
    s = torch.zeros(ntiles, Nout, dtype=torch.float64).index_add_(0, tile, v).reshape(ntiles, G, cg).sum(-1)
    cnt = npix[:, None] * cg
    mean = s / cnt
    dev = v - mean[tile].repeat_interleave(cg, dim=1)
    m2 = torch.zeros(ntiles, Nout, dtype=torch.float64).index_add_(0, tile, dev * dev).reshape(ntiles, G, cg).sum(-1)
    sabs = torch.zeros(ntiles, Nout, dtype=torch.float64).index_add_(0, tile, v.abs()).reshape(ntiles, G, cg).sum(-1)
    amax = torch.zeros(ntiles, Nout, dtype=torch.float64).scatter_reduce_(0, tile[:, None].expand(rows, Nout), v.abs(),
                                                                           "amax")
    amax = amax.reshape(ntiles, G, cg).amax(-1)
    return mean, m2, cnt.expand_as(mean), sabs, amax


def check_tile_stats(got, stored, tile, ntiles, cg, what=""):
    """got [ntiles * G][2] (the kernel's float2 (mean, M2)) against tile_stats_ref of the stored rows under
    _bounds.tile_stats_bounds.  Returns (worst mean ratio, worst M2 ratio)."""
    mean, m2, cnt, sabs, amax = tile_stats_ref(stored, tile, ntiles, cg)
    got = got.detach().cpu().double().reshape(mean.shape + (2,))
    bm, bM2, _ = B.tile_stats_bounds(cnt, cg, sabs, amax, m2)
    out = []
    for k, (ref, bnd) in enumerate(((mean, bm), (m2, bM2))):
        err = (got[..., k] - ref).abs()
        ratio = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err / bnd)
        if not bool((err <= bnd).all()):
            t, gi = divmod(int(torch.argmax(ratio.reshape(-1))), mean.shape[1])
            raise AssertionError(f"{what}: tile statistics {('mean', 'M2')[k]} outside the bound at (tile {t}, group "
                                 f"{gi}): got {float(got[t, gi, k])!r}, ref {float(ref[t, gi])!r}, bound "
                                 f"{float(bnd[t, gi]):.3g}, worst |err|/bound {float(ratio.max()):.3g}")
        out.append(float(ratio.max()) if ratio.numel() else 0.0)
    return tuple(out)


def gn_finish_ref(stored, tile, c, cg, eps):
    """float64 per-(image, group) mean and variance of the stored output, and the bounds of rbvae_gn_finish_tiles'
    mean_out / rstd_out (csrc/conv_halo.hip gn_finish_tiles_k): count-weighted tile means summed over a block of 256
    threads (per-thread strided sums, wave_sum, four wave partials), the tile bounds carried through, rsqrtf 1 ulp."""
    N, (OH, OW, tr, tc, mtiles) = c["N"], ch_geometry(c)[:5]
    return gn_finish_bounds(stored, tile, N, OH * OW, tr * tc, cg, eps)


def gn_finish_bounds(stored, tile, N, HW, nb, cg, eps):
    """gn_finish_ref for any tiling: HW pixels per image in nb tiles each (tile: the statistics tile of every stored row)."""
    mtiles = N * nb
    v = stored.double().reshape(N, HW, -1)
    Nout = v.shape[-1]
    G, total = Nout // cg, HW * cg
    grp = v.reshape(N, HW, G, cg).permute(0, 2, 1, 3).reshape(N, G, -1)
    mean = grp.mean(-1)
    var = ((grp - mean[..., None]) ** 2).sum(-1) / total
    amax = grp.abs().amax(-1)
    tmean, tm2, tcnt, tsabs, tamax = tile_stats_ref(stored, tile, mtiles, cg)
    _, bM2_t, E_t = B.tile_stats_bounds(tcnt, cg, tsabs, tamax, tm2)
    hf = cdiv(nb, 256) + 6 + 3 + 2
    E_f = E_t.reshape(N, nb, G).amax(1) + hf * B.U32 * amax
    Q = var * total
    bq = bM2_t.reshape(N, nb, G).sum(1) + (hf + 3) * B.U32 * Q + 2 * E_f * (total * Q) ** 0.5 + total * E_f ** 2
    b_var = bq / total + B.U32 * var
    veps = var + float(torch.tensor(eps, dtype=torch.float32))
    rstd = veps.rsqrt()
    b_rstd = (0.5 * (b_var / veps + B.U32) + 2 * B.U32) * rstd * 1.01 + B.TINY
    return mean, rstd, E_f + B.TINY, b_rstd


# ---- rbvae_deconv3x3s2_halo -----------------------------------------------------------------------------------------

DH_BN = 64


def dh_strip_cols(TW):
    """deconv_halo.hip dh_strip_cols: strips of 16 / 8 / 4 columns, 0 = not covered."""
    return 16 if TW % 16 == 0 else 8 if TW % 8 == 0 else 4 if TW % 4 == 0 else 0


def dh_max_patch_rows(TH, TR):
    return TR + (TR // TH if TR % TH == 0 else (TR - 1) // TH + 2)


def dh_tile_rows(dtype, N, TH, TW, Kc, Nout):
    """deconv_halo.hip dh_tile_rows (:572-589): 128 (deconv_halo_k<T, SC, 4>), 256 (<T, SC, 8>), 0 not covered."""
    if Kc <= 0 or Kc % KE[dtype] or Nout <= 0 or Nout % DH_BN or TH < 1 or TH > 4095 or N < 1:
        return 0
    sc = dh_strip_cols(TW)
    if not sc or N * (TW // sc) >= (1 << 19):
        return 0
    if dh_max_patch_rows(TH, 128 // sc) <= 176 // (sc + 1):
        return 128
    if dh_max_patch_rows(TH, 256 // sc) <= (320 if sc == 16 else 352 if sc == 8 else 416) // (sc + 1):
        return 256
    return 0


def dh_instance(c):
    """(T, SC, WAVES) of deconv_halo_k a case launches."""
    bm = dh_tile_rows(c["dtype"], c["N"], c["TH"], c["TW"], c["Kc"], c["Nout"])
    return c["dtype"], dh_strip_cols(c["TW"]), 4 if bm == 128 else 8


def dh_colsum_rows(c):
    bm = dh_tile_rows(c["dtype"], c["N"], c["TH"], c["TW"], c["Kc"], c["Nout"])
    sc = dh_strip_cols(c["TW"])
    return 4 * cdiv(c["N"] * (c["TW"] // sc) * c["TH"], bm // sc)


def dh_colsum_row_of_outputs(c):
    """colsum_ws row (4 mtile + class) of every output row: input-grid position (n, a, iw) lies in strip
    s = n * strips + iw // SC, strip-linear row g = s TH + a, tile g // (bm / SC); output (2a + ch, 2iw + cw) is class
    2 ch + cw (deconv_halo.hip tables and epilogue)."""
    N, TH, TW = c["N"], c["TH"], c["TW"]
    bm = dh_tile_rows(c["dtype"], N, TH, TW, c["Kc"], c["Nout"])
    sc = dh_strip_cols(TW)
    OH, OW = 2 * TH, 2 * TW
    p = torch.arange(N * OH * OW)
    n, oy, ox = p // (OH * OW), p // OW % OH, p % OW
    a, iw = oy // 2, ox // 2
    s = n * (TW // sc) + iw // sc
    mtile = (s * TH + a) // (bm // sc)
    return mtile * 4 + (oy % 2) * 2 + ox % 2


# every (T, SC, WAVES) the dispatch reaches (test_halo_bounds_cpu.py derives it from dh_tile_rows over a grid of shapes)
DH_REACHABLE = {(d, sc, wv) for d in ("f32", "bf16") for sc, wv in ((16, 4), (8, 4), (4, 4), (8, 8), (4, 8))}


def dh(id, dtype, N, TH, TW, Kc, Nout, form, lda=0, ldo=0):
    return dict(id=id, dtype=dtype, N=N, TH=TH, TW=TW, Kc=Kc, Nout=Nout, form=form, lda=Kc + lda, ldo=Nout + ldo)


DH_CASES = [
    dh("f32_sc16_w4_fwd", "f32", 2, 8, 16, 32, 64, "forward", lda=32, ldo=4),
    dh("f32_sc8_w4_grad", "f32", 5, 8, 8, 64, 128, "gradient", ldo=8),
    dh("f32_sc4_w4_fwd_ragged", "f32", 1, 17, 20, 96, 64, "forward"),
    dh("f32_sc8_w8_grad", "f32", 3, 6, 24, 32, 192, "gradient", lda=4),
    dh("f32_sc4_w8_fwd_4x4", "f32", 9, 4, 4, 64, 64, "forward", ldo=8),
    dh("bf16_sc16_w4_grad", "bf16", 3, 22, 32, 128, 128, "gradient", ldo=8),
    dh("bf16_sc16_w4_fwd", "bf16", 1, 16, 16, 64, 256, "forward", lda=64),
    dh("bf16_sc8_w4_fwd_8x8", "bf16", 6, 8, 8, 256, 128, "forward", ldo=8),
    dh("bf16_sc4_w4_grad", "bf16", 2, 16, 12, 64, 64, "gradient", lda=8),
    dh("bf16_sc8_w8_grad", "bf16", 2, 6, 40, 128, 64, "gradient"),
    dh("bf16_sc4_w8_fwd_4x4", "bf16", 13, 4, 4, 256, 256, "forward", lda=8, ldo=8),
    dh("bf16_sc4_w8_grad_11x20", "bf16", 2, 11, 20, 192, 128, "gradient", ldo=8),
]


def dh_build(c):
    """Operands and the float64 reference: A rows [N TH TW][Kc], Wp [Nout][9 Kc] (ConvTranspose2d weight [ci][co][kh][kw]
    packed [co][kh kw][ci]); forward: bias, ReLU, scale 1.25, explicit keep-mask; gradient: gate, scale 0.5."""
    tdt, N, TH, TW, Kc, Nout = TDT[c["dtype"]], c["N"], c["TH"], c["TW"], c["Kc"], c["Nout"]
    g = torch.Generator().manual_seed(sum(map(ord, c["id"])))
    x = torch.randn(N, Kc, TH, TW, generator=g).to(tdt)
    w = (torch.randn(Kc, Nout, 3, 3, generator=g) / (4 * Kc) ** 0.5).to(tdt)
    ref, S = B.ref_and_scale("conv_transpose2d", x, w)
    ref, S = B.rows(ref), B.rows(S)
    rows = N * 4 * TH * TW
    out = dict(A=B.rows(x), Wp=w.permute(1, 2, 3, 0).reshape(Nout, 9 * Kc).contiguous(), x=x, w=w, rows=rows,
               nhw=(N, 2 * TH, 2 * TW), bias=None, gate=None, keep=None, K=4 * Kc)
    if c["form"] == "forward":
        out["bias"] = torch.randn(Nout, generator=g) * 0.5
        out["relu"], out["scale"] = 1, 1.25
        ref, S = (ref + out["bias"].double()).clamp_min(0) * 1.25, S + out["bias"].double().abs()
        out["keep"] = torch.rand(rows, Nout, generator=g) > 0.2
        ref = ref * out["keep"]
    else:
        out["relu"], out["scale"] = 0, 0.5
        out["gate"] = torch.randn(rows, Nout, generator=g).to(tdt)
        ref = ref * 0.5 * (out["gate"] > 0)
    out["ref"], out["S"] = ref, S
    return out


def dh_colsum_ref(c, stored):
    """float64 column sums of the kernel's stored rows per colsum_ws row, with the bound of the f32 sums: <= bm
    terms per row (per-thread runs, then the row lanes in order): (bm - 1) u sum |v|."""
    row = dh_colsum_row_of_outputs(c)
    nrow = dh_colsum_rows(c)
    v = stored.double()
    want = torch.zeros(nrow, v.shape[1], dtype=torch.float64).index_add_(0, row, v)
    absw = torch.zeros_like(want).index_add_(0, row, v.abs())
    bm = dh_tile_rows(c["dtype"], c["N"], c["TH"], c["TW"], c["Kc"], c["Nout"])
    return want, (bm - 1) * B.U32 * absw + B.TINY


# ---- rbvae_wgrad3x3s2_halo / rbvae_wgrad3x3s2_row ----------------------------------------------------------------------

WH_BH, WH_BW = 4, 8


def wh_blocks(N, OH, OW):
    return N * cdiv(OH, WH_BH) * cdiv(OW, WH_BW)


def wh_slices(N, OH, OW, ks):
    """Pixel blocks [blk0, blk1) of every K-slice of wgrad_halo_k: per = ceil(nblk / ksplit), slice k takes blocks
    k per .. min((k + 1) per, nblk) (empty when k per >= nblk)."""
    nblk = wh_blocks(N, OH, OW)
    per = cdiv(nblk, ks)
    return [(min(k * per, nblk), min(k * per + per, nblk)) for k in range(ks)]


def wh_block_pixels(N, OH, OW, blk):
    """Low-resolution pixel rows (n OH + r) OW + c of block blk: a 4 x 8 block clipped to the image."""
    BR, BC = cdiv(OH, WH_BH), cdiv(OW, WH_BW)
    n, rem = divmod(blk, BR * BC)
    r0, c0 = rem // BC * WH_BH, rem % BC * WH_BW
    return [(n * OH + r) * OW + cc for r in range(r0, min(r0 + WH_BH, OH)) for cc in range(c0, min(c0 + WH_BW, OW))]


def wh_grid(Ca, Cb, ks):
    """Workgroups launched: (Ca/64)(Cb/64) tiles x ksplit rounded up to a multiple of 8 (the rest return at once)."""
    return (Ca // 64) * (Cb // 64) * 8 * cdiv(ks, 8)


def wr_width(OW):
    """wgrad_row.hip wr_width: 8-column blocks unless 4-column strips waste fewer columns."""
    return 8 if cdiv(OW, 8) * 8 == cdiv(OW, 4) * 4 else 4


def wr_blocks(N, OH, OW):
    W = wr_width(OW)
    return cdiv(OW, W) * cdiv(N * OH, 64 // W)


def wr_slices(N, OH, OW, ks):
    """Balanced K-slices of wgrad_row_k: the first nblk % ksplit slices take one block more."""
    nblk = wr_blocks(N, OH, OW)
    base, rem = divmod(nblk, ks)
    out = []
    for k in range(ks):
        b0 = k * base + min(k, rem)
        out.append((b0, b0 + base + (1 if k < rem else 0)))
    return out


def wr_block_pixels(N, OH, OW, blk):
    """Pixels of 64-pixel block blk = (row block rb, strip): flattened rows rb RB .. + RB - 1 of all Nimg OH rows (a block
    may span images), columns strip W .. + W - 1, clipped."""
    W = wr_width(OW)
    RB, nstrip = 64 // W, cdiv(OW, W)
    rb, strip = divmod(blk, nstrip)
    return [R * OW + cc for R in range(rb * RB, min(rb * RB + RB, N * OH)) for cc in range(strip * W, min(strip * W + W, OW))]


def wr_grid(Ca, Cb, ks):
    return 8 * cdiv((Ca // 128) * (Cb // 128) * 3 * ks, 8)


def wk(id, kind, N, OH, OW, Ca, Cb, ks, lds=0, ldg=0):
    return dict(id=id, kind=kind, N=N, OH=OH, OW=OW, Ca=Ca, Cb=Cb, ks=ks, lds=Ca + lds, ldg=Cb + ldg)


WK_CASES = [
    # wgrad_halo_k: nblk 10 with ksplit 7 (per 2: slices 5, 6 empty; 56 - 7 padding workgroups), ragged blocks
    wk("halo_10blk_ks7", "halo", 1, 18, 13, 64, 64, 7, lds=8, ldg=8),
    wk("halo_2a_ks1", "halo", 2, 8, 16, 128, 64, 1),
    wk("halo_2b_ks9_empty", "halo", 3, 7, 12, 64, 128, 9, ldg=16),
    wk("halo_2x2_ks8_empty", "halo", 2, 11, 20, 128, 128, 8, lds=8),
    wk("halo_ks3", "halo", 2, 13, 27, 64, 64, 3),
    # wgrad_row_k<8> (OW % 8 in {0, 5, 6, 7}) and <4>: row blocks spanning images, ragged strips
    wk("row8_span_ks3", "row", 3, 5, 13, 128, 128, 3),
    wk("row8_2b_ks2", "row", 1, 12, 24, 128, 256, 2, lds=8, ldg=8),
    wk("row4_span_2a_ks5", "row", 4, 9, 12, 256, 128, 5, ldg=8),
    wk("row4_ks1", "row", 2, 20, 4, 128, 128, 1, lds=16),
]


def wk_slices(c):
    f = wh_slices if c["kind"] == "halo" else wr_slices
    return f(c["N"], c["OH"], c["OW"], c["ks"])


def wk_block_pixels(c, blk):
    f = wh_block_pixels if c["kind"] == "halo" else wr_block_pixels
    return f(c["N"], c["OH"], c["OW"], blk)


def wk_slice_pixels(c, slices=None):
    """Pixel lists of every K-slice (slices: [(blk0, blk1)], default the kernel's)."""
    return [[p for b in range(b0, b1) for p in wk_block_pixels(c, b)] for b0, b1 in (slices or wk_slices(c))]


def wk_build(c):
    """Operands S [N OH OW][Ca], G [N 2OH 2OW][Cb] (bf16) and the unfolded G patches U [P][9 Cb] in float64: the slab
    entry (a, t, b) of a slice is sum over its pixels of S[p][a] U[p][t Cb + b] ([Ca][9][Cb] = wgrad_conv2d's)."""
    N, OH, OW, Ca, Cb = c["N"], c["OH"], c["OW"], c["Ca"], c["Cb"]
    g = torch.Generator().manual_seed(sum(map(ord, c["id"])))
    s = torch.randn(N, Ca, OH, OW, generator=g).bfloat16()
    gi = torch.randn(N, Cb, 2 * OH, 2 * OW, generator=g).bfloat16()
    U = torch.nn.functional.unfold(gi.double(), 3, padding=1, stride=2)           # [N][Cb * 9][OH OW], (cb, kh, kw)
    U = U.reshape(N, Cb, 9, OH * OW).permute(0, 3, 2, 1).reshape(N * OH * OW, 9 * Cb)
    return dict(S=B.rows(s), G=B.rows(gi), s=s, g=gi, U=U, P=N * OH * OW)


def wk_slab_refs(d, pix):
    """(ref, S) [Ca][9 Cb] per pixel list."""
    Sd, U = d["S"].double(), d["U"]
    out = []
    for p in pix:
        idx = torch.tensor(p, dtype=torch.long)
        a, u = Sd[idx], U[idx]
        out.append((a.t() @ u, a.abs().t() @ u.abs()))
    return out


def check_slabs(got, d, c, pix=None, what=""):
    """got [ks][Ca][9 Cb]: every slice against the f64 sum over its own pixels (K = its pixel count); empty slices exactly
    zero.  Returns the worst |err| / bound."""
    pix = pix or wk_slice_pixels(c)
    worst = 0.0
    got = got.detach().cpu().double()
    for k, (p, (ref, S)) in enumerate(zip(pix, wk_slab_refs(d, pix))):
        if not p:
            assert bool((got[k] == 0).all()), f"{what}: empty K-slice {k} is not zero"
            continue
        worst = max(worst, B.check(got[k], ref, S, out_dtype=torch.float32, K=len(p), what=f"{what} K-slice {k}"))
    return worst
