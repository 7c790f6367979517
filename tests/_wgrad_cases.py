"""The cases of test_wgrad_bounds_gpu.py for the two stride-2 weight-gradient kernels, rbvae_wgrad3x3s2_halo
(csrc/wgrad_halo.hip) and rbvae_wgrad3x3s2_row (csrc/wgrad_row.hip): case tables, the host restatement of each kernel's
block geometry (which loop arms a case reaches), the float64 operands and references, and a float64 emulation of the sum
written as explicit loops over the kernels' pixel blocks, in which single defects can be planted (CPU only: the GPU tests
upload what is built here, test_wgrad_bounds_cpu.py checks the tables and the checker without a GPU).

Both kernels compute, per K-slice ks (a range of pixel blocks),

    dW[ks][a][3 kh + kw][b] = sum_{p = (n, r, c) in the slice} S[p][a] * G[(n, 2r + kh - 1, 2c + kw - 1)][b]

with S [N OH OW][lds] the low-resolution and G [N 2OH 2OW][ldg] the high-resolution operand (pixel rows, bf16) and pixels
outside the image contributing zero.  role "conv": S = the conv's output gradient, G = its input; role "deconv": S = the
transposed conv's input, G = its output gradient: the same sum, confirmed by the float64 reference of that role.

data "int": integer-valued operands (S in -3..3, G in -4..4), so every product and every partial sum in any order and
any K-slicing is an integer below 2^24, exact in f32: the kernel must EQUAL the reference.  data "randn": S = randn / 8,
G = randn, rounded to bf16, checked under the f32 accumulation model of tests/_bounds.py."""
import functools

import torch

import _bounds as B
from _conv_cases import cdiv
from _halo_cases import WH_BH, WH_BW, wh_blocks, wh_grid, wh_slices, wr_blocks, wr_grid, wr_slices, wr_width

KINDS = ("halo", "row")
CH_UNIT = {"halo": 64, "row": 128}             # channel tile of a workgroup (either direction)


# ---- geometry --------------------------------------------------------------------------------------------------------

def blocks(kind, c):
    return (wh_blocks if kind == "halo" else wr_blocks)(c["N"], c["OH"], c["OW"])


def slices(kind, c):
    """[(blk0, blk1)] of every K-slice (wgrad_halo_k: ceil(nblk / ks) blocks each, trailing slices short or empty;
    wgrad_row_k: balanced, the first nblk % ks slices one block longer)."""
    return (wh_slices if kind == "halo" else wr_slices)(c["N"], c["OH"], c["OW"], c["ks"])


def steps(kind, c):
    """K-loop steps (pixel blocks) of every K-slice."""
    return [b1 - b0 for b0, b1 in slices(kind, c)]


def wh_geometry(c):
    """wgrad_halo_k: 4 x 8 blocks per image (BR x BC), blocks in all, blocks per K-slice, workgroups launched, XCD groups
    (K-slices in groups of 8: slice k runs on XCD k % 8 in group k / 8), whether a block hangs over the bottom / the
    right edge, whether the image is smaller than one block."""
    N, OH, OW, ks = c["N"], c["OH"], c["OW"], c["ks"]
    BR, BC = cdiv(OH, WH_BH), cdiv(OW, WH_BW)
    nblk = N * BR * BC
    return dict(BR=BR, BC=BC, nblk=nblk, per=cdiv(nblk, ks), grid=wh_grid(c["Ca"], c["Cb"], ks), groups=cdiv(ks, 8),
                over_bottom=OH % WH_BH != 0, over_right=OW % WH_BW != 0, sub_block=OH < WH_BH and OW < WH_BW)


def wr_geometry(c):
    """wgrad_row_k<W>: W, RB = 64 / W block rows over the flattened N OH rows, strips of W columns, blocks, the host's
    rbmod = RB % OH, whether some block has `top` set by p_r0 + RB > OH with p_r0 != 0 (an image's first row inside the
    block, not at its head), the most images one block spans, whether the last row block is short, whether the last strip
    overhangs, (K-slice, tile) items and workgroups launched (8 ceil(items / 8): the rest exit at once)."""
    N, OH, OW, ks = c["N"], c["OH"], c["OW"], c["ks"]
    W = wr_width(OW)
    RB, nstrip, rows = 64 // W, cdiv(OW, W), N * OH
    nrb = cdiv(rows, RB)
    nblk = nstrip * nrb
    base, rem = divmod(nblk, ks)
    heads = [(rb * RB) % OH for rb in range(nrb)]
    span = max((min(rb * RB + RB, rows) - 1) // OH - (rb * RB) // OH + 1 for rb in range(nrb))
    items = (c["Ca"] // 128) * (c["Cb"] // 128) * 3 * ks
    return dict(W=W, RB=RB, nstrip=nstrip, rows=rows, nblk=nblk, base=base, rem=rem, rbmod=RB % OH,
                top_inside=any(h != 0 and h + RB > OH for h in heads), span=span, short_last=rows % RB != 0,
                over_right=OW % W != 0, items=items, grid=wr_grid(c["Ca"], c["Cb"], ks))


def k_model(kind, c):
    """K of B.check: the largest number of pixels one slab accumulates, padding included."""
    return 32 * wh_geometry(c)["per"] if kind == "halo" else 64 * (wr_geometry(c)["base"] + 1)


def block_positions(kind, c, blk):
    """Every position of pixel block blk as (n, r, col, inside): the 32 (halo) / 64 (row) positions the kernel stages,
    those hanging over the image (halo), over the last flattened row (row) or over the last column included with
    inside = False (they contribute zero)."""
    N, OH, OW = c["N"], c["OH"], c["OW"]
    if kind == "halo":
        BR, BC = cdiv(OH, WH_BH), cdiv(OW, WH_BW)
        n, rem = divmod(blk, BR * BC)
        r0, c0 = rem // BC * WH_BH, rem % BC * WH_BW
        return [(n, r, cc, r < OH and cc < OW) for r in range(r0, r0 + WH_BH) for cc in range(c0, c0 + WH_BW)]
    W = wr_width(OW)
    RB, nstrip = 64 // W, cdiv(OW, W)
    rb, strip = divmod(blk, nstrip)
    out = []
    for R in range(rb * RB, rb * RB + RB):
        n, r = divmod(R, OH)
        out += [(n, r, cc, R < N * OH and cc < OW) for cc in range(strip * W, strip * W + W)]
    return out


# ---- case tables -----------------------------------------------------------------------------------------------------

# (N, OH, OW, Ca, Cb, ks)
WH_SHAPES = [(1, 1, 1, 64, 64, 1), (1, 4, 8, 64, 64, 1), (2, 3, 5, 64, 128, 2), (1, 16, 8, 64, 64, 1),
             (3, 5, 9, 128, 64, 2), (3, 5, 9, 64, 64, 5), (5, 4, 4, 64, 64, 3), (2, 11, 20, 64, 64, 9),
             (1, 8, 40, 256, 64, 1), (7, 4, 8, 64, 256, 1), (1, 16, 16, 64, 64, 1), (1, 20, 8, 64, 64, 1),
             (1, 12, 24, 64, 64, 1), (4, 9, 7, 128, 128, 11), (3, 8, 24, 256, 256, 17)]
WR_SHAPES = [(1, 1, 5, 128, 128, 1), (1, 8, 8, 128, 128, 1), (3, 3, 7, 128, 256, 2), (2, 5, 13, 256, 128, 3),      # W = 8
             (5, 6, 16, 128, 128, 1), (2, 11, 22, 128, 128, 4), (1, 20, 40, 128, 128, 5), (1, 20, 40, 128, 128, 3),
             (9, 8, 8, 256, 256, 5), (1, 24, 16, 128, 128, 1), (4, 25, 8, 128, 128, 2),        # the last two: 6 and 7, 6 steps
             (1, 1, 1, 128, 128, 1), (16, 1, 4, 128, 128, 1), (7, 2, 3, 128, 256, 1), (5, 4, 4, 128, 128, 2),      # W = 4
             (3, 11, 20, 256, 256, 4), (4, 9, 10, 128, 128, 7), (6, 7, 9, 128, 128, 9), (2, 24, 4, 128, 128, 3),
             (2, 24, 4, 128, 128, 1)]


def _table(kind, shapes):
    """Every shape once with integer and once with random data, so that each geometry class has both; the roles alternate
    (and differ between a shape's two cases); every third case has padded leading dimensions and column offsets."""
    out = []
    for i, (N, OH, OW, Ca, Cb, ks) in enumerate(shapes):
        for j, data in enumerate(("int", "randn")):
            role = ("conv", "deconv")[(i + j) % 2]
            padded = (i + j) % 3 == 0
            # padded: S starts col_off_s columns into a row of lds elements, with sentinels on both sides (G likewise)
            offs, offg = (8, 16) if padded else (0, 0)
            lds, ldg = (Ca + offs + 8, Cb + offg + 24) if padded else (Ca, Cb)
            out.append(dict(id=f"{kind}_{N}x{OH}x{OW}_{Ca}x{Cb}_ks{ks}_{role}_{data}" + ("_ld" if padded else ""),
                            N=N, OH=OH, OW=OW, Ca=Ca, Cb=Cb, ks=ks, lds=lds, ldg=ldg, col_off_s=offs, col_off_g=offg,
                            role=role, data=data))
    return out


WH_CASES = _table("halo", WH_SHAPES)
WR_CASES = _table("row", WR_SHAPES)
TABLES = {"halo": WH_CASES, "row": WR_CASES}
ALL_CASES = [(k, c) for k in KINDS for c in TABLES[k]]


# ---- operands and references -------------------------------------------------------------------------------------------

def tap_layout(dw):
    """dW [Ca][Cb][3][3] of either role -> the kernels' [a][3 kh + kw][b]."""
    return dw.permute(0, 2, 3, 1).reshape(dw.shape[0], 9, dw.shape[1])


def reference(c, s, g):
    """(ref, scale) [Ca][9][Cb] in float64 of the role's own weight gradient (scale: the same sum of |products|)."""
    wshape = (c["Ca"], c["Cb"], 3, 3)
    if c["role"] == "conv":              # s = dy [N][Ca][OH][OW], g = x [N][Cb][2OH][2OW]
        ref, scale = B.ref_and_scale("wgrad_conv2d", s, g, wshape=wshape, stride=2, padding=1)
    else:                                # s = x [N][Ca][OH][OW], g = dy [N][Cb][2OH][2OW]
        ref, scale = B.ref_and_scale("wgrad_conv_transpose2d", g, s, wshape=wshape)
    return tap_layout(ref), tap_layout(scale)


def operands(c):
    """(s [N][Ca][OH][OW], g [N][Cb][2OH][2OW]) in bf16."""
    N, OH, OW, Ca, Cb = c["N"], c["OH"], c["OW"], c["Ca"], c["Cb"]
    gen = torch.Generator().manual_seed(sum(map(ord, c["id"])))
    if c["data"] == "int":
        s = torch.randint(-3, 4, (N, Ca, OH, OW), generator=gen).bfloat16()
        g = torch.randint(-4, 5, (N, Cb, 2 * OH, 2 * OW), generator=gen).bfloat16()
    else:
        s = (torch.randn(N, Ca, OH, OW, generator=gen) / 8).bfloat16()
        g = torch.randn(N, Cb, 2 * OH, 2 * OW, generator=gen).bfloat16()
    return s, g


@functools.lru_cache(maxsize=None)
def _build(kind, cid):
    c = next(c for c in TABLES[kind] if c["id"] == cid)
    s, g = operands(c)
    ref, scale = reference(c, s, g)
    if c["data"] == "int":
        # scale = sum |products| bounds every partial sum of every order: all of them are integers exact in f32
        assert float(scale.max()) < 2 ** 24, c["id"]
        assert bool((ref == ref.round()).all())
    return dict(s=s, g=g, S=B.rows(s).contiguous(), G=B.rows(g).contiguous(), ref=ref, scale=scale)


def build(kind, c):
    """Operands (s, g as images; S, G as pixel rows, bf16) and the float64 (ref, scale) [Ca][9][Cb] of a table case: built
    once and shared, not to be modified."""
    return _build(kind, c["id"])


# ---- the element-wise checks -----------------------------------------------------------------------------------------

def assert_equal_int(got, ref, what=""):
    """got == ref element for element ([Ca][9][Cb], float64); on failure the number of wrong elements per tap and the
    first wrong (a, tap, b)."""
    got = got.detach().cpu().double().reshape(ref.shape)
    bad = ~(got == ref)                                   # NaN counts as wrong
    if bool(bad.any()):
        a, t, b = (int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the exact sum; wrong elements "
                             f"per tap {bad.sum((0, 2)).tolist()}; first at (a {a}, tap {t}, b {b}): got "
                             f"{got[a, t, b].item()!r}, expected {ref[a, t, b].item()!r}")


def check_randn(kind, c, got, d, what=""):
    """B.check of the summed slabs under the f32 accumulation model; returns the worst |err| / bound."""
    Ca, Cb = c["Ca"], c["Cb"]
    return B.check(got.reshape(Ca, 9 * Cb), d["ref"].reshape(Ca, 9 * Cb), d["scale"].reshape(Ca, 9 * Cb),
                   out_dtype=torch.float32, K=k_model(kind, c), what=what or c["id"])


def check_case(kind, c, got, d, what=""):
    """The case's own check of the sum of its slabs got [Ca][9][Cb] (float64); the worst ratio of a randn case."""
    if c["data"] == "int":
        assert_equal_int(got, d["ref"], what or c["id"])
        return 0.0
    return check_randn(kind, c, got, d, what)


# ---- float64 emulation, block by block -------------------------------------------------------------------------------

DEFECTS = ("swap_kw", "drop_pixel", "double_overhang", "prev_image_row", "prev_row_pixel")


def emulate(kind, c, d, defect=None):
    """Slabs [ks][Ca][9][Cb] in float64 by explicit loops over the K-slices' blocks, positions and taps: a second reference
    that shares nothing with torch's convolutions.  defect plants one fault:
      swap_kw          taps kw = 0 and kw = 2 exchanged
      drop_pixel       the last pixel of the first image left out
      double_overhang  the first position hanging over an edge counted as a second copy of its block's last pixel
      prev_image_row   kh = 0 in the first row of an image n > 0 reads the previous image's last row (the row in front of
                       it in memory), not zero
      prev_row_pixel   kw = 0 in column 0 reads the previous row's last pixel (the pixel in front of it in memory)"""
    assert defect is None or defect in DEFECTS
    N, OH, OW, Ca, Cb, ks = c["N"], c["OH"], c["OW"], c["Ca"], c["Cb"], c["ks"]
    IH, IW = 2 * OH, 2 * OW
    Sd = d["S"].double()
    Gz = torch.cat([d["G"].double(), torch.zeros(1, Cb, dtype=torch.float64)])      # row -1: a padding pixel
    slabs = torch.zeros(ks, Ca, 9, Cb, dtype=torch.float64)
    doubled = False
    for k, (b0, b1) in enumerate(slices(kind, c)):
        sidx, gidx = [], [[] for _ in range(9)]

        def add(n, r, col):
            sidx.append((n * OH + r) * OW + col)
            for kh in range(3):
                for kw in range(3):
                    hr, hc = 2 * r + kh - 1, 2 * col + (2 - kw if defect == "swap_kw" else kw) - 1
                    row = (n * IH + hr) * IW + hc
                    ok = hr >= 0 and hc >= 0
                    if defect == "prev_image_row" and hr < 0 and hc >= 0 and n > 0:
                        ok = True
                    if defect == "prev_row_pixel" and hc < 0 and hr >= 0 and row >= 0:
                        ok = True
                    gidx[3 * kh + kw].append(row if ok else -1)

        for blk in range(b0, b1):
            last = None
            for n, r, col, inside in block_positions(kind, c, blk):
                if inside:
                    if not (defect == "drop_pixel" and (n, r, col) == (0, OH - 1, OW - 1)):
                        add(n, r, col)
                    last = (n, r, col)
                elif defect == "double_overhang" and not doubled and last is not None:
                    add(*last)
                    doubled = True
        if sidx:
            a = Sd[torch.tensor(sidx)]
            for t in range(9):
                slabs[k, :, t, :] = a.t() @ Gz[torch.tensor(gidx[t])]
    return slabs
