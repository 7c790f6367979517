"""The 12-wave form of wgrad_gemm_k (waves 0-7 multiply, waves 8-11 issue the LDS-DMA; csrc/wgrad_gemm.hip) against the 8-wave
form, selected through rbvae_dbg_wgrad_gemm_variant (include/rbvae_dbg_variants.h): the same sums in the same order, so
the f32 slabs must be equal bit for bit; the 12-wave slabs are then checked element by element against a float64
reference under the error model of tests/_bounds.py, inside poisoned guard bands.

Shapes: K loops of one step, one pixel more, exactly the ring of three, a little more and many; K split 1 and 3 (with
K-slices that do not divide and K-slices without pixels); whole and partial channel tiles and the 64-column tile; no index
table (one tap) and the nine-tap stride-2 table of 8 x 8 -> 4 x 4 maps with its -1 entries, also with entries beyond
in_rows, which read the zero row."""
import pytest
import torch

import _bounds as B
import _conv_cases as C

pytestmark = pytest.mark.gpu

CHANNELS = [(128, 128), (136, 72), (128, 64)]                 # Co x Ci: whole tiles, partial tiles on both sides, NT = 1
PIXELS = [64, 65, 192, 200, 1000]
IMAGES = [4, 13, 63]                                          # 16 output pixels each: P = 64, 208, 1008


@pytest.fixture(scope="module")
def lib():
    import sfv_amd
    return sfv_amd._lib


def run_variant(lib, variant, Dy, In, idx, P, in_rows, Co, Ci, taps, ks):
    slab = Co * taps
    slabs = B.guarded(ks * slab, Ci, Ci, torch.float32, guard_rows=slab)
    dbg = lib.dbg_lib()
    old = dbg.rbvae_dbg_wgrad_gemm_variant(variant)
    try:
        lib.call("rbvae_wgrad_gemm", 1, Dy.view, In.view, slabs.view, idx, torch.zeros(256, dtype=torch.uint8, device="cuda"),
                 P, in_rows, Co, Ci, Dy.ld, In.ld, taps, ks)
        torch.cuda.synchronize()
    finally:
        dbg.rbvae_dbg_wgrad_gemm_variant(old)
    return slabs


def compare(lib, what, dy, x, idx, in_rows, Co, Ci, taps, ks, ldy=0, ldi=0):
    """dy [P][Co], x [in_rows][Ci] (bf16, CPU); idx [taps][P] int32 on the device or None."""
    P = dy.shape[0]
    inst, grid, blocks = C.wg_instance("bf16", P, Co, Ci, taps, ks)
    assert inst[2] == 3 and blocks <= 256, "outside the one-workgroup-per-CU path the selector covers"
    Dy = B.poisoned(dy, Co + ldy, torch.bfloat16)
    In = B.poisoned(x, Ci + ldi, torch.bfloat16)
    s8 = run_variant(lib, 1, Dy, In, idx, P, in_rows, Co, Ci, taps, ks)
    s12 = run_variant(lib, 2, Dy, In, idx, P, in_rows, Co, Ci, taps, ks)
    B.assert_guards(s8, what + " 8-wave slabs")
    B.assert_guards(s12, what + " 12-wave slabs")
    assert torch.equal(s8.buf.view(torch.int32), s12.buf.view(torch.int32)), what + ": the two forms differ"
    # float64 reference from the table itself: dW[co][t][ci] = sum_p dy[p][co] * x[idx[t][p]][ci], entries outside
    # [0, in_rows) contribute nothing
    if idx is None:
        rows = torch.arange(P)[None, :]
    else:
        rows = idx.cpu().long().reshape(taps, P)
    ok = (rows >= 0) & (rows < in_rows)
    xg = x.double()[rows.clamp(0, in_rows - 1)] * ok[:, :, None]                    # [taps][P][Ci]
    ref = torch.einsum("pc,tpi->cti", dy.double(), xg).reshape(Co, taps * Ci)
    S = torch.einsum("pc,tpi->cti", dy.double().abs(), xg.abs()).reshape(Co, taps * Ci)
    slab = Co * taps
    got = s12.out.double().cpu().reshape(ks, slab, Ci).sum(0).reshape(Co, taps * Ci)
    pper = C.cdiv(C.cdiv(P, ks), 64) * 64
    worst = B.check(got, ref, S, out_dtype=torch.float32, K=min(P, pper), what=what)
    print(f"\nBOUNDS wgrad_gemm 12-wave {what} worst |err|/bound = {worst:.3g}")


@pytest.mark.parametrize("ks", [1, 3])
@pytest.mark.parametrize("Co,Ci", CHANNELS, ids=[f"{a}x{b}" for a, b in CHANNELS])
@pytest.mark.parametrize("P", PIXELS)
def test_roles_one_tap_no_table(lib, P, Co, Ci, ks):
    g = torch.Generator().manual_seed(P * 7 + Co + Ci + ks)
    dy = torch.randn(P, Co, generator=g).bfloat16()
    x = torch.randn(P, Ci, generator=g).bfloat16()
    compare(lib, f"linear P{P} {Co}x{Ci} ks{ks}", dy, x, None, P, Co, Ci, 1, ks, ldy=8 if Co % 128 else 0, ldi=8 if Ci % 64 else 0)


def conv_operands(lib, nimg, Co, Ci):
    g = torch.Generator().manual_seed(nimg * 11 + Co + Ci)
    P, in_rows = nimg * 16, nimg * 64
    dy = torch.randn(P, Co, generator=g).bfloat16()
    x = torch.randn(in_rows, Ci, generator=g).bfloat16()
    idx = torch.empty(9 * P, dtype=torch.int32, device="cuda")
    lib.call("rbvae_conv_gather_index", idx, nimg, 8, 8, 4, 4, 3, 3, 2, 1)
    torch.cuda.synchronize()
    assert bool((idx < 0).any()) and int(idx.max()) < in_rows          # the table holds -1 entries (the padding taps)
    return dy, x, idx, P, in_rows


@pytest.mark.parametrize("ks", [1, 3])
@pytest.mark.parametrize("Co,Ci", CHANNELS, ids=[f"{a}x{b}" for a, b in CHANNELS])
@pytest.mark.parametrize("nimg", IMAGES)
def test_roles_nine_taps_stride2_table(lib, nimg, Co, Ci, ks):
    dy, x, idx, P, in_rows = conv_operands(lib, nimg, Co, Ci)
    compare(lib, f"conv N{nimg} {Co}x{Ci} ks{ks}", dy, x, idx, in_rows, Co, Ci, 9, ks, ldy=8, ldi=8 if Ci % 64 else 0)


@pytest.mark.parametrize("Co,Ci", CHANNELS, ids=[f"{a}x{b}" for a, b in CHANNELS])
def test_roles_table_entries_beyond_in_rows_read_zero_rows(lib, Co, Ci):
    dy, x, idx, P, in_rows = conv_operands(lib, 13, Co, Ci)
    bad = idx.clone()
    pos = torch.tensor([0, 5, P - 1, P + 3, 4 * P + 100, 9 * P - 1], device="cuda")
    bad[pos] = torch.tensor([in_rows, in_rows + 7, 1 << 30, in_rows, -5, in_rows + 1], dtype=torch.int32, device="cuda")
    compare(lib, f"conv table beyond in_rows {Co}x{Ci}", dy, x, bad, in_rows, Co, Ci, 9, 3, ldy=8)
