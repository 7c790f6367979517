"""rbvae_wgrad3x3s2_halo (csrc/wgrad_halo.hip) and rbvae_wgrad3x3s2_row (csrc/wgrad_row.hip) element by element against
float64, over the case tables of tests/_wgrad_cases.py (whose geometry restatement says which loop arms each case runs):

  integer operands   the sum of the slabs EQUALS the float64 reference (every f32 partial sum is an exact integer); every slab
                     is integer-valued; the slabs of K-slices without blocks are zero
  random operands    the sum of the slabs inside the f32 accumulation bound of tests/_bounds.py
  both               operands inside NaN guard rows (more than the 2 OW + 1 pixel rows wgrad_row_k's buffer descriptor
                     reaches back in front of G) and NaN columns on both sides of a column slice: a padding pixel read
                     from memory instead of being zeroed reaches a slab as NaN; slabs inside a guard slab on each side
                     (no stray store, every element of every slab written); two launches bit-equal; padded operands
                     bit-equal to contiguous ones; refused calls write nothing."""
import pytest
import torch

import _bounds as B
import _wgrad_cases as W

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


@pytest.fixture(scope="module")
def lib():
    import sfv_amd
    return sfv_amd._lib


def zero_page():
    return torch.zeros(256, dtype=torch.uint8, device="cuda")


def report(kind, c, dtype, worst):
    print(f"\nBOUNDS {kind} {c} {dtype} worst |err|/bound = {worst:.3g}")


def operand(t, ld, col_off, guard_rows):
    """Pixel rows t [rows][C] as a column slice starting col_off elements into sentinel rows of ld elements, inside
    sentinel guard rows: (buffer, the [rows][ld - col_off] view whose address the kernel gets)."""
    if col_off == 0:
        g = B.poisoned(t, ld, BF, guard_rows=guard_rows)
        return g, g.view
    g = B.guarded(t.shape[0], ld, ld, BF, guard_rows=guard_rows)
    g.view[:, col_off:col_off + t.shape[1]].copy_(t)
    v = g.view[:, col_off:]
    assert v.data_ptr() % 16 == 0 and bool(torch.isnan(g.view[:, :col_off]).all())
    assert bool(torch.isnan(g.view[:, col_off + t.shape[1]:]).all())
    return g, v


def buffers(c, d, padded=True, ks=None):
    """(S, G, lds, ldg, slabs) of a case: freshly poisoned operands (the views whose addresses the kernel gets) and freshly
    guarded slabs; padded = False: contiguous operands."""
    Ca, Cb, OW = c["Ca"], c["Cb"], c["OW"]
    lds, ldg, offs, offg = (c["lds"], c["ldg"], c["col_off_s"], c["col_off_g"]) if padded else (Ca, Cb, 0, 0)
    guard_g = 2 * (2 * OW) + 2
    _, S = operand(d["S"], lds, offs, B.GUARD_ROWS)
    Gg, G = operand(d["G"], ldg, offg, guard_g)
    assert Gg.g >= guard_g > 2 * OW + 1
    ks = c["ks"] if ks is None else ks
    slabs = B.guarded(ks * Ca * 9, Cb, Cb, torch.float32, guard_rows=Ca * 9)        # a whole guard slab on each side
    return S, G, lds, ldg, slabs


def call(lib, kind, c, S, G, lds, ldg, slabs, ks):
    lib.call(f"rbvae_wgrad3x3s2_{kind}", 1, S, G, slabs.view, zero_page(), c["N"], c["OH"], c["OW"], c["Ca"], c["Cb"],
             lds, ldg, ks)
    torch.cuda.synchronize()


def launch(lib, kind, c, d, padded=True):
    S, G, lds, ldg, slabs = buffers(c, d, padded)
    call(lib, kind, c, S, G, lds, ldg, slabs, c["ks"])
    return slabs


@pytest.mark.parametrize("kind,c", W.ALL_CASES, ids=[c["id"] for _, c in W.ALL_CASES])
def test_wgrad3x3s2_exact_bounded_and_guarded(lib, kind, c):
    N, OH, OW, Ca, Cb, ks = c["N"], c["OH"], c["OW"], c["Ca"], c["Cb"], c["ks"]
    name = f"rbvae_wgrad3x3s2_{kind}"
    assert lib.query(name + "_ok", 1, N, OH, OW, Ca, Cb)
    nblk = lib.query(name + "_blocks", N, OH, OW)
    assert nblk == W.blocks(kind, c) and 1 <= ks <= nblk
    d = W.build(kind, c)
    kern = "wgrad_halo_k" if kind == "halo" else f"wgrad_row_k<{W.wr_geometry(c)['W']}>"
    what = f"{c['id']} {kern}"
    slabs = launch(lib, kind, c, d)
    B.assert_guards(slabs, f"{what} slabs")
    each = slabs.out.double().cpu().reshape(ks, Ca, 9, Cb)
    got = each.sum(0)
    if c["data"] == "int":
        W.assert_equal_int(got, d["ref"], what)
        assert bool(torch.isfinite(each).all()) and bool((each == each.round()).all()), f"{what}: a slab is not integer-valued"
    else:
        worst = W.check_randn(kind, c, got, d, what)
        report("wgrad3x3s2", what, "bf16", worst)
    for k, n in enumerate(W.steps(kind, c)):
        if n == 0:
            assert bool((each[k] == 0).all()), f"{what}: empty K-slice {k} is not zero"
    # fixed order: a second launch, into its own guarded buffers, gives the same bits
    again = launch(lib, kind, c, d)
    B.assert_guards(again, f"{what} slabs, second launch")
    assert torch.equal(slabs.out.view(torch.int32), again.out.view(torch.int32)), f"{what}: two launches differ"
    if c["col_off_s"] or c["col_off_g"]:
        dense = launch(lib, kind, c, d, padded=False)
        B.assert_guards(dense, f"{what} slabs, contiguous operands")
        assert torch.equal(slabs.out.view(torch.int32), dense.out.view(torch.int32)), \
            f"{what}: padded leading dimensions and column offsets change the slabs"


@pytest.mark.parametrize("kind", W.KINDS)
def test_wgrad3x3s2_refused_calls_write_nothing(lib, kind):
    """ksplit = blocks + 1, a pointer that is not 16-byte aligned and a leading dimension that is no multiple of 8 raise
    and leave an all-sentinel output untouched."""
    c = next(c for c in W.TABLES[kind] if c["col_off_s"] and W.blocks(kind, c) > 1)
    d = W.build(kind, c)
    nblk = W.blocks(kind, c)
    for why in ("ksplit", "pointer", "ld"):
        ks = nblk + 1 if why == "ksplit" else c["ks"]
        S, G, lds, ldg, slabs = buffers(c, d, ks=ks)
        if why == "pointer":
            S = S[:, 4:]                                  # 8 bytes on: the rows stay inside the padded buffer
            assert S.data_ptr() % 16 == 8
        if why == "ld":
            lds += 4
        with pytest.raises(ValueError):
            call(lib, kind, c, S, G, lds, ldg, slabs, ks)
        B.assert_guards_where(slabs, torch.zeros(slabs.rows, slabs.ld, dtype=torch.bool), f"{kind} refused for its {why}")
