"""The element-wise checker of tests/_bounds.py is not vacuous: exact results pass, single local defects of a tiled
kernel fail, the bound stays tight, guard bands catch stray and missing stores, and the GPU cases of
test_conv_bounds_gpu.py reach every template instance the build dispatches to (no GPU needed)."""
from importlib import import_module

import pytest
import torch
import torch.nn.functional as F

import _bounds as B
import _conv_cases as C

BF, F32 = torch.bfloat16, torch.float32


def conv_case(Kc, Nout=200, N=2, H=22, W=18, dtype=BF, seed=0):
    """A 3x3 stride-2 conv as NHWC rows: x, w (storage-rounded), ref / S rows [N*Ho*Wo][Nout]; 198 rows: a ragged
    second 128-row tile."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Kc, H, W, generator=g).to(dtype)
    w = (torch.randn(Nout, Kc, 3, 3, generator=g) / (9 * Kc) ** 0.5).to(dtype)
    ref, S = B.ref_and_scale("conv2d", x, w, stride=2)
    return x, w, B.rows(ref), B.rows(S), (N, ref.shape[2], ref.shape[3])


@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("Kc", [64, 256])
def test_exact_conv_passes(dtype, Kc):
    x, w, ref, S, nhw = conv_case(Kc, dtype=dtype)
    B.check(ref.to(dtype), ref, S, out_dtype=dtype, K=9 * Kc, nhw=nhw)
    B.check(ref.to(dtype) * 1.0, ref, S, out_dtype=dtype, K=9 * Kc, scale=1.0)


@pytest.mark.parametrize("dtype", [BF, F32])
def test_exact_transposed_conv_and_wgrads_pass(dtype):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 64, 7, 9, generator=g).to(dtype)
    w = (torch.randn(64, 72, 3, 3, generator=g) / 16).to(dtype)
    ref, S = B.ref_and_scale("conv_transpose2d", x, w)
    assert ref.shape == (2, 72, 14, 18)
    B.check(B.rows(ref).to(dtype), B.rows(ref), B.rows(S), out_dtype=dtype, K=4 * 64)
    xi = torch.randn(2, 64, 14, 18, generator=g).to(dtype)
    dy = torch.randn(2, 72, 7, 9, generator=g).to(dtype)
    ref, S = B.ref_and_scale("wgrad_conv2d", dy, xi, wshape=(72, 64, 3, 3), stride=2)
    B.check(ref.float().reshape(72, -1), ref.reshape(72, -1), S.reshape(72, -1), out_dtype=F32, K=2 * 63)
    ref, S = B.ref_and_scale("wgrad_linear", B.rows(dy), B.rows(x))
    B.check(ref.float(), ref, S, out_dtype=F32, K=2 * 63)


def test_weight_gradient_references_are_autograd():
    """The wgrad references of _bounds are the weight gradients torch's autograd computes (f64)."""
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 8, 10, 12, generator=g, dtype=torch.float64)
    w = torch.randn(16, 8, 3, 3, generator=g, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w, None, stride=2, padding=1)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    torch.testing.assert_close(B.ref_and_scale("wgrad_conv2d", dy, x, wshape=w.shape, stride=2)[0], w.grad)
    wt = torch.randn(8, 16, 3, 3, generator=g, dtype=torch.float64, requires_grad=True)     # ConvTranspose2d(8 -> 16)
    xt = torch.randn(2, 8, 5, 6, generator=g, dtype=torch.float64)
    yt = F.conv_transpose2d(xt, wt, None, stride=2, padding=1, output_padding=1)
    dyt = torch.randn(yt.shape, generator=g, dtype=torch.float64)
    yt.backward(dyt)
    torch.testing.assert_close(B.ref_and_scale("wgrad_conv_transpose2d", dyt, xt, wshape=wt.shape)[0], wt.grad)


# ---- single defects ------------------------------------------------------------------------------------------------

def _rejects(got, ref, S, nhw, K=576):
    with pytest.raises(AssertionError, match="outside the bound"):
        B.check(got, ref, S, out_dtype=BF, K=K, nhw=nhw)


def test_one_element_three_ulps_off_is_caught():
    x, w, ref, S, nhw = conv_case(64)
    got = ref.to(BF)
    i = int(ref.abs().argmax())
    got.view(torch.int16).view(-1)[i] += 3
    _rejects(got, ref, S, nhw)


def test_swapped_adjacent_rows_are_caught():
    x, w, ref, S, nhw = conv_case(64)
    got = ref.to(BF)
    got[[40, 41]] = got[[41, 40]]
    _rejects(got, ref, S, nhw)


def test_zeroed_last_row_of_a_ragged_tile_is_caught():
    x, w, ref, S, nhw = conv_case(64)
    assert ref.shape[0] % 128 != 0
    got = ref.to(BF)
    got[-1] = 0
    _rejects(got, ref, S, nhw)


def test_channel_past_the_tile_boundary_taking_its_neighbour_is_caught():
    x, w, ref, S, nhw = conv_case(64)
    got = ref.to(BF)
    got[:, 128] = got[:, 127]
    _rejects(got, ref, S, nhw)


def test_tap_off_by_one_at_the_bottom_edge_is_caught():
    """Tap kh = 2 read one row lower (dh + 1) on the last output row: that row lies outside the image (even H), so its
    contribution is lost there and nowhere else."""
    x, w, ref, S, nhw = conv_case(64)
    wk = torch.zeros_like(w)
    wk[:, :, 2] = w[:, :, 2]
    part = F.conv2d(x.double(), wk.double(), None, stride=2, padding=1)
    part[:, :, :-1] = 0
    got = (ref - B.rows(part)).to(BF)
    _rejects(got, ref, S, nhw)


def test_failure_report_maps_the_worst_element_to_its_pixel():
    x, w, ref, S, nhw = conv_case(64)
    got = ref.to(BF)
    r = 1 * nhw[1] * nhw[2] + 3 * nhw[2] + 4                                     # image 1, y 3, x 4
    got[r, 130] = got[r, 130] * 2 + 1
    with pytest.raises(AssertionError, match=r"image 1, y 3, x 4, c 130"):
        B.check(got, ref, S, out_dtype=BF, K=576, nhw=nhw)


def test_nan_fails():
    x, w, ref, S, nhw = conv_case(64)
    got = ref.to(BF)
    got[5, 5] = float("nan")
    _rejects(got, ref, S, nhw)


# ---- the bound stays tight -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,limit", [(BF, 2.0 ** -7), (F32, 1e-5)])
def test_bound_is_tight(dtype, limit):
    x, w, ref, S, nhw = conv_case(64, dtype=dtype)
    bnd = B.bound(ref, S, out_dtype=dtype, K=576)
    med = float((bnd / ref.abs()).median())
    assert med < limit, med


# ---- guards ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [BF, F32])
def test_guards_catch_stray_and_missing_stores(dtype):
    def fresh():
        g = B.guarded(200, 80, 72, dtype, device="cpu")
        g.fill(torch.randn(200, 72))
        return g
    g = fresh()
    B.assert_guards(g)                                        # all written, nothing else
    assert g.view.data_ptr() % 16 == 0 and g.g >= 128
    g = fresh()
    g.buf.view(torch.uint8)[3, 5] ^= 1                        # one byte of the leading guard band
    with pytest.raises(AssertionError, match="outside the output"):
        B.assert_guards(g)
    g = fresh()
    g.buf.view(torch.uint8)[-1, -1] ^= 0x40                   # the last byte of the trailing band
    with pytest.raises(AssertionError, match="outside the output"):
        B.assert_guards(g)
    g = fresh()
    g.view[199, 75] = 0                                       # a store into Nout..ldo
    with pytest.raises(AssertionError, match="outside the output"):
        B.assert_guards(g)
    g = fresh()
    ib, pat = B.SENTINEL[dtype]
    g.out.view(ib)[57, 3] = pat                               # one declared element never written
    with pytest.raises(AssertionError, match="never written"):
        B.assert_guards(g)


def test_poisoned_operand_is_nan_outside_its_data():
    t = torch.randn(10, 64).to(BF)
    p = B.poisoned(t, 72, BF, device="cpu")
    assert torch.equal(p.out, t)
    assert bool(torch.isnan(p.view[:, 64:].float()).all()) and bool(torch.isnan(p.buf[:p.g].float()).all())
    assert bool(torch.isnan(p.buf[p.g + 10:].float()).all())


# ---- the GPU cases cover the dispatch table --------------------------------------------------------------------------

def test_descriptors_are_the_engines():
    E = import_module("symbols-from-video_amd.engine")
    assert C.conv_classes(3) == (E.conv_classes(3), 1)
    assert tuple(C.dgrad_classes(3)) == tuple(E.dgrad_classes(3))


def test_every_gather_gemm_branch_has_a_gpu_case():
    reached = set()
    for c in C.GG_CASES:
        branch, inst = C.gg_case_instance(c)
        assert branch == c["inst"], (c["id"], branch)
        reached.add((c["dtype"], branch))
    assert C.GG_REACHABLE <= reached, sorted(C.GG_REACHABLE - reached)
    # the shapes and options each instance is asked to cope with
    assert {c["op"] for c in C.GG_CASES} == {"linear", "conv_s2", "conv_s1", "dgrad"}
    for key in ("bias", "relu", "gate", "addend", "mask", "colsum"):
        assert any(c["epi"].get(key) for c in C.GG_CASES), key
    assert any(c["epi"].get("scale", 1) < 0 for c in C.GG_CASES)
    geo = [C.gg_geometry(c) for c in C.GG_CASES]
    assert any(g[4] % 128 for g in geo) and any(c["Nout"] % 128 and c["Nout"] > 128 for c in C.GG_CASES)
    assert any(c["lda"] > c["Kc"] for c in C.GG_CASES) and any(c["ldo"] > c["Nout"] for c in C.GG_CASES)
    thw = [g[0][3] * g[0][4] for g, c in zip(geo, C.GG_CASES) if c["op"] != "linear"]
    assert any(t & (t - 1) == 0 for t in thw) and any(t & (t - 1) for t in thw)


def test_every_wgrad_gemm_instance_has_a_gpu_case():
    reached = set()
    padded = False
    for c in C.WG_CASES:
        inst, grid, blocks = C.wg_case_instance(c)
        assert inst == c["inst"], (c["id"], inst)
        reached.add(inst)
        padded |= grid > blocks
    assert C.WG_REACHABLE <= reached, sorted(C.WG_REACHABLE - reached)
    assert padded                                             # XCD-padding workgroups run (ksplit > 1, blocks % 8 != 0)
    assert any(c["ks"] > 1 and C.cdiv(C.cdiv(C.wg_geometry(c)[0], c["ks"]), 64) * 64 * (c["ks"] - 1) >= C.wg_geometry(c)[0]
               for c in C.WG_CASES)                          # and K-slices with no pixels at all
