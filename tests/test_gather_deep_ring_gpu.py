"""The 64-row tile instance of rbvae_gather_gemm (gather_gemm_k<bf16, 2, 4, RING, 1, 64>: deep K, at most 64 128 x 128
blocks, more than 64 output channels, no column sums) with its deep LDS ring: K loops shorter than, equal to and longer
than the ring, partial row and channel tiles, taps that read the zero rows, and the epilogue options.

Every case is a 3 x 3 stride-2 convolution of 8 x 8 maps restricted to a subset of its taps (the float64 reference is the
convolution with the other taps' weights set to zero), compared element by element under the error model of
tests/_bounds.py inside guard-padded buffers."""
import ctypes

import pytest
import torch

import _bounds as B
import _conv_cases as C
from _ends_cases import keyed_keep_mask

pytestmark = pytest.mark.gpu

RING = 6                    # GG_RING64 of csrc/gather_gemm.hip: the ring depth the build ships
# taps in the order the cases take them: (-1, -1) first, so every case gathers rows outside the image (output row 0 and
# column 0 of a stride-2, pad-1 convolution read input row / column -1)
TAP_ORDER = [0, 8, 2, 4, 6, 1, 3, 5, 7]
# (taps, Kc): K loops of taps * Kc / 64 slices
LOOPS = [(3, 64), (RING - 1, 64), (RING, 64), (RING // 2, 128), (RING + 1, 64), (1, 256), (2, 192), (4, 128), (9, 256)]
SHAPES = [(3, 128), (9, 128), (3, 72), (9, 72)]                        # (images, Nout): 48 / 144 rows, whole / partial N tile


def test_loops_straddle_the_ring():
    steps = {t * kc // 64 for t, kc in LOOPS}
    assert {3, RING - 1, RING, RING + 1, 36} <= steps
    assert all(1 <= t <= 9 and kc % 64 == 0 and 64 <= kc <= 256 for t, kc in LOOPS)


@pytest.fixture(scope="module")
def lib():
    import sfv_amd
    return sfv_amd._lib


def run_case(lib, nimg, nout, ntaps, kc, lda_pad=0, ldo_pad=0, bias=False, relu=False, drop=None, gate=False, scale=1.0):
    H = W = 8
    Ho = Wo = 4
    rows = nimg * Ho * Wo
    assert C.gg_instance("bf16", rows, nout, 1, ntaps * kc // 64, False)[0] == "ns3_64sq"
    g = torch.Generator().manual_seed(1000 * nimg + 10 * nout + ntaps * kc)
    taps = TAP_ORDER[:ntaps]
    x = torch.randn(nimg, kc, H, W, generator=g).bfloat16()
    w = (torch.randn(nout, kc, 3, 3, generator=g) / (ntaps * kc) ** 0.5).bfloat16()
    wm = torch.zeros_like(w)
    for t in taps:
        wm[:, :, t // 3, t % 3] = w[:, :, t // 3, t % 3]
    ref, S = B.ref_and_scale("conv2d", x, wm, stride=2)
    ref, S = B.rows(ref), B.rows(S)
    bias_t = None
    if bias:
        bias_t = torch.randn(nout, generator=g) * 0.5
        ref, S = ref + bias_t.double(), S + bias_t.double().abs()
    if relu:
        ref = ref.clamp_min(0)
    ref = ref * scale
    seed, p = 0, 0.0
    if drop is not None:
        seed, p = drop
        ref = ref * torch.from_numpy(keyed_keep_mask(rows, nout, seed, p))
    gate_g = None
    if gate:
        gv = torch.randn(rows, nout, generator=g).bfloat16()
        ref = ref * (gv > 0)
        gate_g = B.poisoned(gv, nout + ldo_pad, torch.bfloat16)
    lda, ldo = kc + lda_pad, nout + ldo_pad
    A = B.poisoned(B.rows(x), lda, torch.bfloat16)
    Wp = B.poisoned(w.permute(0, 2, 3, 1).reshape(nout, -1), 9 * kc, torch.bfloat16)       # all nine taps: widx picks
    out = B.guarded(rows, ldo, nout, torch.bfloat16)
    d = [ntaps, 0, 0]
    for t in taps:
        d += [t, t // 3 - 1, t % 3 - 1]
    desc = (ctypes.c_int * len(d))(*d)
    zero = torch.zeros(256, dtype=torch.uint8, device="cuda")
    lib.call("rbvae_gather_gemm", 1, A.view, Wp.view, out.view, bias_t.cuda() if bias else None, gate_g and gate_g.view,
             None, None, zero, nimg, H, W, Ho, Wo, 2, Ho, Wo, 1, kc, nout, lda, ldo, 9, 1, ctypes.addressof(desc),
             int(relu), 1 if drop is not None else 0, p, scale, seed, None, None)
    torch.cuda.synchronize()
    what = f"deep ring N{nimg} Nout{nout} taps{ntaps} Kc{kc}"
    # rows beyond Mc and columns beyond Nout of the padded output stay untouched, every declared element is written
    B.assert_guards(out, what)
    worst = B.check(out.out, ref, S, out_dtype=torch.bfloat16, K=ntaps * kc, scale=scale, nhw=(nimg, Ho, Wo), what=what)
    print(f"\nBOUNDS gather_gemm 64-row ring {RING}: {what} worst |err|/bound = {worst:.3g}")


@pytest.mark.parametrize("ntaps,kc", LOOPS, ids=[f"{t}x{k}" for t, k in LOOPS])
@pytest.mark.parametrize("nimg,nout", SHAPES, ids=[f"N{n}o{o}" for n, o in SHAPES])
def test_deep_ring_bounded_and_guarded(lib, nimg, nout, ntaps, kc):
    run_case(lib, nimg, nout, ntaps, kc, lda_pad=64 if nimg == 9 else 0, ldo_pad=8 if nout == 72 else 0)


@pytest.mark.parametrize("ntaps,kc", [(3, 64), (RING + 1, 64), (9, 256)])
def test_deep_ring_bias_relu_keyed_dropout(lib, ntaps, kc):
    run_case(lib, 9, 72, ntaps, kc, ldo_pad=8, bias=True, relu=True, drop=(11, 0.2), scale=1.25)


@pytest.mark.parametrize("ntaps,kc", [(RING - 1, 64), (9, 256)])
def test_deep_ring_gate(lib, ntaps, kc):
    run_case(lib, 3, 128, ntaps, kc, lda_pad=64, gate=True, scale=0.5)
