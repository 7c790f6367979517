"""The raw-frame ABI (include/rbvae_hip.h, "raw frames in") restated in numpy as the header words it, the named defects
the tests must be able to tell from it, and the cases tests/test_frames_abi_cpu.py and tests/test_frames_abi_gpu.py run.

No Pillow here and none of frames.py's kernels: only its host-side coefficient tables (sfv.resample_coeffs), which
boxed_coeffs generalises to Pillow's source box.  A box is what makes the first vertical bound positive, so it is the only
way to the ABI's row0 > 0 (frames.py's resize_u8 never passes one).

Defects (each a one-line change of a reference; test_frames_abi_cpu.py shows that every one changes a byte of a case):
  resample_ref   no_round_constant         acc starts at 0 instead of 1 << 21
                 logical_shift             acc >> 22 on the unsigned bit pattern (a negative acc clips to 255, not 0)
                 h_ignores_row0            the horizontal pass reads source row r instead of row0 + r
                 v_ignores_row0            the vertical pass reads source row first + t instead of first - row0 + t
                 edge_tap_not_skipped      a tap outside the source reads the nearest source element instead of nothing
                 taps_not_clamped_to_ksize taps > ksize runs on into the next row of kk (or the table's guard band)
  perturb_ref    fma_noise                 noise * std + mean rounded once
                 times_reciprocal          x * (1 / 255) instead of x / 255
                 round_not_trunc           round to nearest instead of truncation
                 no_clamp                  no clamp to [0, 1] (the byte wraps)
  to_input_ref   times_reciprocal          as above
A contraction of mode 1's 2 * q - 1 into one fused operation is NOT a defect that can show: 2 * q is exact in binary
floating point, so fma(2, q, -1) and (2 * q) - 1 round the same real number once.  No defect is invented for it."""
import functools

import numpy as np
import torch

import sfv_amd as sfv
from _frames_ref import frame_image, to_tensor

PREC = 22
TABLE_GUARD_WORD = 0x01010101          # what the int32 bands around bounds / kk hold on the device
F32 = np.float32

RESAMPLE_DEFECTS = ("no_round_constant", "logical_shift", "h_ignores_row0", "v_ignores_row0", "edge_tap_not_skipped",
                    "taps_not_clamped_to_ksize")
PERTURB_DEFECTS = ("fma_noise", "times_reciprocal", "round_not_trunc", "no_clamp")
TO_INPUT_DEFECTS = ("times_reciprocal",)


# ---- the resampler --------------------------------------------------------------------------------------------------

def resample_ref(x, vertical, row0, out_h, bounds, kk, ksize, defect=None, return_acc=False):
    """rbvae_resample_u8 of x u8 [N][in_h][in_w][3] in int64.  vertical = 0: -> [N][out_h][len(bounds)][3], output row r
    from source row row0 + r; vertical = 1: -> [N][out_h = len(bounds)][in_w][3], output row yy from source rows
    bounds[yy][0] - row0 + t.  Asserts the int32 precondition |acc| < 2^31 of the unmodified arithmetic."""
    x = np.asarray(x).astype(np.int64)
    bounds = np.asarray(bounds, dtype=np.int64).reshape(-1, 2)
    n_out = bounds.shape[0]
    kflat = np.asarray(kk, dtype=np.int64).reshape(-1)
    assert kflat.shape[0] == n_out * ksize and x.ndim == 4 and x.shape[3] == 3
    first, taps = bounds[:, 0], bounds[:, 1]
    if vertical:
        assert n_out == out_h
        src, in_size, axis = x, x.shape[1], 1
        if defect != "v_ignores_row0":
            first = first - row0
    else:
        r0 = 0 if defect == "h_ignores_row0" else row0
        assert 0 <= row0 and row0 + out_h <= x.shape[1]
        src, in_size, axis = x[:, r0:r0 + out_h], x.shape[2], 2
    t_end = ksize
    if defect == "taps_not_clamped_to_ksize":
        t_end = max(ksize, int(taps.max(initial=0)))
        kflat = np.concatenate([kflat, np.full(t_end, TABLE_GUARD_WORD, dtype=np.int64)])
    else:
        taps = np.minimum(taps, ksize)
    shape = [1, 1, 1, 1]
    shape[axis] = n_out
    acc = np.full(src.shape[:axis] + (n_out,) + src.shape[axis + 1:], 0 if defect == "no_round_constant" else 1 << (PREC - 1),
                  dtype=np.int64)
    o = np.arange(n_out)
    for t in range(t_end):
        idx = first + t
        live = t < taps
        if defect != "edge_tap_not_skipped":
            live = live & (idx >= 0) & (idx < in_size)
        c = np.where(live, kflat[o * ksize + t], 0)
        acc += np.take(src, np.clip(idx, 0, in_size - 1), axis=axis) * c.reshape(shape)
    if defect is None:
        assert int(np.abs(acc).max(initial=0)) < 2 ** 31, "the table breaks the int32 precondition"
    v = ((acc & 0xFFFFFFFF) >> PREC) if defect == "logical_shift" else (acc >> PREC)
    res = np.clip(v, 0, 255).astype(np.uint8)
    return (res, acc) if return_acc else res


def boxed_coeffs(in_size, in0, in1, out_size, filter):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc (Resample.c) for one axis with the source box [in0, in1):
    scale = (in1 - in0) / out_size, center = in0 + (xx + 0.5) * scale; everything else as frames.py's _coeffs."""
    import math
    fn, fsupport = sfv.frames.FILTERS[filter]
    scale = (float(in1) - float(in0)) / out_size
    filterscale = max(scale, 1.0)
    support = fsupport * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    kk = np.zeros((out_size, ksize), dtype=np.int32)
    for xx in range(out_size):
        center = in0 + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [fn((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        kk[xx, :xmax] = [int(-0.5 + v * (1 << PREC)) if v < 0 else int(0.5 + v * (1 << PREC)) for v in w]
        bounds[xx] = (xmin, xmax)
    return bounds, kk


# (source W, H), box (left, upper, right, lower), output (W, H), filter, row0 / rows of the horizontal pass (None: the
# width and the box's sides do not change, Pillow skips the horizontal pass and the vertical one runs with row0 = 0)
BOXED = [
    ((67, 90), (5, 31, 60, 77), (29, 17), "lanczos", (24, 60)),
    ((67, 90), (0, 40, 67, 90), (67, 13), "lanczos", None),
    ((45, 64), (3, 20, 40, 50), (90, 70), "bilinear", (19, 32)),
    ((131, 83), (10, 25, 121, 70), (64, 20), "lanczos", (19, 57)),
    ((70, 200), (1, 120, 69, 190), (33, 9), "bilinear", (116, 78)),
]


@functools.lru_cache(maxsize=None)
def boxed_case(i):
    """-> dict: x u8 [1][ih][iw][3], h = (row0, rows, bounds, kk) or None, v = (row0, bounds, kk), mid (the horizontal
    pass's output, or x) and out, both by resample_ref."""
    (iw, ih), box, (ow, oh), filt, rows = BOXED[i]
    x = frame_image(np.random.default_rng(iw), iw, ih)[None]
    bv, kv = boxed_coeffs(ih, box[1], box[3], oh, filt)
    d = dict(x=x, box=box, size=(ow, oh), filter=filt, h=None)
    mid, row0 = x, 0
    if rows is not None:
        bh, kh = boxed_coeffs(iw, box[0], box[2], ow, filt)
        row0, last = int(bv[0, 0]), int(bv[-1, 0] + bv[-1, 1])
        assert (row0, last - row0) == rows
        mid = resample_ref(x, 0, row0, last - row0, bh, kh, kh.shape[1])
        d["h"] = (row0, last - row0, bh, kh)
    d["v"] = (row0, bv, kv)
    d["mid"] = mid
    d["out"] = resample_ref(mid, 1, row0, oh, bv, kv, kv.shape[1])
    return d


def synthetic_table(n_out, in_size, row0, seed, ksize=7):
    """A table no resampler makes: coefficients in [-2^20, 2^21], first in [row0 - 3, row0 + in_size + 2], taps in
    [0, ksize + 2]; every fifth row all negative (acc < 0: clips to 0), every fifth all positive with a sum above 2^22
    (clips to 255 on bright pixels).  A row whose sum |k| would let 255 * sum |k| + 2^21 reach 2^31 is scaled down to
    sum |k| <= 8 000 000, so the int32 precondition holds for any u8 input."""
    rng = np.random.default_rng(seed)
    k = rng.integers(-2 ** 20, 2 ** 21 + 1, (n_out, ksize))
    k[1::5] = -np.clip(np.abs(k[1::5]), 1, 2 ** 20)
    k[2::5] = np.maximum(np.abs(k[2::5]), 2 ** 20)
    s = np.abs(k).sum(1, keepdims=True)
    k = np.where(s > 8_000_000, np.sign(k) * (np.abs(k) * 8_000_000 // np.maximum(s, 1)), k)
    assert int(np.abs(k).sum(1).max()) * 255 + (1 << 21) < 2 ** 31 and int(k.min()) >= -2 ** 20 and int(k.max()) <= 2 ** 21
    assert bool((k[2::5].sum(1) > 2 ** 22).all()) and bool((k[1::5] < 0).all())
    first = rng.integers(row0 - 3, row0 + in_size + 3, n_out)
    taps = rng.integers(0, ksize + 3, n_out)
    # the corners, whatever the draw: before the source, past its end, and rows longer than ksize inside it
    first[:6] = [row0 - 3, row0 + in_size - 2, row0 + in_size + 2, row0, row0 + in_size - ksize, row0 - 1]
    taps[:6] = [ksize, ksize + 2, 3, ksize + 2, ksize + 1, 0]
    bounds = np.stack([first, taps], 1).astype(np.int32)
    return bounds, k.astype(np.int32)


def _rc(in_size, out_size, filt):
    b, k = sfv.resample_coeffs(in_size, out_size, filt)
    return np.array(b), np.array(k)


def _h(id, x, row0, out_h, table, in_off=0, out_off=0):
    return dict(id=id, vertical=0, x=x, row0=row0, out_h=out_h, bounds=table[0], kk=table[1], ksize=table[1].shape[1],
                in_off=in_off, out_off=out_off)


def _v(id, x, row0, table, in_off=0, out_off=0):
    row_bytes = 3 * x.shape[2]
    path = "vector" if row_bytes % 4 == 0 and in_off % 4 == 0 and out_off % 4 == 0 else "scalar"
    return dict(id=id, vertical=1, x=x, row0=row0, out_h=table[0].shape[0], bounds=table[0], kk=table[1],
                ksize=table[1].shape[1], in_off=in_off, out_off=out_off, path=path)


def _frames(seed, w, h, n):
    return frame_image(np.random.default_rng(seed), w, h, n)


@functools.lru_cache(maxsize=None)
def horizontal_cases():
    """Without the two LDS-boundary sizes (lds_case)."""
    cases = []
    x = _frames(1, 7, 4, 2)
    for i in range(4):                       # rows of 21 -> 15 bytes: the lead of either side changes from row to row
        for o in range(4):
            cases.append(_h(f"align-in{i}-out{o}", x, 1, 3, _rc(7, 5, "lanczos"), i, o))
    x = _frames(2, 97, 3, 1)
    for ow in (1, 255, 256, 257, 300):       # one trip, a full trip, a second trip of the per-thread loop
        cases.append(_h(f"out_w{ow}", x, 1, 2, _rc(97, ow, "bilinear")))
    cases.append(_h("in_w1", _frames(3, 1, 3, 2), 0, 3, _rc(1, 4, "bilinear")))
    cases.append(_h("N3", _frames(4, 33, 5, 3), 2, 3, _rc(33, 20, "lanczos")))
    for i in range(len(BOXED)):
        d = boxed_case(i)
        if d["h"] is not None:
            row0, rows, bh, kh = d["h"]
            cases.append(_h(f"boxed{i}", d["x"], row0, rows, (bh, kh)))
    x = _frames(5, 23, 6, 2)
    x[:, 3] = 255                            # a bright row: the positive rows of the table overflow 255 there
    cases.append(_h("synthetic", x, 2, 3, synthetic_table(40, 23, 0, seed=6)))
    return cases


@functools.lru_cache(maxsize=None)
def lds_case():
    """in_w = out_w = 10921: both LDS rows are (3 * 10921 + 7) & ~3 = 32768 bytes, 65536 together, the largest the entry
    point accepts; out_w = 10922 is the first it refuses."""
    x = _frames(7, 10921, 1, 1)
    return _h("lds65536", x, 0, 1, _rc(10921, 10921, "bilinear"))


@functools.lru_cache(maxsize=None)
def vertical_cases():
    cases = []
    tab = boxed_coeffs(16, 3, 14, 4, "bilinear")
    row0 = int(tab[0][0, 0])
    in_h = int(tab[0][-1, 0] + tab[0][-1, 1]) - row0
    assert row0 > 0
    for W, io, oo in ((4, 0, 0), (4, 1, 0), (4, 0, 2), (5, 0, 0), (87, 0, 0), (344, 0, 0)):
        cases.append(_v(f"W{W}-in{io}-out{oo}", _frames(10 + W, W, in_h, 2), row0, tab, io, oo))
    for i in range(len(BOXED)):
        d = boxed_case(i)
        row0, bv, kv = d["v"]
        cases.append(_v(f"boxed{i}", d["mid"], row0, (bv, kv)))
    for W in (4, 5):                         # the synthetic table on either path
        x = _frames(20 + W, W, 11, 2)
        x[:, 4] = 255
        cases.append(_v(f"synthetic-W{W}", x, 9, synthetic_table(17, 11, 9, seed=8 + W)))
    return cases


def case_ref(c, defect=None, return_acc=False):
    return resample_ref(c["x"], c["vertical"], c["row0"], c["out_h"], c["bounds"], c["kk"], c["ksize"], defect, return_acc)


# ---- ToTensor -> perturbation -> ToPILImage, and the model inputs ---------------------------------------------------------

def _unit(x, defect):
    x = np.asarray(x).astype(F32)
    return x * F32(1.0 / 255.0) if defect == "times_reciprocal" else x / F32(255.0)


def perturb_ref(x, kind, noise=None, std=0.0, mean=0.0, boxes=None, defect=None):
    """rbvae_perturb_u8 of x u8 [N][H][W][3] in f32, one rounding per operation: x / 255; kind 1: noise * std, + mean,
    the add, the clamp; kind 2: 0.5 inside boxes[n] = (x, y, size); then * 255 and truncation."""
    v = _unit(x, defect)
    N, H, W, _ = v.shape
    if kind == 1:
        n = np.transpose(np.asarray(noise, dtype=F32).reshape(N, 3, H, W), (0, 2, 3, 1))
        if defect == "fma_noise":
            t = (n.astype(np.float64) * np.float64(F32(std)) + np.float64(F32(mean))).astype(F32)
        else:
            t = n * F32(std)
            t = t + F32(mean)
        v = v + t
        if defect != "no_clamp":
            v = np.minimum(np.maximum(v, F32(0.0)), F32(1.0))
    else:
        assert kind == 2
        v = v.copy()
        for j, (bx, by, bs) in enumerate(np.asarray(boxes).reshape(N, 3).tolist()):
            assert 0 <= bx <= W - bs and 0 <= by <= H - bs and bs >= 0, "outside the reference's domain"
            v[j, by:by + bs, bx:bx + bs] = F32(0.5)
    v = v * F32(255.0)
    i = np.rint(v) if defect == "round_not_trunc" else np.trunc(v)
    return (i.astype(np.int64) & 0xFF).astype(np.uint8)


def to_input_ref(x, mode, defect=None):
    """rbvae_u8_to_input: u8 [N][H][W][3] -> f32 [N][3][H][W], x / 255 (mode 0) and then 2 * q - 1 (mode 1)."""
    v = _unit(x, defect)
    if mode == 1:
        v = F32(2.0) * v
        v = v - F32(1.0)
    else:
        assert mode == 0
    return np.ascontiguousarray(np.transpose(v, (0, 3, 1, 2)))


def _boundary_noise(a, std, rng):
    """noise whose sum with x/255 lands within an ulp of a k/255 boundary: the truncation of mul(255).byte() decides"""
    x = to_tensor(a)
    k = torch.from_numpy(rng.integers(0, 256, x.shape)).float()
    target = k / 255
    n = (target - x) / std
    ulps = torch.from_numpy(rng.integers(-2, 3, x.shape)).float()
    n = n + ulps * torch.finfo(torch.float32).eps * n.abs().clamp_min(1e-3)
    return n


def all_bytes_frames():
    """u8 [1][16][16][3]: every byte value in every channel, in a different order per channel."""
    v = np.arange(256, dtype=np.uint8)
    return np.stack([v, v[::-1], np.roll(v, 77)], 1).reshape(1, 16, 16, 3).copy()


PERTURB_HW = (37, 53)
NOISE_PARAMS = [(0.1, 0.0), (0.3, 0.05), (1.0, -0.5)]


@functools.lru_cache(maxsize=None)
def perturb_frames():
    return frame_image(np.random.default_rng(3), PERTURB_HW[1], PERTURB_HW[0], 4)


@functools.lru_cache(maxsize=None)
def noise_for(std, mean):
    """f32 [4][3][H][W]: frames 0 and 1 sit on the truncation boundaries of (std, mean), 2 and 3 are normal draws."""
    H, W = PERTURB_HW
    a = perturb_frames()
    rng = np.random.default_rng(int(std * 100) + 5)
    noise = torch.randn(4, 3, H, W, generator=torch.Generator().manual_seed(5))
    noise[:2] = torch.stack([_boundary_noise(a[j], std, rng) for j in range(2)]) - mean / std
    return noise.numpy()


@functools.lru_cache(maxsize=None)
def perturb_cases():
    """-> [dict(id, x, kind, noise, std, mean, boxes)]"""
    H, W = PERTURB_HW
    a = perturb_frames()
    cases = [dict(id=f"noise-std{std}-mean{mean}", x=a, kind=1, noise=noise_for(std, mean), std=std, mean=mean, boxes=None)
             for std, mean in NOISE_PARAMS]
    boxes = np.array([(5, 7, 0), (W - 1, H - 1, 1), (W - H, 0, H), (0, H - 10, 10)], dtype=np.int32)
    cases.append(dict(id="boxes", x=a, kind=2, noise=None, std=0.0, mean=0.0, boxes=boxes))
    b = all_bytes_frames()
    cases.append(dict(id="all-bytes-box0", x=b, kind=2, noise=None, std=0.0, mean=0.0, boxes=np.array([(3, 3, 0)], dtype=np.int32)))
    small = torch.randn(1, 3, 16, 16, generator=torch.Generator().manual_seed(6)).numpy()
    cases.append(dict(id="all-bytes-noise", x=b, kind=1, noise=small, std=0.01, mean=0.0, boxes=None))
    return cases


def perturb_case_ref(c, defect=None):
    return perturb_ref(c["x"], c["kind"], c["noise"], c["std"], c["mean"], c["boxes"], defect)


def to_input_frames():
    """u8 [3][5][7][3]: 315 bytes, all 256 values, shuffled; H * W = 35 and 3 * 35 are the NCHW scatter's strides."""
    v = np.arange(315) % 256
    return np.random.default_rng(9).permutation(v).astype(np.uint8).reshape(3, 5, 7, 3)


def unit_table():
    """f32 [256]: the true quotient v / 255 rounded once (test_frames_cpu.py::test_totensor_is_true_division)."""
    return (torch.arange(256, dtype=torch.float64) / 255).float()
