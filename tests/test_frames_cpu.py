"""CPU: frames.resample_coeffs is Pillow's coefficient table.  Applied with a plain numpy loop (the arithmetic
csrc/frames.hip runs: 22-bit fixed point, horizontal pass over the rows the vertical pass reads, then vertical), it
reproduces PIL.Image.resize byte for byte; and the f32 steps the kernels restate round as the reference does."""
import numpy as np
import pytest
import torch

import sfv_amd as sfv
from _frames_ref import CASES, pil_resize, frame_image

pytest.importorskip("PIL")


def _axis(img, bounds, kk, axis, row0=0):
    img = np.moveaxis(img.astype(np.int64), axis, 0)
    out = np.empty((bounds.shape[0],) + img.shape[1:], dtype=np.int64)
    for o, (first, taps) in enumerate(bounds):
        acc = np.full(img.shape[1:], 1 << 21, dtype=np.int64)
        for t in range(taps):
            acc += img[first - row0 + t] * int(kk[o, t])
        assert np.abs(acc).max() < 2 ** 31                      # the kernels sum in int32
        out[o] = np.clip(acc >> 22, 0, 255)
    return np.moveaxis(out, 0, axis).astype(np.uint8)


def np_resize(a, size, filt):
    W, H = size
    IH, IW = a.shape[:2]
    if (W, H) == (IW, IH):
        return a.copy()
    bv, kv = sfv.resample_coeffs(IH, H, filt)
    row0 = 0
    if W != IW:
        y0, y1 = (int(bv[0, 0]), int(bv[-1, 0] + bv[-1, 1])) if H != IH else (0, IH)
        bh, kh = sfv.resample_coeffs(IW, W, filt)
        a, row0 = _axis(a[y0:y1], bh, kh, 1), y0
    if H != IH:
        a = _axis(a, bv, kv, 0, row0)
    return a


@pytest.mark.parametrize("iw,ih,ow,oh,filt", CASES)
def test_coeffs_reproduce_pillow(iw, ih, ow, oh, filt):
    a = frame_image(np.random.default_rng(iw * 1000 + ih), iw, ih)
    assert np.array_equal(np_resize(a, (ow, oh), filt), pil_resize(a, (ow, oh), filt))


def test_reference_chain():
    """load_img's two LANCZOS resizes of a 1920 x 1080 frame (get_percep_embeddings.py:59-66)."""
    a = frame_image(np.random.default_rng(7), 1920, 1080)
    mid = pil_resize(a, (1280, 720), "lanczos")
    assert np.array_equal(np_resize(a, (1280, 720), "lanczos"), mid)
    assert np.array_equal(np_resize(mid, (1280, 704), "lanczos"), pil_resize(mid, (1280, 704), "lanczos"))


def test_coeff_table_shape_and_sum():
    b, k = sfv.resample_coeffs(1920, 1280, "lanczos")
    assert b.dtype == np.int32 and k.dtype == np.int32 and b.shape == (1280, 2) and k.shape == (1280, 2 * 5 + 1)
    assert np.all(np.abs(k.sum(axis=1) - (1 << 22)) <= k.shape[1])
    assert np.all(b[:, 0] >= 0) and np.all(b[:, 0] + b[:, 1] <= 1920) and np.all(b[:, 1] <= k.shape[1])
    assert sfv.resample_coeffs(1920, 1280, "lanczos")[1] is k                  # cached
    with pytest.raises(ValueError):
        sfv.resample_coeffs(10, 5, "bicubic")
    with pytest.raises(ValueError):
        sfv.resample_coeffs(0, 5, "bilinear")


def test_totensor_is_true_division():
    """ToTensor's div(255) rounds as a true f32 division (what the kernels compute), not as a multiply by 1/255."""
    v = torch.arange(256, dtype=torch.uint8)
    got = v.to(torch.float32).div(255)
    true = (v.double() / 255).float()              # exact quotient rounded once
    assert torch.equal(got, true)
    assert torch.equal(torch.from_numpy(np.arange(256, dtype=np.uint8).astype(np.float32) / 255.0), true)
    assert not torch.equal(v.to(torch.float32) * np.float32(1 / 255), true)
