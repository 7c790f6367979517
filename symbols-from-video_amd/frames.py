"""Raw video frames in: the reference's Pillow preprocessing as device work on u8 frames (csrc/frames.hip).

The reference reads a folder of `%010d.jpg` frames and prepares one frame at a time with Pillow:
  perceptual models   src/stable-diffusion/get_percep_embeddings.py:48-71 (load_img) and
                      scripts/evaluation/state_consistency_eval/embedding_matching.py:318-338 (load_img_for_sd):
                      LANCZOS to 1280 x 720, LANCZOS again to the sides rounded down to a multiple of 32, /255, 2x-1
  contrastive models  models/contrastive_RBVAE/contrastive_RBVAE_train.py:110-114 (ImageTransforms):
                      T.Resize((256, 256)) = a Pillow BILINEAR resize, then ToTensor
Here the frames are u8 [N,H,W,3] (NHWC, the layout a decoded JPEG has) on the device -- a quarter of the f32 bytes, so
a whole video can sit in HBM -- and every step is a batched kernel that reproduces Pillow's 8-bit resampler
(Pillow's src/libImaging/Resample.c: double-precision coefficients, 22-bit fixed point, horizontal pass first) and the
f32 operations of torchvision's ToTensor / ToPILImage bit for bit.  JPEG decoding stays on the host (load_frames).
"""
from __future__ import annotations

import concurrent.futures
import functools
import math
import os
import random
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L

PRECISION_BITS = 32 - 8 - 2             # Resample.c: 8-bit images keep 22 fractional bits
MODE_TOTENSOR, MODE_SD = 0, 1           # rbvae_u8_to_input modes
PERTURB_NOISE, PERTURB_OCCLUSION = 1, 2  # rbvae_perturb_u8 kinds


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    if -3.0 <= x < 3.0:
        return _sinc(x) * _sinc(x / 3)
    return 0.0


def _bilinear(x):
    if x < 0.0:
        x = -x
    if x < 1.0:
        return 1.0 - x
    return 0.0


# the two filters the reference uses: (function, support)
FILTERS = {"lanczos": (_lanczos, 3.0), "bilinear": (_bilinear, 1.0)}


@functools.lru_cache(maxsize=None)
def _coeffs(in_size, out_size, filt):
    fn, fsupport = FILTERS[filt]
    scale = float(in_size) / out_size
    filterscale = max(scale, 1.0)
    support = fsupport * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    kk = np.zeros((out_size, ksize), dtype=np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [fn((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        # normalize_coeffs_8bpc: round half away from zero at 2**22
        kk[xx, :xmax] = [int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
                         for v in w]
        bounds[xx] = (xmin, xmax)
    bounds.setflags(write=False)
    kk.setflags(write=False)
    return bounds, kk


def resample_coeffs(in_size: int, out_size: int, filter: str = "lanczos") -> Tuple[np.ndarray, np.ndarray]:
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc (Resample.c) for one axis: bounds int32 [out][2] =
    (first source index, number of taps) and coefficients int32 [out][ksize] with 22 fractional bits.  Cached per key;
    the arrays are read-only."""
    if filter not in FILTERS:
        raise ValueError(f"filter must be one of {sorted(FILTERS)}, got {filter!r}")
    if int(in_size) < 1 or int(out_size) < 1:
        raise ValueError(f"sizes must be positive, got {in_size} -> {out_size}")
    return _coeffs(int(in_size), int(out_size), filter)


_dev_coeffs = {}


def _device_coeffs(in_size, out_size, filt, device):
    key = (in_size, out_size, filt, str(device))
    t = _dev_coeffs.get(key)
    if t is None:
        b, k = resample_coeffs(in_size, out_size, filt)
        t = _dev_coeffs[key] = (torch.from_numpy(b.copy()).to(device), torch.from_numpy(k.copy()).to(device), k.shape[1])
    return t


def _check_u8(frames, name="frames"):
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8:
        raise ValueError(f"{name} must be a uint8 tensor [N,H,W,3], got "
                         f"{frames.dtype if isinstance(frames, torch.Tensor) else type(frames).__name__}")
    if frames.dim() != 4 or frames.shape[3] != 3:
        raise ValueError(f"{name} must be [N,H,W,3] (RGB, NHWC), got {tuple(frames.shape)}")
    if not frames.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if not frames.is_cuda:
        raise ValueError(f"{name} must be on the GPU (there is no CPU path)")
    if frames.shape[0] == 0 or frames.shape[1] == 0 or frames.shape[2] == 0:
        raise ValueError(f"{name} is empty: {tuple(frames.shape)}")


def _check_out(out, shape, dtype, device):
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if tuple(out.shape) != tuple(shape) or out.dtype != dtype or out.device != device or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous {dtype} tensor of shape {tuple(shape)} on {device}")
    return out


def resize_u8(frames: torch.Tensor, size: Tuple[int, int], filter: str = "lanczos",
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """PIL.Image.resize(size=(W, H), resample=LANCZOS | BILINEAR) of every frame of u8 [N,H,W,3]: the same size is a
    copy; otherwise the horizontal pass (over the source rows the vertical pass reads) and then the vertical pass, each
    skipped when its side does not change (ImagingResampleInner)."""
    _check_u8(frames)
    W, H = int(size[0]), int(size[1])
    if W < 1 or H < 1:
        raise ValueError(f"size must be positive (W, H), got {size}")
    N, IH, IW, _ = frames.shape
    res = _check_out(out, (N, H, W, 3), torch.uint8, frames.device)
    if (W, H) == (IW, IH):
        res.copy_(frames)
        return res
    need_h, need_v = W != IW, H != IH
    src, row0 = frames, 0
    if need_h:
        if need_v:
            bv, _ = resample_coeffs(IH, H, filter)
            y_first, y_last = int(bv[0, 0]), int(bv[-1, 0] + bv[-1, 1])
        else:
            y_first, y_last = 0, IH
        tmp = res if not need_v else torch.empty((N, y_last - y_first, W, 3), dtype=torch.uint8, device=frames.device)
        b, k, ks = _device_coeffs(IW, W, filter, frames.device)
        L.call("rbvae_resample_u8", frames, tmp, N, IH, IW, y_last - y_first, W, 0, y_first, b, k, ks)
        src, row0 = tmp, y_first
    if need_v:
        b, k, ks = _device_coeffs(IH, H, filter, frames.device)
        L.call("rbvae_resample_u8", src, res, N, src.shape[1], W, H, W, 1, row0, b, k, ks)
    return res


def u8_to_input(frames: torch.Tensor, mode: str = "totensor", out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """u8 [N,H,W,3] -> f32 [N,3,H,W]: "totensor" = ToTensor (x / 255), "sd" = load_img's 2 * (x / 255) - 1 (two
    roundings, as the reference).  out: write into this contiguous f32 tensor (e.g. the buffer the encoder reads)."""
    _check_u8(frames)
    m = {"totensor": MODE_TOTENSOR, "sd": MODE_SD}.get(mode)
    if m is None:
        raise ValueError(f"mode must be 'totensor' or 'sd', got {mode!r}")
    N, H, W, _ = frames.shape
    if out is not None and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == N * 3 * H * W \
            and out.device == frames.device:
        out = out.view(N, 3, H, W)
    res = _check_out(out, (N, 3, H, W), torch.float32, frames.device)
    L.call("rbvae_u8_to_input", frames, res, N, H, W, m)
    return res


def sd_target(target=(1280, 720)):
    """(W, H) after load_img's round-down of both sides to a multiple of 32."""
    w, h = int(target[0]), int(target[1])
    return w - w % 32, h - h % 32


def sd_resize(frames: torch.Tensor, target=(1280, 720)) -> torch.Tensor:
    """load_img's two LANCZOS resizes on u8 frames: to `target`, then to the sides rounded down to a multiple of 32."""
    w, h = sd_target(target)
    if w < 32 or h < 32:
        raise ValueError(f"target {target} rounds down to {(w, h)}")
    x = resize_u8(frames, target, "lanczos")
    if (w, h) != tuple(target):
        x = resize_u8(x, (w, h), "lanczos")
    return x


def sd_input(frames: torch.Tensor, target=(1280, 720), out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """load_img / load_img_for_sd (get_percep_embeddings.py:48-71, embedding_matching.py:318-338) on u8 [N,H,W,3]:
    -> f32 [N,3,h,w] in [-1,1], h, w the target's sides rounded down to a multiple of 32 (1280 x 704 by default)."""
    return u8_to_input(sd_resize(frames, target), "sd", out=out)


def contrastive_input(frames: torch.Tensor, resolution: int = 256, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ImageTransforms (contrastive_RBVAE_train.py:110-114: T.Resize((r, r)) = Pillow BILINEAR, then ToTensor) on
    u8 [N,H,W,3] -> f32 [N,3,r,r] in [0,1]."""
    r = int(resolution)
    return u8_to_input(resize_u8(frames, (r, r), "bilinear"), "totensor", out=out)


def occlusion_boxes(n: int, hw: Tuple[int, int], coverage: float) -> torch.Tensor:
    """add_occlusion's squares (embedding_matching.py:163-193) for n frames of H x W, drawn with the global `random`
    module in the reference's order: per frame s = int(sqrt(coverage*H*W)), x = randint(0, W-s), y = randint(0, H-s).
    -> int32 [n,3] rows (x, y, s)."""
    H, W = int(hw[0]), int(hw[1])
    s = int(np.sqrt(coverage * H * W))
    rows = []
    for _ in range(int(n)):
        x = random.randint(0, W - s)
        y = random.randint(0, H - s)
        rows.append((x, y, s))
    return torch.tensor(rows, dtype=torch.int32).reshape(-1, 3)


def perturb_u8(frames: torch.Tensor, kind: str, std: float = 0.1, mean: float = 0.0, coverage: float = 0.2,
               noise: Optional[torch.Tensor] = None, boxes=None, generator: Optional[torch.Generator] = None,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ToTensor -> add_gaussian_noise / add_occlusion -> ToPILImage (embedding_matching.py:141-193, 241-248) on u8
    [N,H,W,3], u8 out, with the reference's f32 operations in its order.
      "gaussian_noise": clamp(x + (n * std + mean), 0, 1); noise = n, f32 [N,3,H,W] (randn_like of each frame's
                        [1,3,H,W] tensor); default: torch.randn on the frames' device from `generator`.
      "occlusion":      a square of 0.5 per frame; boxes = int [N,3] rows (x, y, size); default: occlusion_boxes().
    ToPILImage's mul(255).byte() truncates, so the grey square is 127."""
    _check_u8(frames)
    N, H, W, _ = frames.shape
    res = _check_out(out, (N, H, W, 3), torch.uint8, frames.device)
    if kind == "gaussian_noise":
        if noise is None:
            noise = torch.randn((N, 3, H, W), generator=generator, device=frames.device)
        if tuple(noise.shape) not in ((N, 3, H, W), (N, 1, 3, H, W)) or noise.dtype != torch.float32:
            raise ValueError(f"noise must be f32 [N,3,H,W] = {(N, 3, H, W)}, got {noise.dtype} {tuple(noise.shape)}")
        noise = noise.to(frames.device).contiguous()
        L.call("rbvae_perturb_u8", frames, res, N, H, W, PERTURB_NOISE, noise, float(std), float(mean), None)
    elif kind == "occlusion":
        if boxes is None:
            boxes = occlusion_boxes(N, (H, W), coverage)
        boxes = torch.as_tensor(np.asarray(boxes.cpu() if isinstance(boxes, torch.Tensor) else boxes), dtype=torch.int32)
        if tuple(boxes.shape) != (N, 3):
            raise ValueError(f"boxes must be [N,3] rows (x, y, size), got {tuple(boxes.shape)}")
        L.call("rbvae_perturb_u8", frames, res, N, H, W, PERTURB_OCCLUSION, None, 0.0, 0.0,
               boxes.to(frames.device).contiguous())
    else:
        raise ValueError(f"kind must be 'gaussian_noise' or 'occlusion', got {kind!r}")
    return res


def _load_one(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"))


def load_frames(frames_dir, frame_indices: Sequence[int], device="cuda", threads: int = 16) -> torch.Tensor:
    """Decode `%010d.jpg` frames with Pillow (Image.open(p).convert("RGB"), the reference's loaders) on at most 16 host
    threads -> u8 [F,H,W,3] on `device`.  The only host step of the pipeline; every frame must have the same size."""
    paths = [os.path.join(os.fspath(frames_dir), f"{int(i):010d}.jpg") for i in frame_indices]
    if not paths:
        raise ValueError("no frame indices")
    with concurrent.futures.ThreadPoolExecutor(max_workers=max(1, min(16, int(threads), len(paths)))) as ex:
        imgs = list(ex.map(_load_one, paths))
    shapes = {a.shape for a in imgs}
    if len(shapes) != 1:
        raise ValueError(f"frames of different sizes: {sorted(shapes)}")
    host = torch.from_numpy(np.stack(imgs))
    if torch.device(device).type == "cuda":
        host = host.pin_memory()
    return host.to(device, non_blocking=True)


@torch.no_grad()
def extract_embeddings(encoder, frames, frame_indices: Optional[Sequence[int]] = None, chunk: int = 16,
                       eps: Optional[torch.Tensor] = None, target=(1280, 720), sample: bool = True) -> torch.Tensor:
    """get_percep_embeddings.py:89-106 (load_img -> encode_first_stage -> get_first_stage_encoding, one frame at a time)
    as batched device work: `chunk` frames per sd_input + LDMEncoder.encode.
      frames: u8 [F,H,W,3] on the device, or a folder of `%010d.jpg` frames (read chunk by chunk with load_frames);
      frame_indices: the frame numbers of the rows (needed for a folder; default range(F));
      eps: the posterior draws f32 [F,4,h,w] (default: the encoder's host torch.randn per chunk, which is the
           reference's per-frame stream of draws).
    -> f32 [F,4,h,w] with h, w = the SD input's sides / 8; row i = frame_indices[i].  With frame_indices = range(F)
    DeviceStatePairDataset takes it as it is; to_reference_dict() writes the reference's dict."""
    from_dir = not isinstance(frames, torch.Tensor)
    if from_dir:
        if frame_indices is None:
            raise ValueError("frame_indices are needed to read frames from a folder")
        idx = [int(i) for i in frame_indices]
        F = len(idx)
    else:
        _check_u8(frames)
        F = frames.shape[0]
        if frame_indices is not None and len(frame_indices) != F:
            raise ValueError(f"{len(frame_indices)} frame indices for {F} frames")
    if F == 0:
        raise ValueError("no frames")
    chunk = max(1, int(chunk))
    w, h = sd_target(target)
    Z = encoder.cfg["embed_dim"]
    dev = frames.device if not from_dir else torch.device("cuda")
    if eps is not None and (tuple(eps.shape) != (F, Z, h // 8, w // 8)):
        raise ValueError(f"eps must be [F,{Z},{h // 8},{w // 8}], got {tuple(eps.shape)}")
    table = torch.empty((F, Z, h // 8, w // 8), dtype=torch.float32, device=dev)
    x = None
    for s in range(0, F, chunk):
        e = min(F, s + chunk)
        src = load_frames(frames, idx[s:e], device=dev) if from_dir else frames[s:e]
        if x is None or x.shape[0] != e - s:
            x = torch.empty((e - s, 3, h, w), dtype=torch.float32, device=dev)
        sd_input(src, target, out=x)
        encoder.encode(x, eps=None if eps is None else eps[s:e].to(dev), sample=sample, out=table[s:e])
    return table


def to_reference_dict(table: torch.Tensor, frame_indices: Optional[Sequence[int]] = None) -> dict:
    """The reference's embeddings dict (get_percep_embeddings.py:103-106): {"%010d.jpg": float32 [1,4,h,w]}, ready
    for np.save."""
    t = table.detach().float().cpu().numpy()
    idx = range(t.shape[0]) if frame_indices is None else frame_indices
    if len(idx) != t.shape[0]:
        raise ValueError(f"{len(idx)} frame indices for {t.shape[0]} rows")
    return {f"{int(i):010d}.jpg": t[r:r + 1].copy() for r, i in enumerate(idx)}
