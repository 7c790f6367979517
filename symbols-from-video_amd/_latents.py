"""What the latent analyses (projection, scores, symbols, segments, spectral, mixture, hmm) share on the host: the checks
of a device matrix, the way the script's frames become labels, soft latents and hard codes, and the driver of an
iteration whose stopping rule is decided on the device.  One definition each, so a fix reaches every latent_* function.
  device_matrix, require_finite, finite_device_matrix, checked_matrix     the input checks and their messages
  frame_count, frame_labels, encode_frames                                x [F, C, H, W] -> F, the states, (latents, codes)
  run_until_done                                                          enqueue ENQUEUE iterations, read the state once
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L

ENQUEUE = 8                                         # iterations enqueued between two reads of the state


def device_matrix(X, name, dtype=torch.float32):
    if not isinstance(X, torch.Tensor):
        raise ValueError(f"{name} must be a torch tensor on the GPU, got {type(X).__name__}")
    if not X.is_cuda:
        raise ValueError(f"{name} must be on the GPU (there is no CPU path)")
    if X.dim() != 2 or X.dtype != dtype:
        raise ValueError(f"{name} must be a 2-D {dtype} tensor, got {X.dtype} {tuple(X.shape)}")
    if not X.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return X


def require_finite(X):
    if not bool(torch.isfinite(X).all()):
        raise ValueError("X holds NaN or infinite values")
    return X


def finite_device_matrix(X):
    return require_finite(device_matrix(X, "X"))


def checked_matrix(X, what, ok, limits, **sizes):
    """X as a finite f32 device matrix whose (N, L, *sizes) the library's query `ok` accepts -> (X, N, L, *sizes as ints);
    otherwise "what: (N=.., L=.., K=..) outside <limits>" """
    X = device_matrix(X, "X")
    N, Ld = X.shape
    sizes = {k: int(v) for k, v in sizes.items()}
    if L.query(ok, N, Ld, *sizes.values()) != 1:
        given = "".join(f", {k}={v}" for k, v in sizes.items())
        raise ValueError(f"{what}: (N={N}, L={Ld}{given}) outside {limits}")
    return (require_finite(X), N, Ld, *sizes.values())


def frame_count(x) -> int:
    """F of the frames x [F, C, H, W] on the device"""
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise ValueError("x must be on the GPU (there is no CPU path)")
    if x.dim() != 4:
        raise ValueError(f"x must be [F, C, H, W], got {tuple(x.shape)}")
    return x.shape[0]


def frame_labels(frame_indices, flags, F: int) -> np.ndarray:
    """the states of F frames: data.assign_label(frame_indices[f], flags) -> int64 [F] on the host"""
    from .data import assign_label
    if len(frame_indices) != F:
        raise ValueError(f"{len(frame_indices)} frame indices for {F} frames")
    return np.array([assign_label(int(f), flags) for f in frame_indices], dtype=np.int64)


def encode_frames(model, x, *, hard, latents=None, temperature=0.2, noise_ratio=0.3, u=None):
    """The frames x [F, C, H, W] as one sequence of length 1 each -> (soft latents f32 [F, L], hard codes f32 [F, L] or None
    without `hard`).  The soft pass is model.encode(..., hard=False) unless `latents` is given; the hard pass uses the same
    binarisation uniforms u [F, L].  Without u they are the host draw torch.rand((F, L)) that encode() itself would make,
    drawn once whenever a pass runs.  The model encodes in eval mode and leaves in the mode it came in."""
    if latents is not None and not hard:
        return latents.float().contiguous(), None
    if u is None:
        u = torch.rand((x.shape[0], model.latent_dim))
    kw = dict(temperature=temperature, noise_ratio=noise_ratio, u=u.to(x.device))
    z, codes = latents, None
    was_training = model.training
    model.eval()
    try:
        if z is None:
            z = model.encode(x[:, None], hard=False, **kw)[:, 0]
        if hard:
            codes = model.encode(x[:, None], hard=True, **kw)[:, 0].float().contiguous()
    finally:
        model.train(was_training)
    return z.float().contiguous(), codes


def run_until_done(enqueue_one, state, max_iter, enqueue=ENQUEUE, also_stop=None):
    """The iterations of a fit whose kernels decide on the device and return at once behind the decision: enqueue_one(it)
    is called for it = 0, 1, ... in batches of `enqueue` (never beyond max_iter), then state int32 [>= 3] = {done, n_iter,
    why, ...} is read once and, after it, also_stop() asked.  -> (n_iter, why, stopped): stopped says that also_stop ended
    the loop, which it does ahead of done."""
    it = 0
    while True:
        for _ in range(min(enqueue, max_iter - it)):
            enqueue_one(it)
            it += 1
        done, n_iter, why = state.cpu().tolist()[:3]
        if also_stop is not None and also_stop():
            return n_iter, why, True
        if done or it >= max_iter:
            return n_iter, why, False
