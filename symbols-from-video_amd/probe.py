"""Linear probe evaluation (the reference's scripts/evaluation/linear_projection_eval/linear_regression_eval.py:97-151):
embed frames, fit a multi-output least-squares map from the embedding (L <= 128 values) to the flattened frame
(3 x r x r targets) on a random 80 % of the frames and report R^2, MSE, MAE and explained variance on the rest.

The reference hands f32 frames to scikit-learn on the host.  Here the targets stay on the device as the u8 frames the
resize wrote (a quarter of the bytes) and the arithmetic is f64 (csrc/probe.hip):
  split        train_test_split(test_size, random_state): n_test = ceil(test_size N), perm = RandomState(seed)
               .permutation(N), test = perm[:n_test], train = perm[n_test:]                              (host)
  fit factor   Xc = X[train] - mean_x = U S V^T; singular values <= rcond s_max are dropped (rcond defaults to
               max(n_train, L) 2^-52); A = V S^+ U^T is the minimum-norm least-squares operator.  The columns of Xc
               sum to zero, so A 1 = 0 and W = A Y[train] needs no centring of Y.  B = [A^T | 1 / n_train]    (host, tiny)
  pass 1       C [L + 1][P] = B^T (Y[train] - y0) on the f64 matrix cores, y0 = the first train row; rows 0..L-1 are W,
               row L the shifted target mean; intercept = (C[L] - sum_l mean_x[l] C[l]) + y0
  pass 2       over the test rows, per target: sum e, sum e^2, sum |e| (e = y - (intercept + x W)) and sum d, sum d^2
               (d = y - y[test[0]])
  finish       r2 = 1 - sum e^2 / SStot, SStot = sum d^2 - (sum d)^2 / m; evs = 1 - (sum e^2 / m - (sum e / m)^2) /
               (SStot / m); a zero denominator scores 1 with a zero numerator and 0 otherwise (scikit-learn's
               force_finite); r2, evs = uniform means over the targets, mse, mae = means over rows and targets
The shifts by a data row are exact in f64, so a target that is constant over all rows scores exactly 1.0 (W = 0, zero
residuals, SStot == 0); scikit-learn's answer for such a column depends on rounding.
There is no host path: targets on the CPU raise.
"""
from __future__ import annotations

import dataclasses
import math
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib as L

MAX_L = 128
Y_U8, Y_F32 = 0, 1                       # RBVAE_PROBE_U8 / RBVAE_PROBE_F32


def split_indices(n: int, test_size: float = 0.2, seed: int = 42) -> Tuple[np.ndarray, np.ndarray]:
    """sklearn.model_selection.train_test_split(test_size=, random_state=) as index arrays, in its order
    (linear_regression_eval.py:117-119).  -> (train, test) int64."""
    n = int(n)
    n_test = int(math.ceil(test_size * n))
    if n < 2 or n_test < 1 or n_test >= n:
        raise ValueError(f"test_size {test_size} of {n} rows leaves an empty train or test set")
    perm = np.random.RandomState(seed).permutation(n)
    return perm[n_test:].astype(np.int64), perm[:n_test].astype(np.int64)


def fit_factor(X_train, rcond: Optional[float] = None) -> Tuple[np.ndarray, np.ndarray]:
    """The factor of LinearRegression().fit (linear_regression_eval.py:123-126) that does not depend on the targets.
    X_train [n, L] -> (B f64 [n, L + 1], mean_x f64 [L]): with Y the train targets, (B^T Y)[:L] = coef_^T and
    (B^T Y)[L] = the target mean; intercept_ = mean_y - mean_x . coef_^T."""
    X = np.asarray(X_train, dtype=np.float64)
    if X.ndim != 2 or X.shape[0] < 1 or not 1 <= X.shape[1] <= MAX_L:
        raise ValueError(f"X_train must be [n >= 1, 1 <= L <= {MAX_L}], got {X.shape}")
    n, Ld = X.shape
    mean_x = X.mean(axis=0)
    U, s, Vt = np.linalg.svd(X - mean_x, full_matrices=False)
    if rcond is None:
        rcond = max(n, Ld) * 2.0 ** -52
    keep = s > rcond * (s[0] if s.size else 0.0)
    sinv = np.zeros_like(s)
    sinv[keep] = 1.0 / s[keep]
    At = (U * sinv) @ Vt                                    # A^T = U S^+ V^T, [n, L]
    B = np.empty((n, Ld + 1), dtype=np.float64)
    B[:, :Ld] = At
    B[:, Ld] = 1.0 / n
    return B, mean_x


@dataclasses.dataclass
class ProbeResult:
    """linear_regression_eval.py:135-159.  coef [P, L] and intercept [P] are model.coef_ / model.intercept_; they and
    the per-target scores are f64 device tensors in the reference's flatten order (CHW for frame targets)."""
    r2: float
    mse: float
    mae: float
    evs: float
    n_train: int
    n_test: int
    n_constant_targets: int
    r2_per_target: torch.Tensor
    evs_per_target: torch.Tensor
    coef: torch.Tensor
    intercept: torch.Tensor
    train_idx: np.ndarray
    test_idx: np.ndarray

    def metrics(self) -> dict:
        return {"r2": self.r2, "mse": self.mse, "mae": self.mae, "evs": self.evs}


def _targets(Y):
    """-> (flat [N, P] view, dtype code, NHWC shape or None)"""
    if not isinstance(Y, torch.Tensor):
        raise ValueError(f"Y must be a torch tensor on the GPU, got {type(Y).__name__}")
    if not Y.is_cuda:
        raise ValueError("Y must be on the GPU (there is no CPU path)")
    if not Y.is_contiguous():
        raise ValueError("Y must be contiguous")
    if Y.dtype == torch.uint8 and Y.dim() == 4 and Y.shape[3] == 3:
        nhwc = tuple(Y.shape[1:])
    elif Y.dtype in (torch.uint8, torch.float32) and Y.dim() == 2:
        nhwc = None
    else:
        raise ValueError(f"Y must be u8 [N,H,W,3], u8 [N,P] or f32 [N,P], got {Y.dtype} {tuple(Y.shape)}")
    flat = Y.view(Y.shape[0], -1)
    if flat.shape[0] < 2 or flat.shape[1] < 1:
        raise ValueError(f"Y is empty: {tuple(Y.shape)}")
    return flat, (Y_U8 if Y.dtype == torch.uint8 else Y_F32), nhwc


def _to_reference_order(t, nhwc):
    """[..., P] in memory (NHWC) order -> CHW flatten order, P last"""
    if nhwc is None:
        return t
    H, W, C = nhwc
    lead = t.shape[:-1]
    return t.reshape(*lead, H, W, C).movedim(-1, -3).reshape(*lead, H * W * C)


def _rows(idx, device):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(idx, dtype=np.int32))).to(device)


def probe_xty(Y: torch.Tensor, rows: torch.Tensor, B: torch.Tensor, row0: int, out: Optional[torch.Tensor] = None):
    """rbvae_probe_xty: C [M, P] = B^T (Y[rows] - Y[row0]) in f64.  Y as linear_probe's, rows int32 [n] and B f64
    [n, M] on the device; targets in memory order."""
    flat, code, _ = _targets(Y)
    N, P = flat.shape
    n, M = B.shape
    if rows.dtype != torch.int32 or rows.numel() != n or B.dtype != torch.float64 or not B.is_contiguous():
        raise ValueError("rows must be int32 [n] and B a contiguous f64 [n, M]")
    C = torch.empty((M, P), dtype=torch.float64, device=Y.device) if out is None else out
    nbytes = L.query("rbvae_probe_xty_ws_bytes", n, M, P)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=Y.device) if nbytes else None
    L.call("rbvae_probe_xty", code, flat, N, P, rows, n, int(row0), B, M, C, ws)
    return C


class _Passes:
    """device time of each pass (ms) into a dict, when one is given"""

    def __init__(self, sink):
        self.sink, self.marks = sink, []

    def mark(self, name):
        if self.sink is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self.marks.append((name, ev))

    def close(self):
        if self.sink is not None:
            torch.cuda.synchronize()
            for (_, a), (name, b) in zip(self.marks, self.marks[1:]):
                self.sink[name] = a.elapsed_time(b)


def linear_probe(X, Y: torch.Tensor, test_size: float = 0.2, random_state: int = 42, rcond: Optional[float] = None,
                 train_idx=None, test_idx=None, timings: Optional[dict] = None) -> ProbeResult:
    """linear_regression_eval.py:114-144 on device-resident targets.
      X: embeddings [N, L] (tensor or array; the fit factor is host f64), L <= 128;
      Y: u8 [N,H,W,3] frames (target = ToTensor's v / 255, coef / intercept returned in CHW flatten order) or u8 / f32
         [N, P], on the GPU;
      train_idx / test_idx: explicit row lists instead of the split (any order);
      timings: a dict that receives the device milliseconds of "xty" (pass 1), "intercept", "residual" (pass 2) and
         "finish"."""
    flat, code, nhwc = _targets(Y)
    N, P = flat.shape
    Xh = X.detach().cpu().numpy() if isinstance(X, torch.Tensor) else np.asarray(X)
    Xh = Xh.astype(np.float64)
    if Xh.ndim != 2 or Xh.shape[0] != N or not 1 <= Xh.shape[1] <= MAX_L:
        raise ValueError(f"X must be [N = {N}, 1 <= L <= {MAX_L}], got {Xh.shape}")
    Ld = Xh.shape[1]
    if (train_idx is None) != (test_idx is None):
        raise ValueError("give both train_idx and test_idx, or neither")
    if train_idx is None:
        train, test = split_indices(N, test_size, random_state)
    else:
        train, test = np.asarray(train_idx, dtype=np.int64), np.asarray(test_idx, dtype=np.int64)
        for name, idx in (("train_idx", train), ("test_idx", test)):
            if idx.ndim != 1 or idx.size < 1 or idx.min() < 0 or idx.max() >= N:
                raise ValueError(f"{name} must be a non-empty list of rows in [0, {N})")
    dev = Y.device
    B, mean_x = fit_factor(Xh[train], rcond)
    Bd, mx = torch.from_numpy(B).to(dev), torch.from_numpy(mean_x).to(dev)
    Xr = torch.from_numpy(np.ascontiguousarray(Xh[test])).to(dev)
    rtr, rte = _rows(train, dev), _rows(test, dev)
    n_tr, m = int(train.size), int(test.size)

    t = _Passes(timings)
    t.mark("start")
    C = probe_xty(Y, rtr, Bd, int(train[0]))
    t.mark("xty")
    icpt = torch.empty(P, dtype=torch.float64, device=dev)
    L.call("rbvae_probe_intercept", code, flat, N, P, int(train[0]), C, mx, Ld, icpt)
    t.mark("intercept")
    sums = torch.empty((5, P), dtype=torch.float64, device=dev)
    L.call("rbvae_probe_residual_sums", code, flat, N, P, rte, m, int(test[0]), Xr, C, icpt, Ld, sums)
    t.mark("residual")
    r2 = torch.empty(P, dtype=torch.float64, device=dev)
    evs = torch.empty(P, dtype=torch.float64, device=dev)
    part = torch.empty(L.query("rbvae_probe_finish_parts", P) * 5, dtype=torch.float64, device=dev)
    met = torch.empty(4, dtype=torch.float64, device=dev)
    ncon = torch.empty(1, dtype=torch.int32, device=dev)
    L.call("rbvae_probe_finish", sums, P, m, r2, evs, part, met, ncon)
    t.mark("finish")
    t.close()
    mh = met.cpu().numpy()
    return ProbeResult(r2=float(mh[0]), mse=float(mh[1]), mae=float(mh[2]), evs=float(mh[3]), n_train=n_tr, n_test=m,
                       n_constant_targets=int(ncon.item()), r2_per_target=_to_reference_order(r2, nhwc),
                       evs_per_target=_to_reference_order(evs, nhwc),
                       coef=_to_reference_order(C[:Ld], nhwc).t(), intercept=_to_reference_order(icpt, nhwc),
                       train_idx=train, test_idx=test)


@torch.no_grad()
def frame_embeddings(model, frames: torch.Tensor, resolution: int = 256, temperature: float = 0.5,
                     embedding: str = "h", batch: int = 64, ldm_encoder=None, u=None, eps=None,
                     noise_ratio: float = 0.1, target=(1280, 720)) -> Tuple[torch.Tensor, torch.Tensor]:
    """The script's embedding loop (linear_regression_eval.py:97-112) over u8 frames [F,H,W,3] on the device, `batch`
    frames per step, one sequence of length 1 per frame:
      targets   resize_u8(frames, (resolution,) * 2, "bilinear"): ImageTransforms' Resize, kept as u8 [F,r,r,3];
      inputs    u8_to_input(targets, "totensor") (contrastive model), or, with ldm_encoder, the perceptual path of
                robustness.state_codes_under: sd_input(frames, target) -> LDM encode;
      embedding "h": h_seq of model(x, temperature=temperature), the script's choice; "z": the hard codes of
                model.encode(x, temperature, hard=True).
    u [F, L] binarisation uniforms and eps [F,4,h,w] posterior draws default to the host draws of the callees.
    -> (embeddings f32 [F, L], targets u8 [F,r,r,3]), both on the device."""
    from .frames import _check_u8, resize_u8, sd_input, u8_to_input
    _check_u8(frames)
    if embedding not in ("h", "z"):
        raise ValueError(f"embedding must be 'h' or 'z', got {embedding!r}")
    F, r, Ld = frames.shape[0], int(resolution), model.latent_dim
    if u is not None and tuple(u.shape) != (F, Ld):
        raise ValueError(f"u must have shape {(F, Ld)}, got {tuple(u.shape)}")
    was_training = model.training
    model.eval()
    targets = torch.empty((F, r, r, 3), dtype=torch.uint8, device=frames.device)
    emb = torch.empty((F, Ld), dtype=torch.float32, device=frames.device)
    batch = max(1, int(batch))
    try:
        for s in range(0, F, batch):
            e = min(F, s + batch)
            resize_u8(frames[s:e], (r, r), "bilinear", out=targets[s:e])
            if ldm_encoder is not None:
                ep = None if eps is None else eps[s:e].to(frames.device)
                x = ldm_encoder.encode(sd_input(frames[s:e], target), eps=ep)[:, None]
            else:
                x = u8_to_input(targets[s:e], "totensor")[:, None]
            ub = None if u is None else u[s:e].to(frames.device)
            if embedding == "h":
                _, h_seq, _ = model(x, temperature=temperature, noise_ratio=noise_ratio, u=ub)
                emb[s:e] = h_seq.reshape(e - s, Ld)
            else:
                emb[s:e] = model.encode(x, temperature=temperature, hard=True, noise_ratio=noise_ratio, u=ub)[:, 0]
    finally:
        model.train(was_training)
    return emb, targets


def frame_probe(model, frames_u8: torch.Tensor, resolution: int = 256, temperature: float = 0.5, embedding: str = "h",
                batch: int = 64, ldm_encoder=None, u=None, eps=None, noise_ratio: float = 0.1, target=(1280, 720),
                **probe_kw) -> ProbeResult:
    """linear_regression_eval.py:97-151 on raw u8 frames [F,H,W,3] on the device: frame_embeddings, then linear_probe
    of the embeddings against the resident resized u8 frames (probe_kw: test_size, random_state, rcond, train_idx,
    test_idx, timings)."""
    emb, targets = frame_embeddings(model, frames_u8, resolution, temperature, embedding, batch, ldm_encoder, u, eps,
                                    noise_ratio, target)
    return linear_probe(emb, targets, **probe_kw)
