"""State boundaries without the labels: given the per-frame latents of a video in frame order, where do the states
change?  The answer is the optimal partition of the N rows into K contiguous segments with the least within-segment sum
of squared deviations, found exactly by the dynamic programme over (segments, end row) on the device (csrc/segment.hip);
on hard 0/1 codes a segment's cost is its summed per-bit variance times its length, so one kernel segments soft latents
and codes.
  segment_prefix        P [N + 1, L] and Q [N + 1]: the running sums of the rows and of their squared norms
  segment_layer         one layer: out[t] = min over s <= t - min_size of prev[s] + cost(s, t), and its argmin
  segment_table         the K layers and the traced boundaries of the best k-segmentation for every k <= K
  segment               the segmentation with n_segments segments, or the k <= max_segments that minimises
                        cost_k + penalty k
  boundary_agreement    precision, recall and F1 of predicted against true boundaries within a tolerance (host)
  latent_segments       all of it for the script's data, scored against the hand-annotated transition flags
A boundary is the position of the first row of a new segment.  cost(s, t) = (Q[t] - Q[s]) - |P[t] - P[s]|^2 / (t - s); the
header include/rbvae_hip.h has the full definition.  There is no host path: X on the CPU raises.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from ._latents import checked_matrix, encode_frames, frame_count, frame_labels
from .symbols import clustering_agreement

MAX_SEGMENTS = 256                                  # rbvae_segment_ok


@dataclass
class SegmentTable:
    P: torch.Tensor                 # f64 [N + 1, L] on the device
    Q: torch.Tensor                 # f64 [N + 1] on the device
    cost: torch.Tensor              # f64 [K, N + 1] on the device: D_k[t]
    arg: torch.Tensor               # int32 [K, N + 1] on the device
    cuts: np.ndarray                # int32 [K, K] on the host: row k - 1 = the k - 1 boundaries ascending, then -1
    costs: np.ndarray               # f64 [K] on the host: cost[:, N]
    min_size: int


@dataclass
class SegmentResult:
    boundaries: np.ndarray          # int64 [n_segments - 1]: the first row of every segment but the first
    labels: torch.Tensor            # int32 [N] on the device: the segment index of every row
    n_segments: int
    cost: float                     # costs[n_segments - 1]
    costs: np.ndarray               # f64 [K]: the best cost for every k <= K (+inf where there is no k-segmentation)
    table: SegmentTable


def _checked(X, K, min_size, what):
    return checked_matrix(X, what, "rbvae_segment_ok", f"2 <= N <= 65536, 1 <= L <= 128, 1 <= K <= {MAX_SEGMENTS}, "
                          f"min_size >= 1, K min_size <= N", K=K, min_size=min_size)


def _workspace(N, Ld, device):
    return torch.empty(L.query("rbvae_segment_ws_bytes", N, Ld) // 8, dtype=torch.float64, device=device)


def segment_prefix(X: torch.Tensor):
    """-> (P f64 [N + 1, L], Q f64 [N + 1]) on the device for an f32 device matrix X [N, L] with rows in time order"""
    X, N, Ld, _, _ = _checked(X, 1, 1, "segment_prefix")
    P = torch.empty((N + 1, Ld), dtype=torch.float64, device=X.device)
    Q = torch.empty(N + 1, dtype=torch.float64, device=X.device)
    L.call("rbvae_segment_prefix", X, N, Ld, P, Q)
    return P, Q


def _prefix_pair(P, Q):
    for t, name in ((P, "P"), (Q, "Q")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f"{name} must be on the GPU (there is no CPU path)")
        if t.dtype != torch.float64 or not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous float64, got {t.dtype}")
    if P.dim() != 2 or Q.dim() != 1 or P.shape[0] != Q.shape[0]:
        raise ValueError(f"P must be [N + 1, L] and Q [N + 1], got {tuple(P.shape)} and {tuple(Q.shape)}")
    return P.shape[0] - 1, P.shape[1]


def segment_layer(P: torch.Tensor, Q: torch.Tensor, prev: torch.Tensor, min_size: int = 1):
    """One layer of the table from segment_prefix's sums -> (out f64 [N + 1], arg int32 [N + 1]) on the device: the
    smallest prev[s] + cost(s, t) over 0 <= s <= t - min_size with prev[s] finite in the order (value, s), and its s;
    (+inf, -1) where no candidate exists."""
    N, Ld = _prefix_pair(P, Q)
    m = int(min_size)
    if L.query("rbvae_segment_ok", N, Ld, 1, m) != 1:
        raise ValueError(f"segment_layer: (N={N}, L={Ld}, min_size={m}) outside 2 <= N <= 65536, 1 <= L <= 128, "
                         f"1 <= min_size <= N")
    if not isinstance(prev, torch.Tensor) or not prev.is_cuda or prev.dtype != torch.float64 or tuple(prev.shape) != (N + 1,):
        raise ValueError(f"prev must be {N + 1} float64 values on the GPU")
    out = torch.empty(N + 1, dtype=torch.float64, device=P.device)
    arg = torch.empty(N + 1, dtype=torch.int32, device=P.device)
    L.call("rbvae_segment_layer", P, Q, N, Ld, prev.contiguous(), m, out, arg, _workspace(N, Ld, P.device))
    return out, arg


def segment_table(X: torch.Tensor, max_segments: int, min_size: int = 1) -> SegmentTable:
    """The table D_1 = layer([0, +inf, ...]), D_k = layer(D_{k - 1}) for k <= K = max_segments, traced on the device for
    every k; only the boundaries and the K costs D_k[N] come to the host."""
    X, N, Ld, K, m = _checked(X, max_segments, min_size, "segment_table")
    dev = X.device
    P = torch.empty((N + 1, Ld), dtype=torch.float64, device=dev)
    Q = torch.empty(N + 1, dtype=torch.float64, device=dev)
    L.call("rbvae_segment_prefix", X, N, Ld, P, Q)
    cost = torch.empty((K, N + 1), dtype=torch.float64, device=dev)
    arg = torch.empty((K, N + 1), dtype=torch.int32, device=dev)
    cuts = torch.empty((K, K), dtype=torch.int32, device=dev)
    ws = _workspace(N, Ld, dev)
    prev = torch.full((N + 1,), float("inf"), dtype=torch.float64, device=dev)
    prev[0] = 0.0
    for k in range(K):
        L.call("rbvae_segment_layer", P, Q, N, Ld, prev, m, cost[k], arg[k], ws)
        prev = cost[k]
    L.call("rbvae_segment_trace", arg, N, K, cost, cuts)
    return SegmentTable(P, Q, cost, arg, cuts.cpu().numpy(), cost[:, N].cpu().numpy(), m)


def _choose(costs: np.ndarray, penalty: float) -> int:
    """the k >= 1 that minimises costs[k - 1] + penalty k; a tie goes to the smaller k"""
    best, bk = math.inf, 0
    for k in range(1, len(costs) + 1):
        v = float(costs[k - 1]) + penalty * k
        if v < best:
            best, bk = v, k
    if bk == 0:
        raise ValueError("no segmentation has a finite cost")
    return bk


def segment(X: torch.Tensor, n_segments: Optional[int] = None, max_segments: Optional[int] = None,
            penalty: Optional[float] = None, min_size: int = 1) -> SegmentResult:
    """The least-squares segmentation of the rows of X.  With n_segments: that many segments (the table is built up to
    max_segments when given, so `costs` holds the whole curve).  With penalty: the k <= max_segments that minimises
    costs[k - 1] + penalty k, a tie going to the smaller k.  With neither: ValueError."""
    if n_segments is None and penalty is None:
        raise ValueError("give n_segments, or penalty with max_segments")
    if n_segments is None and max_segments is None:
        raise ValueError("penalty needs max_segments")
    if n_segments is not None and penalty is not None:
        raise ValueError("give n_segments or penalty, not both")
    K = int(max_segments) if max_segments is not None else int(n_segments)
    if n_segments is not None and not 1 <= int(n_segments) <= K:
        raise ValueError(f"n_segments ({n_segments}) must be between 1 and max_segments ({K})")
    if penalty is not None and not float(penalty) >= 0.0:
        raise ValueError(f"penalty ({penalty}) must be non-negative")
    table = segment_table(X, K, min_size)
    k = int(n_segments) if n_segments is not None else _choose(table.costs, float(penalty))
    if not np.isfinite(table.costs[k - 1]):
        raise ValueError(f"there is no segmentation into {k} segments of at least {table.min_size} rows")
    bounds = table.cuts[k - 1, :k - 1].astype(np.int64)
    N = X.shape[0]
    labels = torch.zeros(N, dtype=torch.int32, device=X.device)
    if k > 1:
        labels[torch.from_numpy(bounds).to(X.device)] = 1
        labels = torch.cumsum(labels, 0, dtype=torch.int32)
    return SegmentResult(bounds, labels, k, float(table.costs[k - 1]), table.costs, table)


def boundary_agreement(pred: Sequence[int], true: Sequence[int], tolerance: int = 0) -> dict:
    """Predicted against true boundaries, both sorted positions, matched one to one by the two-pointer walk: where
    |p_i - t_j| <= tolerance the two are matched and both advance, otherwise the smaller advances.
    -> {"precision": matched / len(pred), "recall": matched / len(true), "f1", "n_matched", "mean_abs_offset" (NaN when
    nothing matches)}.  Two empty lists score 1.0 on all three, exactly one empty list 0.0."""
    p, t = [int(v) for v in pred], [int(v) for v in true]
    tol = int(tolerance)
    if tol < 0:
        raise ValueError(f"tolerance ({tolerance}) must be non-negative")
    if any(b < a for a, b in zip(p, p[1:])) or any(b < a for a, b in zip(t, t[1:])):
        raise ValueError("boundaries must be sorted")
    i = j = matched = 0
    offset = 0
    while i < len(p) and j < len(t):
        if abs(p[i] - t[j]) <= tol:
            matched += 1
            offset += abs(p[i] - t[j])
            i += 1
            j += 1
        elif p[i] < t[j]:
            i += 1
        else:
            j += 1
    if not p and not t:
        precision = recall = f1 = 1.0
    elif not p or not t:
        precision = recall = f1 = 0.0
    else:
        precision, recall = matched / len(p), matched / len(t)
        f1 = 2.0 * precision * recall / (precision + recall) if matched else 0.0
    return {"precision": precision, "recall": recall, "f1": f1, "n_matched": matched,
            "mean_abs_offset": offset / matched if matched else float("nan")}


@torch.no_grad()
def latent_segments(model, x: torch.Tensor, frame_indices: Sequence[int], flags: Sequence[int],
                    n_segments: Optional[int] = None, tolerance: int = 2, temperature: float = 0.2, noise_ratio: float = 0.3,
                    u=None, min_size: int = 1) -> dict:
    """The recovered state boundaries of the script's data in one call: x [F, C, H, W] frames (or latents) on the device in
    frame order, encoded by _latents.encode_frames (the same uniforms u [F, L] for the soft and the hard pass); the states
    are data.assign_label(frame_indices[f], flags) and the true boundaries the positions where the state changes;
    n_segments defaults to the number of true segments.  The default tolerance of 2 is the reference's grey_out = 1 frame on
    either side of a flag, plus the flag itself.
    -> {"latents", "codes", "labels" (the states), "true_boundaries", "true_frames", "n_segments", and for each of "soft" and
        "hard" a dict {"segments": SegmentResult, "boundaries" (positions), "frames" (frame_indices[pos]),
        "boundary_agreement" against the true boundaries, "label_agreement": clustering_agreement of the segment labels
        against the states}}"""
    F = frame_count(x)
    frames = np.array([int(f) for f in frame_indices], dtype=np.int64)      # indexed by boundary positions below
    labels = frame_labels(frames, flags, F)
    true = np.nonzero(labels[1:] != labels[:-1])[0].astype(np.int64) + 1
    K = len(true) + 1 if n_segments is None else int(n_segments)
    z, codes = encode_frames(model, x, hard=True, temperature=temperature, noise_ratio=noise_ratio, u=u)
    out = {"latents": z, "codes": codes, "labels": labels, "true_boundaries": true, "true_frames": frames[true], "n_segments": K}
    S = len(flags) + 1
    for name, rows in (("soft", z), ("hard", codes)):
        seg = segment(rows, n_segments=K, min_size=min_size)
        out[name] = {"segments": seg, "boundaries": seg.boundaries, "frames": frames[seg.boundaries],
                     "boundary_agreement": boundary_agreement(seg.boundaries, true, tolerance),
                     "label_agreement": clustering_agreement(labels, seg.labels, S, K)}
    return out
