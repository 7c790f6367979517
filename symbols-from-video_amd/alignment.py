"""Two videos aligned: given the per-frame latents of two recordings in frame order, which frame of A corresponds to which
frame of B?  Dynamic time warping with the steps {diagonal, up, left} on the device (csrc/dtw.hip): the table is filled tile by
tile, one launch per anti-diagonal of tiles, and traced on the device; only the path comes to the host.
  dtw_fill            the directions and the last row of the table (and the whole table when asked)
  dtw_trace           the path, its cost and its ends from the directions
  dtw                 both -> DTWResult
  warp_map            for every row of Y the first and last aligned row of X, and the reverse (host)
  transfer_labels     A's labels carried along the path to B's rows by majority (host)
  latent_alignment    all of it for the script's data: both videos encoded, aligned on soft latents and on hard codes, A's
                      states transferred to B and scored against B's own
metric "sqeuclidean" and "euclidean" take f32 rows, "hamming" 0/1 f32 codes (packed by bernoulli.pack_codes).  window is a
Sakoe-Chiba band |i - j| <= window; subsequence=True finds the clip X inside the longer Y (open ends on Y).  The header
include/rbvae_hip.h has the full definition, the tie order included.  There is no host path: X or Y on the CPU raises.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from ._latents import device_matrix, encode_frames, frame_count, frame_labels, require_finite
from .bernoulli import pack_codes
from .segments import boundary_agreement
from .symbols import clustering_agreement

METRICS = {"sqeuclidean": 0, "euclidean": 1, "hamming": 2}
LIMITS = "1 <= N, M <= 16384, 1 <= L <= 128, window None or |N - M| <= window without subsequence"


@dataclass
class DTWTable:
    dirs: torch.Tensor              # uint8 [N, ceil(M / 4)] on the device: 2 bits per cell
    last_row: torch.Tensor          # f64 [M] on the device: D[N - 1][.]
    table: Optional[torch.Tensor]   # f64 [N, M] on the device, or None
    N: int
    M: int
    subsequence: bool


@dataclass
class DTWResult:
    cost: float                     # D at the end cell
    path: np.ndarray                # int64 [path_len, 2] on the host: the pairs (i, j) ascending
    path_len: int
    normalized_cost: float          # cost / path_len
    start: int                      # the first aligned row of Y (0 without subsequence)
    end: int                        # the last aligned row of Y (M - 1 without subsequence)
    last_row: torch.Tensor          # f64 [M] on the device
    table: Optional[torch.Tensor]   # f64 [N, M] on the device with return_table, else None


def _checked_pair(X, Y, metric, window, subsequence, what):
    if metric not in METRICS:
        raise ValueError(f"{what}: metric must be one of {sorted(METRICS)}, got {metric!r}")
    X, Y = device_matrix(X, "X"), device_matrix(Y, "Y")
    if X.device != Y.device:
        raise ValueError(f"{what}: X is on {X.device} and Y on {Y.device}")
    (N, Ld), (M, Ly) = X.shape, Y.shape
    if Ld != Ly:
        raise ValueError(f"{what}: X has L={Ld} columns and Y has L={Ly}")
    if window is not None and int(window) < 0:
        raise ValueError(f"{what}: window ({window}) must be None or non-negative")
    w = -1 if window is None else min(int(window), 1 << 30)
    sub = 1 if subsequence else 0
    if L.query("rbvae_dtw_ok", N, M, Ld, METRICS[metric], w, sub) != 1:
        raise ValueError(f"{what}: (N={N}, M={M}, L={Ld}, window={window}, subsequence={bool(subsequence)}) outside {LIMITS}")
    require_finite(X)
    require_finite(Y)
    return X, Y, N, M, Ld, w, sub


def dtw_fill(X: torch.Tensor, Y: torch.Tensor, *, metric: str = "sqeuclidean", window: Optional[int] = None,
             subsequence: bool = False, return_table: bool = False) -> DTWTable:
    """The table of X [N, L] against Y [M, L] (f32 on the device, rows in time order) -> DTWTable; the N x M doubles are
    stored only with return_table."""
    X, Y, N, M, Ld, w, sub = _checked_pair(X, Y, metric, window, subsequence, "dtw_fill")
    dev = X.device
    dirs = torch.empty((N, (M + 3) // 4), dtype=torch.uint8, device=dev)
    last_row = torch.empty(M, dtype=torch.float64, device=dev)
    table = torch.empty((N, M), dtype=torch.float64, device=dev) if return_table else None
    ws = torch.empty(L.query("rbvae_dtw_ws_bytes", N, M) // 8, dtype=torch.float64, device=dev)
    if metric == "hamming":
        L.call("rbvae_dtw_fill_bits", pack_codes(X), N, pack_codes(Y), M, Ld, w, sub, dirs, last_row, table, ws)
    else:
        L.call("rbvae_dtw_fill", X, N, Y, M, Ld, METRICS[metric], w, sub, dirs, last_row, table, ws)
    return DTWTable(dirs, last_row, table, N, M, bool(sub))


def dtw_trace(t: DTWTable) -> DTWResult:
    """The path of a filled table, walked on the device from the end cell -> DTWResult"""
    dev = t.dirs.device
    path = torch.empty((t.N + t.M - 1, 2), dtype=torch.int32, device=dev)
    state = torch.empty(3, dtype=torch.int32, device=dev)
    cost = torch.empty(1, dtype=torch.float64, device=dev)
    L.call("rbvae_dtw_trace", t.dirs, t.last_row, t.N, t.M, int(t.subsequence), path, state, cost)
    n, start, end = state.cpu().tolist()
    if n < 1:
        raise RuntimeError("dtw_trace: the directions do not lead from the end cell to the first row")
    c = float(cost.cpu()[0])
    return DTWResult(c, path[:n].cpu().numpy().astype(np.int64), n, c / n, start, end, t.last_row, t.table)


def dtw(X: torch.Tensor, Y: torch.Tensor, *, metric: str = "sqeuclidean", window: Optional[int] = None,
        subsequence: bool = False, return_table: bool = False) -> DTWResult:
    """The cheapest warping path between the rows of X and of Y, both in time order.  A tie between predecessors goes to the
    diagonal, then to (i - 1, j), then to (i, j - 1); in subsequence mode the end is the lowest j among the smallest
    D[N - 1][j]."""
    return dtw_trace(dtw_fill(X, Y, metric=metric, window=window, subsequence=subsequence, return_table=return_table))


def _checked_path(path, N=None, M=None):
    p = np.asarray(path)
    if p.ndim != 2 or p.shape[1] != 2 or p.shape[0] < 1:
        raise ValueError(f"path must be [len, 2] with len >= 1, got {p.shape}")
    p = p.astype(np.int64)
    if np.any(np.diff(p, axis=0) < 0) or p.min() < 0:
        raise ValueError("path must be non-negative and ascending in both columns")
    if (N is not None and p[:, 0].max() >= N) or (M is not None and p[:, 1].max() >= M):
        raise ValueError(f"path leaves the {N} x {M} table")
    return p


def warp_map(path, N: int, M: int) -> dict:
    """-> {"first_i", "last_i": int64 [M], the first and last row of X aligned with every row of Y (-1 where none is, which
    happens only outside [start, end] in subsequence mode); "first_j", "last_j": int64 [N], the reverse}"""
    p = _checked_path(path, N, M)
    out = {}
    for name, col, other, n in (("i", 1, 0, M), ("j", 0, 1, N)):
        first, last = np.full(n, -1, dtype=np.int64), np.full(n, -1, dtype=np.int64)
        last[p[:, col]] = p[:, other]                       # ascending: the last write is the largest
        first[p[::-1, col]] = p[::-1, other]
        out["first_" + name], out["last_" + name] = first, last
    return out


def transfer_labels(path, labels_a, M: int) -> np.ndarray:
    """Row j of Y takes the most frequent labels_a[i] among the rows i of X aligned with it, the smallest label on a tie;
    rows of Y that the path does not visit (outside [start, end] in subsequence mode) get -1.  -> int64 [M]"""
    la = np.asarray(labels_a.cpu() if isinstance(labels_a, torch.Tensor) else labels_a).astype(np.int64)
    if la.ndim != 1 or la.size < 1 or la.min() < 0:
        raise ValueError("labels_a must be a vector of non-negative labels")
    p = _checked_path(path, la.size, M)
    K = int(la.max()) + 1
    votes = np.zeros((M, K), dtype=np.int64)
    np.add.at(votes, (p[:, 1], la[p[:, 0]]), 1)
    out = votes.argmax(axis=1).astype(np.int64)             # the first maximum: the smallest label
    out[votes.sum(axis=1) == 0] = -1
    return out


@torch.no_grad()
def latent_alignment(model, x_a: torch.Tensor, x_b: torch.Tensor, frame_indices_a: Sequence[int], flags_a: Sequence[int],
                     frame_indices_b: Sequence[int], flags_b: Sequence[int], *, latents_a=None, latents_b=None,
                     window: Optional[int] = None, tolerance: int = 2, temperature: float = 0.2, noise_ratio: float = 0.3,
                     u_a=None, u_b=None) -> dict:
    """Two recordings of one task aligned in one call: x_a [Fa, C, H, W] and x_b [Fb, C, H, W] frames (or latents) on the
    device in frame order, each encoded by _latents.encode_frames with its own uniforms (u_a [Fa, L], u_b [Fb, L]; without
    them two independent host draws); the states are data.assign_label(frame_indices[f], flags) per video.  The soft latents
    are aligned under "sqeuclidean" and the hard codes under "hamming"; A's states are carried to B along each path
    (transfer_labels) and scored against B's own states.
    -> {"latents_a", "codes_a", "latents_b", "codes_b", "labels_a", "labels_b", "true_boundaries_b", and for each of "soft" and
        "hard" a dict {"dtw": DTWResult, "warp": warp_map, "labels": the transferred states int64 [Fb], "accuracy": the share
        of B's frames whose transferred state is their own, "label_agreement": clustering_agreement against B's states,
        "boundaries": the positions where the transferred state changes, "boundary_agreement" against B's own}}"""
    Fa, Fb = frame_count(x_a), frame_count(x_b)
    la, lb = frame_labels(frame_indices_a, flags_a, Fa), frame_labels(frame_indices_b, flags_b, Fb)
    kw = dict(hard=True, temperature=temperature, noise_ratio=noise_ratio)
    za, ca = encode_frames(model, x_a, latents=latents_a, u=u_a, **kw)
    zb, cb = encode_frames(model, x_b, latents=latents_b, u=u_b, **kw)
    true_b = np.nonzero(lb[1:] != lb[:-1])[0].astype(np.int64) + 1
    out = {"latents_a": za, "codes_a": ca, "latents_b": zb, "codes_b": cb, "labels_a": la, "labels_b": lb,
           "true_boundaries_b": true_b}
    S = max(len(flags_a), len(flags_b)) + 1
    for name, a, b, metric in (("soft", za, zb, "sqeuclidean"), ("hard", ca, cb, "hamming")):
        res = dtw(a, b, metric=metric, window=window)
        got = transfer_labels(res.path, la, Fb)
        bounds = np.nonzero(got[1:] != got[:-1])[0].astype(np.int64) + 1
        out[name] = {"dtw": res, "warp": warp_map(res.path, Fa, Fb), "labels": got, "accuracy": float((got == lb).mean()),
                     "label_agreement": clustering_agreement(lb, torch.from_numpy(got).to(za.device), S, S),
                     "boundaries": bounds, "boundary_agreement": boundary_agreement(bounds, true_b, tolerance)}
    return out
