"""Density clustering of the latents: how many dense islands are there, and which frames lie on the bridges between them?
DBSCAN needs no K: a row is core when at least min_samples rows (itself included) lie within eps of it, the clusters are the
connected components of the core rows, a non-core row next to a core row is a border row of that row's cluster, and every other
row is noise (-1).  The kernels (csrc/dbscan.hip) state scikit-learn 1.7.2's DBSCAN in its order-free form -- clusters numbered
by their smallest core index, a contested border row taking the lowest id -- so the labels and the core rows equal
sklearn.cluster.DBSCAN's on every row, for Euclidean distance on the soft latents and for Hamming distance on the hard codes.
  radius_graph          the neighbourhoods as a bit matrix int64 [N, W] and their sizes (rbvae_dbscan_adj / _adj_bits)
  dbscan                core rows, FastSV rounds to the components' smallest core index (rbvae_dbscan_round, the stop decided on
                        the device), labels (rbvae_dbscan_labels)
  dbscan_sweep          one graph, one fit per min_samples
  k_distances, suggest_eps      the sorted distances to the k-th neighbour (projection.knn_graph) and their knee
  noise_runs            the maximal runs of -1
  latent_density        both fits on the script's data, scored against the states and the flags
The graph is N x N bits (19 MB at N = 12298), so 2 <= N <= 65536; 1 <= L <= 128 (rbvae_dbscan_ok).  Not built: the upper
triangle alone and its mirror image, an implicit graph for larger N, OPTICS and HDBSCAN, assigning new points to a fit, sample
weights.  There is no host path: a matrix on the CPU raises.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from . import symbols
from ._latents import ENQUEUE  # noqa: F401  (the batch of run_until_done)
from ._latents import checked_matrix, encode_frames, frame_count, frame_labels, run_until_done
from .bernoulli import pack_codes
from .hmm import change_points

MAX_ROWS = 65536                                    # rbvae_dbscan_ok
MAX_KNN_ROWS = 16384                                # rbvae_knn's N, the limit of k_distances and suggest_eps
METRICS = ("euclidean", "hamming")
_LIMITS = "2 <= N <= 65536, 1 <= L <= 128"


@dataclass
class DBSCANResult:
    labels: torch.Tensor                # int32 [N] on the device: the cluster of every row, -1 for noise
    core: torch.Tensor                  # bool [N]: the core rows (sklearn's core_sample_indices_ are its nonzero positions)
    counts: torch.Tensor                # int32 [N]: |N(i)|, the row itself included
    n_clusters: int
    n_noise: int
    n_rounds: int                       # the rounds of rbvae_dbscan_round that ran, the last (which changes nothing) included
    eps: float                          # the radius (Euclidean) or the number of differing bits (Hamming)
    min_samples: int
    metric: str
    graph: Tuple[torch.Tensor, torch.Tensor]        # radius_graph's (adj, counts)


def _metric(metric):
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {METRICS}, got {metric!r}")
    return metric


def _bits_of(eps, Ld):
    if isinstance(eps, bool) or int(eps) != eps:
        raise ValueError(f"eps ({eps!r}) must be a whole number of differing bits for metric='hamming'")
    if not 0 <= int(eps) <= Ld:
        raise ValueError(f"eps ({eps}) must lie in [0, L = {Ld}] for metric='hamming'")
    return int(eps)


def _packed(X):
    """int32 [N, 4] on the device (pack_codes' words) -> (words, N, 128: the words do not say how long the code is)"""
    if not X.is_cuda:
        raise ValueError("X must be on the GPU (there is no CPU path)")
    if X.dim() != 2 or X.shape[1] != 4 or not X.is_contiguous():
        raise ValueError(f"packed codes must be a contiguous int32 [N, 4], got {tuple(X.shape)}")
    Ld = 128
    if L.query("rbvae_dbscan_ok", X.shape[0], Ld) != 1:
        raise ValueError(f"radius_graph: (N={X.shape[0]}, L={Ld}) outside {_LIMITS}")
    return X, X.shape[0], Ld


def radius_graph(X: torch.Tensor, eps, metric: str = "euclidean"):
    """The neighbourhoods N(i) = {j: d(i, j) <= eps} of the rows of a device matrix, i itself included
    -> (adj int64 [N, W] on the device, W = ceil(N / 64): bit j % 64 of word j / 64 of row i says j in N(i), the bits of columns
        >= N are zero; counts int32 [N]: |N(i)|).
    metric="euclidean": X f32 [N, L]; eps2 = float(eps) * float(eps) is computed here in f64 and the kernel compares rbvae_knn's
    f64 squared distance with it (<=, so a distance equal to eps is inside).
    metric="hamming": X is the f32 hard codes [N, L] (a value > 0.5 is a set bit) or pack_codes' int32 [N, 4]; eps is a whole
    number of differing bits, at most L (128 for packed codes).  scikit-learn's "hamming" is the share of differing positions,
    so its equivalent is eps = (bits + 0.5) / L."""
    metric = _metric(metric)
    if metric == "hamming" and isinstance(X, torch.Tensor) and X.dtype == torch.int32:
        words, N, Ld = _packed(X)
    else:
        X, N, Ld = checked_matrix(X, "radius_graph", "rbvae_dbscan_ok", _LIMITS)
        words = pack_codes(X) if metric == "hamming" else None
    W = L.query("rbvae_dbscan_words", N)
    adj = torch.empty((N, W), dtype=torch.int64, device=X.device)
    cnt = torch.empty(N, dtype=torch.int32, device=X.device)
    if metric == "hamming":
        L.call("rbvae_dbscan_adj_bits", words, N, Ld, _bits_of(eps, Ld), adj, cnt)
    else:
        eps = float(eps)
        if not eps >= 0.0:
            raise ValueError(f"eps ({eps}) must be non-negative")
        L.call("rbvae_dbscan_adj", X, N, Ld, eps * eps, adj, cnt)
    return adj, cnt


def _checked_graph(graph, N=None):
    adj, cnt = graph
    for t, dtype, name in ((adj, torch.int64, "adj"), (cnt, torch.int32, "counts")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
            raise ValueError(f"graph: {name} must be a contiguous {dtype} tensor on the GPU (radius_graph's)")
    n = cnt.shape[0]
    if adj.dim() != 2 or cnt.dim() != 1 or L.query("rbvae_dbscan_ok", n, 1) != 1 or \
            tuple(adj.shape) != (n, L.query("rbvae_dbscan_words", n)):
        raise ValueError(f"graph: adj {tuple(adj.shape)} and counts {tuple(cnt.shape)} are not radius_graph's of one matrix")
    if N is not None and n != N:
        raise ValueError(f"graph: built from {n} rows, X has {N}")
    return adj, cnt, n


def _fit(graph, eps, min_samples, metric) -> DBSCANResult:
    """the fit on a finished graph"""
    adj, cnt, N = _checked_graph(graph)
    if isinstance(min_samples, bool) or int(min_samples) != min_samples or int(min_samples) < 1:
        raise ValueError(f"min_samples ({min_samples!r}) must be a positive integer")
    m = int(min_samples)
    dev = adj.device
    W = adj.shape[1]
    core_mask = torch.empty(W, dtype=torch.int64, device=dev)
    f = [torch.empty(N, dtype=torch.int32, device=dev) for _ in range(2)]
    L.call("rbvae_dbscan_core", cnt, N, m, core_mask, f[0])
    state = torch.zeros(4, dtype=torch.int32, device=dev)

    def one_round(it):
        L.call("rbvae_dbscan_round", adj, core_mask, N, f[it & 1], f[(it + 1) & 1], state)

    # the round that changes nothing leaves both buffers equal, and the rounds enqueued behind it write nothing
    n_rounds, _, _ = run_until_done(one_round, state, N + 64)
    if not int(state[0]):
        raise RuntimeError(f"dbscan: the components did not settle in {n_rounds} rounds")
    labels = torch.empty(N, dtype=torch.int32, device=dev)
    n_clusters = torch.empty(1, dtype=torch.int32, device=dev)
    ws = torch.empty(L.query("rbvae_dbscan_ws_bytes", N) // 8, dtype=torch.int64, device=dev)
    L.call("rbvae_dbscan_labels", adj, core_mask, f[0], N, labels, n_clusters, ws)
    return DBSCANResult(labels, cnt >= m, cnt, int(n_clusters), int((labels < 0).sum()), int(n_rounds), eps, m, metric,
                        (adj, cnt))


def dbscan(X: torch.Tensor, eps, min_samples: int = 5, metric: str = "euclidean",
           graph: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> DBSCANResult:
    """sklearn.cluster.DBSCAN(eps, min_samples=min_samples, metric=metric).fit(X) on the device; the labels and the core rows
    equal scikit-learn 1.7.2's on every row (for Hamming with its eps = (bits + 0.5) / L, see radius_graph).  min_samples counts
    the row itself.  graph: radius_graph's result for the same X, eps and metric, to fit again without building it; X may then
    be None."""
    metric = _metric(metric)
    if graph is None:
        graph = radius_graph(X, eps, metric)
    elif X is not None:
        _checked_graph(graph, X.shape[0])
    return _fit(graph, eps, min_samples, metric)


def dbscan_sweep(X: torch.Tensor, eps, min_samples_list: Sequence[int], metric: str = "euclidean") -> List[DBSCANResult]:
    """One graph, one fit per entry of min_samples_list (the graph does not depend on min_samples) -> the results in the
    list's order, each equal to dbscan(X, eps, m, metric)."""
    metric = _metric(metric)
    graph = radius_graph(X, eps, metric)
    return [_fit(graph, eps, m, metric) for m in min_samples_list]


def k_distances(X: torch.Tensor, k: int) -> torch.Tensor:
    """f64 [N] on the device, ascending: every row's Euclidean distance to its k-th nearest row, the row itself counted as the
    first (as min_samples counts it): the (k - 1)-th column of projection.knn_graph(X, k - 1), k = 1 gives zeros.  Limited to
    rbvae_knn's 2 <= N <= 16384 and k - 1 <= min(N - 1, 128)."""
    from .projection import knn_graph
    k = int(k)
    if k < 1:
        raise ValueError(f"k ({k}) must be at least 1")
    X, N, _ = checked_matrix(X, "k_distances", "rbvae_dbscan_ok", _LIMITS)
    if k == 1:
        return torch.zeros(N, dtype=torch.float64, device=X.device)
    if L.query("rbvae_knn_ok", N, X.shape[1], k - 1) != 1:
        raise ValueError(f"k_distances: (N={N}, L={X.shape[1]}, k={k}) outside 2 <= N <= {MAX_KNN_ROWS}, 1 <= L <= 128, "
                         "k - 1 <= min(N - 1, 128)")
    return torch.sort(torch.sqrt(knn_graph(X, k - 1)[1][:, k - 2])).values


def knee(curve: np.ndarray) -> int:
    """the index of an ascending curve's knee: with both axes scaled to [0, 1], the point farthest from the chord between the
    curve's ends (the first of equals); 0 for a flat curve"""
    y = np.asarray(curve, dtype=np.float64)
    n = len(y)
    span = y[-1] - y[0]
    if n < 3 or not span > 0:
        return 0
    x = np.arange(n) / (n - 1.0)
    return int(np.argmax(np.abs((y - y[0]) / span - x)))       # the chord is the diagonal: the distance is |y - x| / sqrt(2)


def suggest_eps(X: torch.Tensor, k: int = 5) -> float:
    """The k-distance heuristic: the value of k_distances(X, k) at its knee (computed on the host).  Limits as k_distances."""
    curve = k_distances(X, k).cpu().numpy()
    return float(curve[knee(curve)])


def noise_runs(labels) -> List[Tuple[int, int]]:
    """the maximal runs of -1 in a label vector (host or device) as (start, stop) pairs, stop exclusive"""
    lab = labels.cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)
    noise = np.concatenate(([False], lab == -1, [False]))
    edges = np.flatnonzero(noise[1:] != noise[:-1])
    return [(int(a), int(b)) for a, b in zip(edges[0::2], edges[1::2])]


def _density_scores(fit: DBSCANResult, states: np.ndarray, S: int, tolerance: int) -> dict:
    from .segments import boundary_agreement
    lab = fit.labels.cpu().numpy()
    keep = lab >= 0
    true_cps = change_points(states)
    noise = np.flatnonzero(~keep)
    cps = np.asarray(true_cps, dtype=np.int64)
    near = int((np.abs(noise[:, None] - cps[None, :]).min(axis=1) <= tolerance).sum()) if len(noise) and len(cps) else 0
    runs = noise_runs(lab)
    agreement = (symbols.clustering_agreement(states[keep], lab[keep].astype(np.int64), S, max(fit.n_clusters, 1))
                 if keep.any() else None)
    return {"fit": fit, "agreement": agreement, "noise_fraction": float(len(noise)) / len(lab),
            "noise_near_change": near / len(noise) if len(noise) else float("nan"), "noise_runs": runs,
            "boundaries": boundary_agreement([(a + b) // 2 for a, b in runs], true_cps, tolerance)}


@torch.no_grad()
def latent_density(model, x: torch.Tensor, frame_indices: Sequence[int], flags: Sequence[int], eps: Optional[float] = None,
                   code_bits: Optional[int] = None, min_samples: int = 5, tolerance: int = 2,
                   projections: Optional[dict] = None, temperature: float = 0.2, noise_ratio: float = 0.3, u=None) -> dict:
    """Both density fits of the script's data in one call: x [F, C, H, W] frames (or latents) on the device in time order,
    encoded by _latents.encode_frames (projections["latents"] serves as the soft latents when present); the states are
    data.assign_label(frame_indices[f], flags).  The soft latents are fitted with Euclidean distance (eps=None:
    suggest_eps(latents, min_samples)), the hard codes with Hamming distance (code_bits=None: 1 bit).
    -> {"latents", "codes", "labels" (the states), "eps", "code_bits", "soft": {...}, "hard": {...}}, each of the two with
       "fit": DBSCANResult, "agreement": clustering_agreement of the non-noise frames against the states (None when every frame
       is noise), "noise_fraction", "noise_near_change": the share of noise frames within `tolerance` of a position where the
       state changes (NaN without noise), "noise_runs", "boundaries": segments.boundary_agreement of the noise runs' midpoints
       against hmm.change_points(labels), at `tolerance`}"""
    labels = frame_labels(frame_indices, flags, frame_count(x))
    S = len(flags) + 1
    z, codes = encode_frames(model, x, hard=True, latents=projections.get("latents") if projections is not None else None,
                             temperature=temperature, noise_ratio=noise_ratio, u=u)
    eps = suggest_eps(z, min_samples) if eps is None else float(eps)
    bits = 1 if code_bits is None else int(code_bits)
    soft = dbscan(z, eps, min_samples)
    hard = dbscan(codes, bits, min_samples, metric="hamming")
    return {"latents": z, "codes": codes, "labels": labels, "eps": eps, "code_bits": bits,
            "soft": _density_scores(soft, labels, S, tolerance), "hard": _density_scores(hard, labels, S, tolerance)}
