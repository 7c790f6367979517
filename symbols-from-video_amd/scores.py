"""Latent scores: what the reference's scripts/evaluation/clustering_eval/embedding_umap.py leaves to a look at its scatter
plots, as numbers, on the device (csrc/scores.hip), as scikit-learn 1.7.2 computes them:
  neighbour_ranks       rbvae_nbr_ranks: where row i's neighbours in one space stand among its neighbours in another
  trustworthiness       sklearn.manifold.trustworthiness(X, Y, n_neighbors): the ranks in X of knn_graph(Y, k)'s neighbours
  continuity            the same with the roles swapped: the ranks in the map of the neighbours in X
  label_distance_sums   rbvae_label_dist_sums / rbvae_label_hamming_sums: per row and state, the sum of its distances to the
                        state's rows
  silhouette_samples    sklearn.metrics.silhouette_samples from those sums (Euclidean on the soft latents, Hamming on the
  silhouette_score      hard codes), finished on the host in f64
  knn_label_agreement   knn_graph plus a gather: the share of a row's neighbours with its label, and the leave-one-out vote
                        KNeighborsClassifier would cast on kneighbors() of its own training set
  latent_scores         all of them for the script's data: the soft latents and hard codes of the frames, their labels, and
                        the maps of projection.latent_projections
d2 is rbvae_knn's (f64, one device function), so ranks and neighbours can never disagree about an order; ties go to the
lower index, where scikit-learn's argsort leaves them undefined.  There is no host path: inputs on the CPU raise.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from ._latents import device_matrix as _device_matrix
from ._latents import encode_frames, frame_count, frame_labels, require_finite
from .projection import knn_graph

MAX_STATES = 256                                    # rbvae_label_sums_ok


def neighbour_ranks(X: torch.Tensor, nbr: torch.Tensor):
    """rbvae_nbr_ranks: X f32 [N, L], nbr int32 [N, k] on the device -> (rank int32 [N, k], excess int32 [N]);
    rank[i, r] = the 1-based position of nbr[i, r] among the other rows of X by (d2, index), -1 for an entry that is no
    other row; excess[i] = sum_r max(0, rank[i, r] - k)."""
    X = _device_matrix(X, "X")
    nbr = _device_matrix(nbr, "nbr", torch.int32)
    N, Ld = X.shape
    if nbr.shape[0] != N:
        raise ValueError(f"nbr has {nbr.shape[0]} rows, X {N}")
    require_finite(X)
    k = nbr.shape[1]
    rank = torch.empty((N, k), dtype=torch.int32, device=X.device)
    excess = torch.empty(N, dtype=torch.int32, device=X.device)
    L.call("rbvae_nbr_ranks", X, N, Ld, nbr, k, rank, excess)
    return rank, excess


def trustworthiness(X: torch.Tensor, Y: torch.Tensor, n_neighbors: int = 5) -> float:
    """sklearn.manifold.trustworthiness(X, Y, n_neighbors=k) for f32 device matrices X [N, L] and Y [N, M]:
    1 - 2 sum_i excess_i / (N k (2N - 3k - 1)), the ranks taken in X for the k nearest neighbours in Y; the sum of the
    excesses is exact (a Python int)."""
    X, Y = _device_matrix(X, "X"), _device_matrix(Y, "Y")
    N, k = X.shape[0], int(n_neighbors)
    if Y.shape[0] != N:
        raise ValueError(f"X has {N} rows, Y {Y.shape[0]}")
    if k < 1 or k >= N / 2:
        raise ValueError(f"n_neighbors ({k}) should be at least 1 and less than n_samples / 2 ({N / 2})")
    idx, _ = knn_graph(Y, k)
    _, excess = neighbour_ranks(X, idx)
    t = int(excess.cpu().numpy().astype(np.int64).sum())
    return 1.0 - t * (2.0 / (N * k * (2.0 * N - 3.0 * k - 1.0)))


def continuity(X: torch.Tensor, Y: torch.Tensor, n_neighbors: int = 5) -> float:
    """trustworthiness with the roles swapped: how far the k nearest neighbours in X stand from each other in the map Y"""
    return trustworthiness(Y, X, n_neighbors)


def _host_labels(labels, N, n_states):
    if isinstance(labels, torch.Tensor):
        labels = labels.cpu().numpy()
    lab = np.asarray(labels)
    if lab.ndim != 1 or len(lab) != N or not np.issubdtype(lab.dtype, np.integer):
        raise ValueError(f"labels must be {N} integers, got {lab.dtype} {lab.shape}")
    lab = lab.astype(np.int64)
    S = int(lab.max()) + 1 if n_states is None else int(n_states)
    if lab.min() < 0 or lab.max() >= S:
        raise ValueError(f"labels outside [0, {S})")
    return lab, S


def label_distance_sums(X: torch.Tensor, labels, n_states: Optional[int] = None, metric: str = "euclidean") -> torch.Tensor:
    """sums [N, S] on the device: sums[i, s] = the sum over the rows j of state s (ascending) of the distance of rows i and
    j.  metric "euclidean": sqrt(d2) in f64 -> f64; "hamming": the number of differing bits of the codes X > 0.5 -> int32
    (not divided by L).  labels: N integers in [0, n_states), on the host or the device."""
    X = _device_matrix(X, "X")
    N, Ld = X.shape
    if metric not in ("euclidean", "hamming"):
        raise ValueError(f"metric must be 'euclidean' or 'hamming', got {metric!r}")
    lab, S = _host_labels(labels, N, n_states)
    require_finite(X)
    order = np.argsort(lab, kind="stable").astype(np.int32)
    seg = np.concatenate([[0], np.cumsum(np.bincount(lab, minlength=S))]).astype(np.int32)
    order_d, seg_d = torch.from_numpy(order).to(X.device), torch.from_numpy(seg).to(X.device)
    if metric == "euclidean":
        sums = torch.empty((N, S), dtype=torch.float64, device=X.device)
        L.call("rbvae_label_dist_sums", X, N, Ld, order_d, seg_d, S, sums)
    else:
        sums = torch.empty((N, S), dtype=torch.int32, device=X.device)
        L.call("rbvae_label_hamming_sums", X, N, Ld, order_d, seg_d, S, sums)
    return sums


def silhouette_samples(X: torch.Tensor, labels, n_states: Optional[int] = None, metric: str = "euclidean") -> np.ndarray:
    """sklearn.metrics.silhouette_samples(X, labels, metric=metric) -> f64 [N] on the host, from label_distance_sums:
    a = the mean distance to the other rows of the row's state, b = the smallest mean distance to another non-empty state,
    s = (b - a) / max(a, b); 0 where a = b = 0 and for a row alone in its state.  The number of non-empty states must be in
    2..N - 1."""
    N = _device_matrix(X, "X").shape[0]
    sums = label_distance_sums(X, labels, n_states, metric).cpu().numpy().astype(np.float64)
    lab, S = _host_labels(labels, N, n_states)
    freq = np.bincount(lab, minlength=S)
    filled = int((freq > 0).sum())
    if not 1 < filled < N:
        raise ValueError(f"Number of labels is {filled}. Valid values are 2 to n_samples - 1 (inclusive)")
    rows = np.arange(N)
    with np.errstate(divide="ignore", invalid="ignore"):
        a = sums[rows, lab] / (freq[lab] - 1)
        other = sums / freq[None, :]
        other[rows, lab] = np.inf
        other[:, freq == 0] = np.inf
        b = other.min(axis=1)
        s = (b - a) / np.maximum(a, b)
    s[freq[lab] == 1] = 0.0
    return np.nan_to_num(s)


def silhouette_score(X: torch.Tensor, labels, n_states: Optional[int] = None, metric: str = "euclidean") -> float:
    """sklearn.metrics.silhouette_score: the mean of silhouette_samples"""
    return float(np.mean(silhouette_samples(X, labels, n_states, metric)))


def knn_label_agreement(X: torch.Tensor, labels, k: int, n_states: Optional[int] = None) -> dict:
    """The labels of knn_graph(X, k)'s neighbours, gathered on the device.  -> {"purity": the mean share of a row's k
    neighbours that carry its label, "predictions": int64 [N] on the host, the label with the most votes among the k
    neighbours (the row itself excluded, ties to the smallest label: KNeighborsClassifier(k) on kneighbors() of its own
    training set), "accuracy": the share of rows predicted as labelled}"""
    X = _device_matrix(X, "X")
    N = X.shape[0]
    lab, S = _host_labels(labels, N, n_states)
    idx, _ = knn_graph(X, int(k))
    lab_d = torch.from_numpy(lab).to(X.device)
    nl = lab_d[idx.long()]                                              # [N, k]
    purity = int((nl == lab_d[:, None]).sum()) / (N * int(k))
    votes = torch.zeros((N, S), dtype=torch.int32, device=X.device)
    votes.scatter_add_(1, nl, torch.ones_like(nl, dtype=torch.int32))   # integer adds: any order gives the same counts
    states = torch.arange(S, device=X.device)[None, :]
    pred = torch.where(votes == votes.max(dim=1, keepdim=True).values, states, S).min(dim=1).values
    return {"purity": purity, "predictions": pred.cpu().numpy().astype(np.int64),
            "accuracy": int((pred == lab_d).sum()) / N}


@torch.no_grad()
def latent_scores(model, x: torch.Tensor, frame_indices: Sequence[int], flags: Sequence[int],
                  projections: Optional[dict] = None, n_neighbors: int = 24, temperature: float = 0.2,
                  noise_ratio: float = 0.3, u=None) -> dict:
    """The scores of the script's data in one call: x [F, C, H, W] frames (or latents) on the device, one sequence of
    length 1 per frame.  _latents.encode_frames encodes them: the soft latents
    (model.encode(..., temperature, hard=False, noise_ratio); projections["latents"] is used instead when present), the
    hard codes from the same uniforms with hard=True (embedding_hamming_distance.py:180); the labels are
    data.assign_label(frame_indices[f], flags).  u [F, L]: the binarisation uniforms instead of the host draw.
    -> {"latents" f32 [F, L], "codes" f32 [F, L], "labels" int64 array, "silhouette" (soft latents, Euclidean),
        "silhouette_hamming" (hard codes), "knn_purity", "knn_accuracy" (soft latents, k = n_neighbors)} and, when
    `projections` (latent_projections' dict) is given, "trustworthiness_pca", "continuity_pca", "trustworthiness_tsne" and
    "continuity_tsne" of its maps at n_neighbors, and "trustworthiness_umap" and "continuity_umap" when it holds "umap"."""
    labels = frame_labels(frame_indices, flags, frame_count(x))
    S = len(flags) + 1
    z, codes = encode_frames(model, x, hard=True, latents=projections.get("latents") if projections is not None else None,
                             temperature=temperature, noise_ratio=noise_ratio, u=u)
    agree = knn_label_agreement(z, labels, n_neighbors, S)
    out = {"latents": z, "codes": codes, "labels": labels,
           "silhouette": silhouette_score(z, labels, S), "silhouette_hamming": silhouette_score(codes, labels, S, "hamming"),
           "knn_purity": agree["purity"], "knn_accuracy": agree["accuracy"]}
    if projections is not None:
        for name in ("pca", "tsne") + (("umap",) if "umap" in projections else ()):
            Y = projections[name].embedding.float().contiguous()
            out[f"trustworthiness_{name}"] = trustworthiness(z, Y, n_neighbors)
            out[f"continuity_{name}"] = continuity(z, Y, n_neighbors)
    return out
