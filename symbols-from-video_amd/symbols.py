"""Unsupervised symbols: do the latents fall into the states by themselves?  The soft latents are clustered with k-means
on the device (csrc/kmeans.hip) as scikit-learn 1.7.2's KMeans(n_init=1, algorithm="lloyd") clusters them, every distinct
hard code is taken as a symbol, and either labelling is scored against the hand-labelled states:
  kmeans_plusplus       sklearn.cluster.kmeans_plusplus's indices: its RandomState draws on the host, the trials'
                        distances, minima and potentials on the device (rbvae_kmeans_pp_trials)
  kmeans                Lloyd's iterations (rbvae_kmeans_assign / _update / _decide), enqueued eight at a time: the
                        decision is taken on the device after every iteration and later launches return at once
  code_symbols          np.unique(codes > 0.5, axis=0, return_inverse=True, return_counts=True) on the device
  contingency           the integer table of two labellings, on the device
  clustering_agreement  ARI, NMI, homogeneity, completeness, V-measure and Fowlkes-Mallows from that table, finished on the
                        host with sklearn.metrics' formulas
  davies_bouldin, calinski_harabasz    sklearn.metrics' indices from the update kernel's centroids, counts, within and spread
  latent_symbols        all of them for the script's data
An empty cluster keeps its centre (scikit-learn moves it to the row farthest from its centre); KMeansResult.n_empty says
how many the fit ended with.  n_init other than 1, sample weights and Elkan's variant are not built.  There is no host
path: matrices (X, codes, frames) and contingency's vectors on the CPU raise.  The one exception is label vectors given to
clustering_agreement, cluster_sums and the two indices: as in scores.py they may be host integers (the states come from
data.assign_label as a numpy array) and are copied to the device, where the table and the sums are computed.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence, Union

import numpy as np
import torch

from . import _lib as L
from ._latents import ENQUEUE  # noqa: F401  (the batch of run_until_done)
from ._latents import checked_matrix, encode_frames, frame_count, frame_labels, run_until_done
from ._latents import device_matrix as _device_matrix

MAX_CLUSTERS = 256                                  # rbvae_kmeans_ok
WHY = {1: "strict", 2: "tol", 3: "max_iter"}


@dataclass
class KMeansResult:
    labels: torch.Tensor            # int32 [N] on the device
    centers: torch.Tensor           # f64 [K, L] on the device
    inertia: float                  # sum_k within_k, k ascending, from the final assignment
    n_iter: int
    converged: str                  # "strict" (no label moved), "tol" (the centres' shift), "max_iter"
    counts: np.ndarray              # int64 [K]
    n_empty: int


def _checked(X, K, what):
    return checked_matrix(X, what, "rbvae_kmeans_ok", f"1 <= L <= 128, 1 <= K <= {MAX_CLUSTERS}, K <= N <= 1048576", K=K)


def _workspace(N, Ld, K, device):
    return torch.empty(L.query("rbvae_kmeans_ws_bytes", N, Ld, K) // 8, dtype=torch.float64, device=device)


def _pp_candidates(closest: np.ndarray, vals: np.ndarray) -> np.ndarray:
    """_kmeans_plusplus' candidate rows: searchsorted(stable_cumsum(closest), vals), clipped to N - 1 (a value above the
    last cumulative sum, which rounding allows, would otherwise name row N)"""
    return np.minimum(np.searchsorted(np.cumsum(closest), vals), len(closest) - 1)


def kmeans_plusplus(X: torch.Tensor, n_clusters: int, seed: int = 42) -> np.ndarray:
    """sklearn.cluster.kmeans_plusplus(X, n_clusters, random_state=seed)'s indices -> int64 [K] on the host.  The draws are
    scikit-learn's: choice(N, p = 1 / N) for the first centre, then per centre T = 2 + int(ln K) candidates at
    searchsorted(cumsum(closest), uniform(size=T) * potential) clipped to N - 1, of which the one with the lowest potential
    wins.  The device takes min(closest, d2(., X[candidate])) and its sum for all T at once; the host reads back the T
    potentials and the winner's N minima."""
    X, N, Ld, K = _checked(X, n_clusters, "kmeans_plusplus")
    rs = np.random.RandomState(seed)
    T = 2 + int(math.log(K))
    dev = X.device
    ws = _workspace(N, Ld, K, dev)
    out = torch.empty((T, N), dtype=torch.float64, device=dev)
    pot_d = torch.empty(T, dtype=torch.float64, device=dev)
    idx = np.full(K, -1, dtype=np.int64)
    idx[0] = rs.choice(N, p=np.ones(N) / np.ones(N).sum())
    closest_d = torch.full((N,), float("inf"), dtype=torch.float64, device=dev)
    L.call("rbvae_kmeans_pp_trials", X, N, Ld, torch.tensor([int(idx[0])], dtype=torch.int32, device=dev), 1, closest_d,
           out, pot_d, ws)
    closest_d = out[0].clone()
    closest, pot = closest_d.cpu().numpy(), float(pot_d[0])
    for c in range(1, K):
        vals = rs.uniform(size=T) * pot
        cand = _pp_candidates(closest, vals)
        L.call("rbvae_kmeans_pp_trials", X, N, Ld, torch.from_numpy(cand.astype(np.int32)).to(dev), T, closest_d, out,
               pot_d, ws)
        pots = pot_d.cpu().numpy()
        best = int(np.argmin(pots))
        closest_d = out[best].clone()
        closest, pot, idx[c] = closest_d.cpu().numpy(), float(pots[best]), cand[best]
    return idx


def kmeans(X: torch.Tensor, n_clusters: int, init: Union[str, torch.Tensor, np.ndarray] = "k-means++", max_iter: int = 300,
           tol: float = 1e-4, seed: int = 42) -> KMeansResult:
    """KMeans(n_clusters, init=init, n_init=1, algorithm="lloyd", max_iter=max_iter, tol=tol, random_state=seed).fit(X)
    for an f32 device matrix X [N, L].  init: "k-means++" or the K initial centres [K, L].  An iteration assigns every
    row to its nearest centre (ties to the lower one), moves the centres to their clusters' means and then decides on the
    device: no label moved -> "strict"; else sum_k |shift_k|^2 <= tol * mean_l var_l(X) -> "tol"; else n_iter = max_iter ->
    "max_iter".  Unless the fit ended strictly the labels are taken again from the final centres.  Iterations are enqueued
    ENQUEUE at a time and the state is read once per batch; launches behind the decision return at once, so the result
    is that of a check after every iteration."""
    X, N, Ld, K = _checked(X, n_clusters, "kmeans")
    dev = X.device
    max_iter = int(max_iter)
    if max_iter < 1 or not tol >= 0:
        raise ValueError(f"max_iter ({max_iter}) must be at least 1 and tol ({tol}) non-negative")
    if isinstance(init, str):
        if init != "k-means++":
            raise ValueError(f"init must be 'k-means++' or the initial centres, got {init!r}")
        C = X[torch.from_numpy(kmeans_plusplus(X, K, seed)).to(dev)].double().contiguous()
    else:
        C = torch.as_tensor(init).to(device=dev, dtype=torch.float64).contiguous().clone()
        if tuple(C.shape) != (K, Ld) or not bool(torch.isfinite(C).all()):
            raise ValueError(f"init must be {K} x {Ld} finite centres, got {tuple(C.shape)}")
    tol_abs = float(X.double().var(dim=0, unbiased=False).mean()) * float(tol)
    state = torch.zeros(4, dtype=torch.int32, device=dev)
    lab = [torch.full((N,), -1, dtype=torch.int32, device=dev) for _ in range(2)]
    d2 = torch.empty(N, dtype=torch.float64, device=dev)
    count = torch.empty(K, dtype=torch.int32, device=dev)
    shift2, within, spread = (torch.empty(K, dtype=torch.float64, device=dev) for _ in range(3))
    ws = _workspace(N, Ld, K, dev)

    def iteration(it):
        L.call("rbvae_kmeans_assign", X, N, Ld, C, K, lab[(it + 1) & 1], None, lab[it & 1], d2, state)
        L.call("rbvae_kmeans_update", X, N, Ld, lab[it & 1], d2, K, C, count, shift2, within, spread, ws, state)
        L.call("rbvae_kmeans_decide", shift2, K, tol_abs, max_iter, state)

    n_iter, why, _ = run_until_done(iteration, state, max_iter)
    # scikit-learn's trailing E-step; after a strict stop the centres did not move and it repeats the last assignment
    labels = torch.empty(N, dtype=torch.int32, device=dev)
    L.call("rbvae_kmeans_assign", X, N, Ld, C, K, None, None, labels, d2, None)
    L.call("rbvae_kmeans_update", X, N, Ld, labels, d2, K, C.clone(), count, shift2, within, spread, ws, None)
    counts = count.cpu().numpy().astype(np.int64)
    inertia = 0.0
    for w in within.cpu().tolist():
        inertia += w
    return KMeansResult(labels, C, inertia, int(n_iter), WHY[why], counts, int((counts == 0).sum()))


def code_symbols(codes: torch.Tensor):
    """np.unique(codes > 0.5, axis=0, return_inverse=True, return_counts=True) on the device -> (symbols int64 [N]: the
    index of each row's code among the distinct ones, codes_unique bool [U, L] in lexicographic order with element 0 most
    significant, counts int64 [U])"""
    codes = _device_matrix(codes, "codes")
    uniq, inv, cnt = torch.unique((codes > 0.5).to(torch.uint8), dim=0, sorted=True, return_inverse=True, return_counts=True)
    return inv.reshape(-1).long(), uniq.bool(), cnt.long()


def _device_labels(a, name, device=None):
    if isinstance(a, torch.Tensor):
        t = a
    else:
        t = torch.from_numpy(np.ascontiguousarray(a))
    if t.dim() != 1 or t.dtype not in (torch.int32, torch.int64, torch.int16, torch.uint8, torch.int8):
        raise ValueError(f"{name} must be a vector of integers, got {t.dtype} {tuple(t.shape)}")
    return t.to(device if device is not None else "cuda").long()


def contingency(a: torch.Tensor, b: torch.Tensor, A: int, B: int) -> torch.Tensor:
    """int64 [A, B] on the device: the number of rows with a = i and b = j, for integer device vectors a in [0, A) and b in
    [0, B).  Integer adds: any order gives the same counts."""
    for t, name in ((a, "a"), (b, "b")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f"{name} must be on the GPU (there is no CPU path)")
    a, b = _device_labels(a, "a", a.device), _device_labels(b, "b", a.device)
    A, B = int(A), int(B)
    if a.shape != b.shape:
        raise ValueError(f"a has {a.shape[0]} rows, b {b.shape[0]}")
    if a.numel() and (int(a.min()) < 0 or int(a.max()) >= A or int(b.min()) < 0 or int(b.max()) >= B):
        raise ValueError(f"labels outside [0, {A}) x [0, {B})")
    table = torch.zeros(A * B, dtype=torch.int64, device=a.device)
    table.scatter_add_(0, a * B + b, torch.ones_like(a))
    return table.view(A, B)


def _entropy(n: np.ndarray) -> float:
    """sklearn.metrics.cluster.entropy from the labels' counts"""
    n = n[n > 0].astype(np.float64)
    if n.size == 1:
        return 0.0
    total = np.sum(n)
    return float(-np.sum((n / total) * (np.log(n) - math.log(total))))


def _mutual_info(table: np.ndarray) -> float:
    """sklearn.metrics.mutual_info_score(None, None, contingency=table), the empty rows and columns dropped"""
    table = table[table.sum(1) > 0][:, table.sum(0) > 0]
    pi, pj = table.sum(1), table.sum(0)
    if pi.size == 1 or pj.size == 1:
        return 0.0
    nzx, nzy = np.nonzero(table)
    nz = table[nzx, nzy].astype(np.float64)
    total = float(table.sum())
    outer = pi.take(nzx).astype(np.int64) * pj.take(nzy).astype(np.int64)
    log_outer = -np.log(outer) + math.log(pi.sum()) + math.log(pj.sum())
    mi = nz / total * (np.log(nz) - math.log(total)) + nz / total * log_outer
    mi = np.where(np.abs(mi) < np.finfo(np.float64).eps, 0.0, mi)
    return float(np.clip(mi.sum(), 0.0, None))


def clustering_agreement(a, b, A: Optional[int] = None, B: Optional[int] = None) -> dict:
    """sklearn.metrics' scores of the labelling b against the true labelling a (integer vectors on the host or the device):
    {"ari": adjusted_rand_score, "nmi": normalized_mutual_info_score (arithmetic mean), "homogeneity", "completeness",
    "v_measure", "fowlkes_mallows", "contingency": int64 [A, B] on the host}.  The table is counted on the device; the pair
    counts are Python integers and the entropies follow scikit-learn's formulas and its values for single-cluster
    inputs."""
    dev = next((t.device for t in (a, b) if isinstance(t, torch.Tensor) and t.is_cuda), None)
    a, b = _device_labels(a, "a", dev), _device_labels(b, "b", dev)
    A = int(a.max()) + 1 if A is None else int(A)
    B = int(b.max()) + 1 if B is None else int(B)
    T = contingency(a, b, A, B).cpu().numpy()
    n = int(T.sum())
    rows, cols = [int(v) for v in T.sum(1)], [int(v) for v in T.sum(0)]
    squares = sum(int(v) * int(v) for v in T.reshape(-1))
    tp = squares - n
    fp = sum(v * v for v in cols) - squares
    fn = sum(v * v for v in rows) - squares
    tn = n * n - fp - fn - squares
    ari = 1.0 if fn == 0 and fp == 0 else 2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))
    h_a, h_b = _entropy(T.sum(1)), _entropy(T.sum(0))
    mi = _mutual_info(T)
    hom = mi / h_a if h_a else 1.0
    com = mi / h_b if h_b else 1.0
    v = 0.0 if hom + com == 0.0 else 2.0 * hom * com / (hom + com)
    n_a, n_b = sum(1 for r in rows if r), sum(1 for c in cols if c)
    if n_a == n_b == 1 or n_a == n_b == 0:
        nmi = 1.0
    elif mi == 0:
        nmi = 0.0
    else:
        nmi = float(mi / np.mean([h_a, h_b]))
    pk, qk = sum(v_ * v_ for v_ in cols) - n, sum(v_ * v_ for v_ in rows) - n
    fmi = float(np.sqrt(tp / pk) * np.sqrt(tp / qk)) if tp != 0 else 0.0
    return {"ari": float(ari), "nmi": nmi, "homogeneity": float(hom), "completeness": float(com), "v_measure": float(v),
            "fowlkes_mallows": fmi, "contingency": T}


def cluster_sums(X: torch.Tensor, labels):
    """The per-cluster sums both indices start from, for the non-empty labels in ascending order: one rbvae_kmeans_update
    from the labels (centroids and counts), one distance pass of each row to its own centroid (rbvae_kmeans_assign with
    `own`), and the update's within = sum d2 and spread = sum sqrt(d2) of that pass.
    -> (centroids f64 [K, L], counts int64 [K], within f64 [K], spread f64 [K]) on the host"""
    X = _device_matrix(X, "X")
    N, Ld = X.shape
    lab = _device_labels(labels, "labels", X.device)
    if lab.shape[0] != N:
        raise ValueError(f"labels must be {N} integers, got {tuple(lab.shape)}")
    dense = torch.unique(lab, return_inverse=True)[1].to(torch.int32).contiguous()
    K = int(dense.max()) + 1
    if not 1 < K < N:
        raise ValueError(f"Number of labels is {K}. Valid values are 2 to n_samples - 1 (inclusive)")
    X, N, Ld, K = _checked(X, K, "cluster_sums")
    dev = X.device
    C = torch.zeros((K, Ld), dtype=torch.float64, device=dev)
    count = torch.empty(K, dtype=torch.int32, device=dev)
    shift2, within, spread = (torch.empty(K, dtype=torch.float64, device=dev) for _ in range(3))
    d2 = torch.empty(N, dtype=torch.float64, device=dev)
    own = torch.empty(N, dtype=torch.int32, device=dev)
    ws = _workspace(N, Ld, K, dev)
    L.call("rbvae_kmeans_update", X, N, Ld, dense, None, K, C, count, shift2, within, spread, ws, None)
    L.call("rbvae_kmeans_assign", X, N, Ld, C, K, None, dense, own, d2, None)
    L.call("rbvae_kmeans_update", X, N, Ld, dense, d2, K, C, count, shift2, within, spread, ws, None)
    return C.cpu().numpy(), count.cpu().numpy().astype(np.int64), within.cpu().numpy(), spread.cpu().numpy()


def davies_bouldin(X: torch.Tensor, labels) -> float:
    """sklearn.metrics.davies_bouldin_score(X, labels): the mean over the clusters of the largest (s_i + s_j) / |c_i - c_j|,
    s = a cluster's mean distance to its centroid (spread / count); a zero centroid distance contributes 0, and the score
    is 0 when every spread or every centroid distance is.  The K x K centroid distances are taken on the host in f64."""
    C, n, _, spread = cluster_sums(X, labels)
    intra = spread / n
    cd = np.zeros((len(C), len(C)))
    for l in range(C.shape[1]):
        df = C[:, None, l] - C[None, :, l]
        cd += df * df
    cd = np.sqrt(cd)
    if np.allclose(intra, 0) or np.allclose(cd, 0):
        return 0.0
    cd[cd == 0] = np.inf
    return float(np.mean(np.max((intra[:, None] + intra[None, :]) / cd, axis=1)))


def calinski_harabasz(X: torch.Tensor, labels) -> float:
    """sklearn.metrics.calinski_harabasz_score(X, labels): extra (N - K) / (within (K - 1)), extra = sum_k n_k |c_k - mean|^2,
    within = sum_k within_k; 1.0 when within is 0"""
    C, n, within, _ = cluster_sums(X, labels)
    N, K = X.shape[0], len(C)
    mean = X.double().mean(dim=0).cpu().numpy()
    extra = float((n * ((C - mean) ** 2).sum(1)).sum())
    intra = float(within.sum())
    return 1.0 if intra == 0.0 else extra * (N - K) / (intra * (K - 1.0))


@torch.no_grad()
def latent_symbols(model, x: torch.Tensor, frame_indices: Sequence[int], flags: Sequence[int],
                   n_clusters: Optional[int] = None, projections: Optional[dict] = None, temperature: float = 0.2,
                   noise_ratio: float = 0.3, u=None, max_iter: int = 300, tol: float = 1e-4, seed: int = 42) -> dict:
    """The unsupervised symbols of the script's data in one call: x [F, C, H, W] frames (or latents) on the device, encoded
    by _latents.encode_frames (the same uniforms u [F, L] for the soft and the hard pass; projections["latents"] is used
    instead when present); the states are data.assign_label(frame_indices[f], flags) and
    n_clusters defaults to their number, len(flags) + 1.
    -> {"latents", "codes", "labels" (the states), "kmeans": KMeansResult of the soft latents, "symbols", "codes_unique",
        "symbol_counts": code_symbols of the hard codes, "kmeans_agreement", "symbol_agreement": clustering_agreement of
        either against the states, "davies_bouldin_states", "calinski_harabasz_states", "davies_bouldin_kmeans",
        "calinski_harabasz_kmeans"}"""
    labels = frame_labels(frame_indices, flags, frame_count(x))
    S = len(flags) + 1
    K = S if n_clusters is None else int(n_clusters)
    z, codes = encode_frames(model, x, hard=True, latents=projections.get("latents") if projections is not None else None,
                             temperature=temperature, noise_ratio=noise_ratio, u=u)
    km = kmeans(z, K, max_iter=max_iter, tol=tol, seed=seed)
    symbols, uniq, counts = code_symbols(codes)
    return {"latents": z, "codes": codes, "labels": labels, "kmeans": km, "symbols": symbols, "codes_unique": uniq,
            "symbol_counts": counts,
            "kmeans_agreement": clustering_agreement(labels, km.labels, S, K),
            "symbol_agreement": clustering_agreement(labels, symbols, S, int(uniq.shape[0])),
            "davies_bouldin_states": davies_bouldin(z, labels), "calinski_harabasz_states": calinski_harabasz(z, labels),
            "davies_bouldin_kmeans": davies_bouldin(z, km.labels), "calinski_harabasz_kmeans": calinski_harabasz(z, km.labels)}
