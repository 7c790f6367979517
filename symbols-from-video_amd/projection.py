"""Latent-space projections (the reference's scripts/evaluation/clustering_eval/embedding_umap.py): the soft latents
model.encode(..., temperature=0.2, hard=False, noise_ratio=0.3) of the frames (:214, :224) projected to 2-D by
PCA(n_components=2) (:111-112) and TSNE(n_components=2, random_state=42, perplexity=30) (:87-88), on the device
(csrc/project.hip), as scikit-learn 1.7.2 computes them:
  knn_graph        the exact k nearest neighbours in f64, sorted by (d2, index): what t-SNE (k = 3 perplexity + 1 = 91) and
                   UMAP (:63, n_neighbors = 24 counts the point itself: k = 23) both start from
  tsne_affinities  _binary_search_perplexity on the device; P + P^T, normalised, as one merged CSR on the host, once per fit
  tsne_project     TSNE._tsne: 250 iterations with momentum 0.5 and P x early_exaggeration, then momentum 0.8, learning rate
                   max(N / early_exaggeration / 4, 50), gains as _gradient_descent keeps them; every 50 iterations the KL
                   and the gradient norm come back once, nothing else synchronises
  pca_project      covariance on the device, numpy.linalg.eigh of the L x L matrix, svd_flip(u_based_decision=False),
                   projection on the device, all f64
Two deliberate differences from scikit-learn's defaults: the repulsion is exact (what
_kl_divergence_bh(angle=0) computes) instead of Barnes-Hut at angle 0.5, and the initial map is this module's exact PCA
instead of the randomised-SVD PCA seeded by random_state.

umap.UMAP(n_neighbors=24, min_dist=0.25, metric='euclidean', random_state=42) (:63-64) follows McInnes, Healy, Melville 2018
(Algorithms 2-5) and umap-learn's published defaults (csrc/umap.hip; umap-learn itself is not a dependency):
  umap_ab          a, b of 1 / (1 + a x^(2b)) by scipy's curve fit to the offset exponential (find_ab_params)
  fuzzy_graph      the smooth kNN distances (rho, the bisection on sigma, the memberships) on the device from
                   knn_graph(X, n_neighbors - 1); the fuzzy union W = A + A^T - A o A^T as one merged CSR on the host
  umap_optimise    the edge schedule (entries below max(W) / n_epochs dropped, period = max(W) / W) and one launch per
                   epoch: attraction along the active edges, hashed negative samples, learning rate 1 - n / n_epochs
  umap_project     kNN graph, fuzzy graph, initial map, n_epochs = 500 (200 above 10 000 rows) epochs
Two deliberate differences from umap-learn: the default initial map is this module's exact PCA
(scaled to [0, 10] with 1e-4 noise); umap-learn's own default, the spectral layout of the graph, is init="spectral"
(spectral.py).  And an epoch is synchronous: every vertex moves from the epoch-start map, the attraction of an edge counted twice for the mirror edge's move of the other end, negatives drawn by a
counter hash, so that two runs with one seed agree bit for bit.  The plots stay with the caller.
There is no host path: inputs on the CPU raise.
"""
from __future__ import annotations

import dataclasses
import time
from typing import Optional, Sequence, Union

import numpy as np
import torch

from . import _lib as L
from ._latents import device_matrix as _device_matrix
from ._latents import encode_frames, finite_device_matrix, frame_count, frame_labels

MAX_COMPONENTS = 8                                  # rbvae_pca_project; rbvae_knn: L <= 128, k <= 128, N <= 16384
EXPLORATION_ITERS, N_ITER_CHECK = 250, 50           # TSNE._EXPLORATION_MAX_ITER, TSNE._N_ITER_CHECK
MACHINE_EPSILON = float(np.finfo(np.float64).eps)


def knn_graph(X: torch.Tensor, k: int):
    """rbvae_knn: X f32 [N, L] on the device -> (idx int32 [N, k], d2 f64 [N, k]); row i's k nearest other rows by
    squared Euclidean distance in f64, sorted by (d2, index) ascending."""
    X = finite_device_matrix(X)
    N, Ld = X.shape
    idx = torch.empty((N, int(k)), dtype=torch.int32, device=X.device)
    d2 = torch.empty((N, int(k)), dtype=torch.float64, device=X.device)
    L.call("rbvae_knn", X, N, Ld, int(k), idx, d2)
    return idx, d2


@dataclasses.dataclass
class TSNEAffinities:
    """conditional [N, k] f64, beta [N] f64 and steps [N] int32 from the perplexity search (device); the joint
    distribution (P + P^T) / sum as CSR (indptr int32 [N + 1], indices int32, data f32), on the device."""
    conditional: torch.Tensor
    beta: torch.Tensor
    steps: torch.Tensor
    indptr: torch.Tensor
    indices: torch.Tensor
    data: torch.Tensor


def joint_csr(idx: np.ndarray, cond: np.ndarray):
    """_joint_probabilities_nn's P = P + P.T; P /= max(P.sum(), eps) as (indptr int32, indices int32, data f32): the
    entries (i, idx[i, r]) and their transposes merged by a stable sort on (row, column), exact zeros dropped as the
    sparse sum drops them."""
    N, k = idx.shape
    if idx.min() < 0 or idx.max() >= N:
        raise ValueError(f"neighbour indices outside [0, {N})")
    own = np.repeat(np.arange(N, dtype=np.int64), k)
    nb = idx.reshape(-1).astype(np.int64)
    rows, cols = np.concatenate([own, nb]), np.concatenate([nb, own])
    vals = np.concatenate([cond.reshape(-1), cond.reshape(-1)]).astype(np.float64)
    key = rows * N + cols
    order = np.argsort(key, kind="stable")
    key, vals = key[order], vals[order]
    first = np.concatenate([[True], key[1:] != key[:-1]])
    starts = np.nonzero(first)[0]
    data = np.add.reduceat(vals, starts)
    key = key[starts]
    keep = data != 0.0
    key, data = key[keep], data[keep]
    data = data / max(float(data.sum()), MACHINE_EPSILON)
    indptr = np.zeros(N + 1, dtype=np.int64)
    np.add.at(indptr, key // N + 1, 1)
    return np.cumsum(indptr).astype(np.int32), (key % N).astype(np.int32), data.astype(np.float32)


def tsne_affinities(idx: torch.Tensor, d2: torch.Tensor, perplexity: float = 30.0, timers=None) -> TSNEAffinities:
    """_joint_probabilities_nn on knn_graph's output: the perplexity search on the device, the symmetrised CSR on the
    host."""
    idx = _device_matrix(idx, "idx", torch.int32)
    d2 = _device_matrix(d2, "d2", torch.float64)
    if idx.shape != d2.shape:
        raise ValueError(f"idx {tuple(idx.shape)} and d2 {tuple(d2.shape)} differ in shape")
    N, k = d2.shape
    dev = d2.device
    P = torch.empty((N, k), dtype=torch.float64, device=dev)
    beta = torch.empty(N, dtype=torch.float64, device=dev)
    steps = torch.empty(N, dtype=torch.int32, device=dev)
    (timers or _Timers(None)).span("perplexity", lambda: L.call("rbvae_tsne_perplexity", d2, N, k, float(perplexity), P,
                                                                 beta, steps))
    Ph = P.cpu().numpy()
    if not np.all(np.isfinite(Ph)):
        raise ValueError("the conditional probabilities are not finite (are the distances?)")
    indptr, indices, data = joint_csr(idx.cpu().numpy(), Ph)
    return TSNEAffinities(P, beta, steps, torch.from_numpy(indptr).to(dev), torch.from_numpy(indices).to(dev),
                          torch.from_numpy(data).to(dev))


@dataclasses.dataclass
class PCAResult:
    """embedding f64 [N, n_components] on the device; components [n_components, L], explained_variance
    [n_components] and mean [L] as f64 host arrays (PCA.components_, .explained_variance_, .mean_)."""
    embedding: torch.Tensor
    components: np.ndarray
    explained_variance: np.ndarray
    mean: np.ndarray


def pca_moments(X: torch.Tensor):
    """rbvae_pca_moments -> (mean f64 [L], covariance f64 [L, L], divisor N - 1) on the device"""
    X = _device_matrix(X, "X")
    N, Ld = X.shape
    mean = torch.empty(Ld, dtype=torch.float64, device=X.device)
    cov = torch.empty((Ld, Ld), dtype=torch.float64, device=X.device)
    L.call("rbvae_pca_moments", X, N, Ld, mean, cov)
    return mean, cov


def pca_project(X: torch.Tensor, n_components: int = 2) -> PCAResult:
    """PCA(n_components).fit_transform(X) (:111-112) in f64: the covariance_eigh solver, the sign of each component fixed
    as svd_flip(u_based_decision=False) fixes it (its entry of largest magnitude is positive)."""
    X = _device_matrix(X, "X")
    N, Ld = X.shape
    nc = int(n_components)
    if not 1 <= nc <= min(Ld, MAX_COMPONENTS):
        raise ValueError(f"n_components={nc} outside 1..min(L = {Ld}, {MAX_COMPONENTS})")
    mean, cov = pca_moments(X)
    w, v = np.linalg.eigh(cov.cpu().numpy())
    order = np.argsort(w, kind="stable")[::-1][:nc]
    comp = np.ascontiguousarray(v[:, order].T)
    big = np.argmax(np.abs(comp), axis=1)
    comp *= np.sign(comp[np.arange(nc), big])[:, None]
    out = torch.empty((N, nc), dtype=torch.float64, device=X.device)
    L.call("rbvae_pca_project", X, N, Ld, mean, torch.from_numpy(comp).to(X.device), nc, out)
    return PCAResult(out, comp, np.maximum(w[order], 0.0), mean.cpu().numpy())


@dataclasses.dataclass
class TSNEResult:
    """embedding f32 [N, 2] on the device; kl_divergence and n_iter as TSNE.kl_divergence_ and TSNE.n_iter_ (the index
    of the last iteration run).  One edge differs: at max_iter = 250 scikit-learn still enters its second phase, which
    runs no iteration, and reports n_iter_ = 250 with the largest float as kl_divergence_; here that run ends with
    n_iter = 249 and the KL of the first phase's last iteration."""
    embedding: torch.Tensor
    kl_divergence: float
    n_iter: int


class _Timers:
    """device milliseconds per launch kind, summed over the run, into a dict, when one is given"""

    def __init__(self, sink):
        self.sink, self.spans = sink, []

    def span(self, name, fn):
        if self.sink is None:
            return fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        self.spans.append((name, a, b))

    def close(self):
        if self.sink is not None:
            torch.cuda.synchronize()
            for name, a, b in self.spans:
                self.sink[name] = self.sink.get(name, 0.0) + a.elapsed_time(b)


def tsne_optimise(Y0: torch.Tensor, aff: TSNEAffinities, max_iter: int = 1000, early_exaggeration: float = 12.0,
                  learning_rate: float = 200.0, n_iter_without_progress: int = 300, min_grad_norm: float = 1e-7,
                  timings: Optional[dict] = None) -> TSNEResult:
    """TSNE._tsne from the map Y0 f32 [N, 2]: three launches per iteration, one read-back every 50."""
    Y0 = _device_matrix(Y0, "Y0")
    N = Y0.shape[0]
    if Y0.shape[1] != 2:
        raise ValueError(f"the map must be [N, 2], got {tuple(Y0.shape)}")
    dev = Y0.device
    Y, Yn = Y0.clone(), torch.empty_like(Y0)
    update, gains = torch.zeros_like(Y0), torch.ones_like(Y0)
    part = torch.empty((L.query("rbvae_tsne_repulse_splits", N), N, 3), dtype=torch.float32, device=dev)
    Z = torch.empty(1, dtype=torch.float64, device=dev)
    stats = torch.empty((L.query("rbvae_tsne_step_parts", N), 3), dtype=torch.float64, device=dev)
    sched = torch.empty(3, dtype=torch.float32, device=dev)
    t = _Timers(timings)
    error, it = float(np.finfo(float).max), -1

    def phase(start, stop, exaggeration, momentum, patience):
        nonlocal Y, Yn, error
        sched.copy_(torch.tensor([exaggeration, momentum, learning_rate], dtype=torch.float32))
        best_error, best_iter, i = float(np.finfo(float).max), start, start
        for i in range(start, stop):
            t.span("repulse", lambda: L.call("rbvae_tsne_repulse", Y, N, part))
            t.span("zsum", lambda: L.call("rbvae_tsne_zsum", part, N, Z))
            t.span("step", lambda: L.call("rbvae_tsne_step", Y, Yn, update, gains, aff.indptr, aff.indices, aff.data,
                                          part, Z, sched, N, stats))
            Y, Yn = Yn, Y
            check = (i + 1) % N_ITER_CHECK == 0
            if check or i == stop - 1:
                s = stats.cpu().numpy().sum(axis=0)         # the one synchronisation of these 50 iterations
                error = float(s[2])
            if check:
                if error < best_error:
                    best_error, best_iter = error, i
                elif i - best_iter > patience:
                    break
                if float(np.sqrt(s[1])) <= min_grad_norm:
                    break
        return i

    it = phase(0, EXPLORATION_ITERS, float(early_exaggeration), 0.5, EXPLORATION_ITERS)
    if it + 1 < max_iter:
        it = phase(it + 1, max_iter, 1.0, 0.8, int(n_iter_without_progress))
    t.close()
    return TSNEResult(Y, error, it)


def tsne_project(X: torch.Tensor, perplexity: float = 30.0, max_iter: int = 1000, early_exaggeration: float = 12.0,
                 learning_rate="auto", init: Optional[torch.Tensor] = None, timings: Optional[dict] = None) -> TSNEResult:
    """TSNE(n_components=2, perplexity=perplexity).fit_transform(X) (:87-88) for X f32 [N, L] on the device, with the
    exact repulsion and, unless `init` f32 [N, 2] is given, the exact PCA of X scaled to std(Y[:, 0]) = 1e-4 as the
    initial map.  max_iter >= 250 as in scikit-learn.  timings: a dict that receives the device milliseconds of "knn",
    "perplexity", "pca" and, summed over the iterations, "repulse", "zsum" and "step"."""
    X = _device_matrix(X, "X")
    N = X.shape[0]
    if max_iter < EXPLORATION_ITERS:
        raise ValueError(f"max_iter={max_iter} must be at least {EXPLORATION_ITERS}")
    if not perplexity < N:
        raise ValueError(f"perplexity={perplexity} must be less than the {N} rows")
    k = min(N - 1, int(3.0 * perplexity + 1))
    t = _Timers(timings)
    graph, res = [], []
    t.span("knn", lambda: graph.extend(knn_graph(X, k)))
    aff = tsne_affinities(graph[0], graph[1], perplexity, timers=t)
    if init is None:
        t.span("pca", lambda: res.append(pca_project(X, 2)))
        t.close()
        emb = res[0].embedding.cpu().numpy().astype(np.float32)
        Y0 = torch.from_numpy((emb / np.std(emb[:, 0]) * 1e-4).astype(np.float32)).to(X.device)
    else:
        t.close()
        Y0 = _device_matrix(init, "init")
        if tuple(Y0.shape) != (N, 2):
            raise ValueError(f"init must be [{N}, 2], got {tuple(Y0.shape)}")
    lr = max(N / early_exaggeration / 4.0, 50.0) if learning_rate == "auto" else float(learning_rate)
    return tsne_optimise(Y0, aff, max_iter, early_exaggeration, lr, timings=timings)


# ---- UMAP --------------------------------------------------------------------------------------------------------------

MAX_UMAP_NEIGHBORS = 128                            # rbvae_umap_smooth_knn: n_neighbors - 1 <= 127, two per lane
MAX_UMAP_ROWS = 16384                               # rbvae_umap_epoch


def umap_ab(spread: float = 1.0, min_dist: float = 0.1):
    """umap-learn's find_ab_params: (a, b) of 1 / (1 + a x^(2b)) fitted by scipy.optimize.curve_fit to y = 1 for
    x < min_dist, else exp(-(x - min_dist) / spread), on linspace(0, 3 spread, 300)."""
    from scipy.optimize import curve_fit
    x = np.linspace(0.0, 3.0 * float(spread), 300)
    y = np.where(x < min_dist, 1.0, np.exp(-(x - min_dist) / spread))
    (a, b), _ = curve_fit(lambda x, a, b: 1.0 / (1.0 + a * x ** (2 * b)), x, y)
    return float(a), float(b)


def fuzzy_csr(idx: np.ndarray, w: np.ndarray):
    """The fuzzy union W = A + A^T - A o A^T, A[i, idx[i, r]] = w[i, r] (a row's neighbours distinct), as (indptr int32,
    indices int32, data f32): the entries and their transposes merged by a stable sort on (row, column), the products
    formed in f64 from the f32 memberships as (a + b) - a b, which is the same number for (i, j) and (j, i); exact zeros
    dropped."""
    N, K1 = idx.shape
    if idx.min() < 0 or idx.max() >= N:
        raise ValueError(f"neighbour indices outside [0, {N})")
    own = np.repeat(np.arange(N, dtype=np.int64), K1)
    nb = idx.reshape(-1).astype(np.int64)
    vals = np.asarray(w, dtype=np.float32).reshape(-1).astype(np.float64)
    zero = np.zeros_like(vals)
    key = np.concatenate([own * N + nb, nb * N + own])
    order = np.argsort(key, kind="stable")
    key = key[order]
    starts = np.nonzero(np.concatenate([[True], key[1:] != key[:-1]]))[0]
    a = np.add.reduceat(np.concatenate([vals, zero])[order], starts)
    b = np.add.reduceat(np.concatenate([zero, vals])[order], starts)
    data = (a + b) - a * b
    key = key[starts]
    keep = data != 0.0
    key, data = key[keep], data[keep]
    indptr = np.zeros(N + 1, dtype=np.int64)
    np.add.at(indptr, key // N + 1, 1)
    return np.cumsum(indptr).astype(np.int32), (key % N).astype(np.int32), data.astype(np.float32)


@dataclasses.dataclass
class UMAPGraph:
    """rho [N] f32, sigma [N] f32, steps [N] int32 and membership [N, n_neighbors - 1] f32 from the smooth kNN distances
    (device); the fuzzy union as CSR (indptr int32 [N + 1], indices int32, data f32), on the device."""
    rho: torch.Tensor
    sigma: torch.Tensor
    steps: torch.Tensor
    membership: torch.Tensor
    indptr: torch.Tensor
    indices: torch.Tensor
    data: torch.Tensor


def fuzzy_graph(idx: torch.Tensor, d2: torch.Tensor, n_neighbors: int, timers=None) -> UMAPGraph:
    """The fuzzy simplicial set of knn_graph(X, n_neighbors - 1)'s output: rbvae_umap_smooth_knn on the device, the union
    on the host."""
    idx = _device_matrix(idx, "idx", torch.int32)
    d2 = _device_matrix(d2, "d2", torch.float64)
    if idx.shape != d2.shape:
        raise ValueError(f"idx {tuple(idx.shape)} and d2 {tuple(d2.shape)} differ in shape")
    N, K1 = d2.shape
    k = int(n_neighbors)
    if not 2 <= k <= min(N, MAX_UMAP_NEIGHBORS):
        raise ValueError(f"n_neighbors={k} outside 2..min(N = {N}, {MAX_UMAP_NEIGHBORS})")
    if K1 != k - 1:
        raise ValueError(f"n_neighbors={k} counts the point itself: the graph must have {k - 1} columns, not {K1}")
    dev = d2.device
    dsum = torch.empty(1, dtype=torch.float64, device=dev)
    rho = torch.empty(N, dtype=torch.float32, device=dev)
    sigma = torch.empty(N, dtype=torch.float32, device=dev)
    w = torch.empty((N, K1), dtype=torch.float32, device=dev)
    steps = torch.empty(N, dtype=torch.int32, device=dev)
    (timers or _Timers(None)).span("smooth_knn", lambda: L.call("rbvae_umap_smooth_knn", d2, N, K1, dsum, rho, sigma, w,
                                                                 steps))
    wh = w.cpu().numpy()
    if not np.all(np.isfinite(wh)):
        raise ValueError("the memberships are not finite (are the distances?)")
    indptr, indices, data = fuzzy_csr(idx.cpu().numpy(), wh)
    return UMAPGraph(rho, sigma, steps, w, torch.from_numpy(indptr).to(dev), torch.from_numpy(indices).to(dev),
                     torch.from_numpy(data).to(dev))


def umap_schedule(indptr: np.ndarray, indices: np.ndarray, data: np.ndarray, n_epochs: int, negative_sample_rate: int = 5):
    """The layout's edges and their f32 schedule: entries below max(W) / n_epochs dropped, period = max(W) / W,
    next = period, next_neg = period / negative_sample_rate -> (indptr, indices, period, next, next_neg)."""
    data = np.asarray(data, dtype=np.float32)
    N = len(indptr) - 1
    if data.size == 0:
        raise ValueError("the graph has no edges")
    top = data.max()
    keep = ~(data < top / np.float32(n_epochs))
    rows = np.repeat(np.arange(N), np.diff(indptr))[keep]
    ip = np.zeros(N + 1, dtype=np.int64)
    np.add.at(ip, rows + 1, 1)
    period = (top / data[keep]).astype(np.float32)
    return (np.cumsum(ip).astype(np.int32), np.asarray(indices)[keep].astype(np.int32), period, period.copy(),
            (period / np.float32(negative_sample_rate)).astype(np.float32))


@dataclasses.dataclass
class UMAPResult:
    """embedding f32 [N, 2] on the device; the epochs run and the curve parameters used; init: where the initial map came
    from, "pca", "spectral" or "given" ("pca" after init="spectral" on a graph of several components)"""
    embedding: torch.Tensor
    n_epochs: int
    a: float
    b: float
    init: str = "given"


def umap_optimise(Y0: torch.Tensor, graph: UMAPGraph, n_epochs: Optional[int] = None, a: Optional[float] = None,
                  b: Optional[float] = None, gamma: float = 1.0, negative_sample_rate: int = 5, seed: int = 42,
                  timings: Optional[dict] = None) -> UMAPResult:
    """The layout from the map Y0 f32 [N, 2]: the schedule on the host, then one launch per epoch and no read-back.
    n_epochs None: 500 up to 10 000 rows, else 200; a, b None: umap_ab() of umap-learn's default min_dist 0.1."""
    Y0 = _device_matrix(Y0, "Y0")
    N = Y0.shape[0]
    if Y0.shape[1] != 2:
        raise ValueError(f"the map must be [N, 2], got {tuple(Y0.shape)}")
    if graph.indptr.numel() != N + 1:
        raise ValueError(f"the graph has {graph.indptr.numel() - 1} rows, the map {N}")
    if n_epochs is None:
        n_epochs = 500 if N <= 10000 else 200
    n_epochs, rate = int(n_epochs), int(negative_sample_rate)
    if not L.query("rbvae_umap_epoch_ok", N, n_epochs, rate):
        raise ValueError(f"N={N} (2..{MAX_UMAP_ROWS}), n_epochs={n_epochs} or negative_sample_rate={rate} is not covered")
    if a is None or b is None:
        a, b = umap_ab()
    dev = Y0.device
    sch = umap_schedule(graph.indptr.cpu().numpy(), graph.indices.cpu().numpy(), graph.data.cpu().numpy(), n_epochs, rate)
    indptr, indices, period, nxt, nxt_neg = (torch.from_numpy(x).to(dev) for x in sch)
    Y, Yn = Y0.clone(), torch.empty_like(Y0)
    t = _Timers(timings)

    def run():
        nonlocal Y, Yn
        for n in range(n_epochs):
            L.call("rbvae_umap_epoch", Y, Yn, indptr, indices, period, nxt, nxt_neg, N, n, n_epochs, float(a), float(b),
                   float(gamma), rate, int(seed))
            Y, Yn = Yn, Y

    t.span("epochs", run)
    t.close()
    return UMAPResult(Y, n_epochs, float(a), float(b))


def umap_initial_map(pca_embedding: np.ndarray, seed: int = 42) -> np.ndarray:
    """The exact PCA scaled by 10 / max |.|, plus RandomState(seed).normal(scale=1e-4), each column min-max scaled to
    [0, 10]; f64 on the host, cast to f32."""
    Y = np.asarray(pca_embedding, dtype=np.float64)
    Y = Y * (10.0 / max(float(np.abs(Y).max()), np.finfo(np.float64).tiny))
    Y = Y + np.random.RandomState(seed).normal(scale=1e-4, size=Y.shape)
    lo, hi = Y.min(0), Y.max(0)
    return (10.0 * (Y - lo) / np.where(hi > lo, hi - lo, 1.0)).astype(np.float32)


def umap_project(X: torch.Tensor, n_neighbors: int = 15, min_dist: float = 0.1, spread: float = 1.0,
                 n_epochs: Optional[int] = None, seed: int = 42, init: Union[None, str, torch.Tensor] = None,
                 timings: Optional[dict] = None) -> UMAPResult:
    """umap.UMAP(n_neighbors, min_dist, metric='euclidean', random_state=seed).fit_transform(X) (:63-64) for X f32 [N, L]
    on the device, as this module states it: the exact kNN graph, the synchronous epoch and an initial map: init None or
    "pca": umap_initial_map of the exact PCA; "spectral": umap_initial_map of spectral.spectral_layout(graph, 2) of the
    graph just built (umap-learn's default), falling back to the PCA map when the graph has several components; an f32
    [N, 2] device tensor: that map.  UMAPResult.init says which was used.  timings: a dict that receives the device
    milliseconds of "knn", "smooth_knn", "pca" and "epochs", and the host's wall milliseconds for "fuzzy_csr" and
    "spectral"."""
    X = _device_matrix(X, "X")
    N = X.shape[0]
    k = int(n_neighbors)
    if not 2 <= k <= min(N, MAX_UMAP_NEIGHBORS):
        raise ValueError(f"n_neighbors={k} outside 2..min(N = {N}, {MAX_UMAP_NEIGHBORS})")
    if N > MAX_UMAP_ROWS:
        raise ValueError(f"N={N} above {MAX_UMAP_ROWS}")
    a, b = umap_ab(spread, min_dist)
    t = _Timers(timings)
    knn, res = [], []
    t.span("knn", lambda: knn.extend(knn_graph(X, k - 1)))
    t0 = time.perf_counter()
    graph = fuzzy_graph(knn[0], knn[1], k, timers=t)
    if timings is not None:
        timings["fuzzy_csr"] = 1e3 * (time.perf_counter() - t0)     # includes the wait for the kNN and smooth-kNN launches
    if isinstance(init, str) and init not in ("pca", "spectral"):
        raise ValueError(f"init must be 'pca', 'spectral', None or the initial map, got {init!r}")
    used, Y0 = "given", None
    if isinstance(init, str) and init == "spectral":
        from . import spectral
        t1 = time.perf_counter()
        ng = spectral.normalized_graph(graph)
        if ng.n_components == 1:
            lay = spectral.spectral_layout(ng, 2)
            Y0, used = torch.from_numpy(umap_initial_map(lay.cpu().numpy(), seed)).to(X.device), "spectral"
        if timings is not None:
            timings["spectral"] = 1e3 * (time.perf_counter() - t1)
    if Y0 is None and (init is None or isinstance(init, str)):
        t.span("pca", lambda: res.append(pca_project(X, 2)))
        t.close()
        Y0, used = torch.from_numpy(umap_initial_map(res[0].embedding.cpu().numpy(), seed)).to(X.device), "pca"
    elif Y0 is None:
        t.close()
        Y0 = _device_matrix(init, "init")
        if tuple(Y0.shape) != (N, 2):
            raise ValueError(f"init must be [{N}, 2], got {tuple(Y0.shape)}")
    else:
        t.close()
    return dataclasses.replace(umap_optimise(Y0, graph, n_epochs, a, b, seed=seed, timings=timings), init=used)


@torch.no_grad()
def latent_projections(model, x: torch.Tensor, temperature: float = 0.2, noise_ratio: float = 0.3,
                       frame_indices: Optional[Sequence[int]] = None, flags: Optional[Sequence[int]] = None,
                       u=None, umap: Optional[dict] = None, **tsne_kw) -> dict:
    """The script's loop (:209-228) as one batched call: x [F, C, H, W] frames (or latents) on the device, one
    sequence of length 1 per frame, z = model.encode(x, temperature, hard=False, noise_ratio) (:214, :224) through
    _latents.encode_frames, then both projections of the soft latents.  Labels (:228) come from
    data.assign_label(frame_indices[f], flags) when both are given; u [F, L]: the binarisation uniforms instead of the host draw.  tsne_kw goes to tsne_project.  umap: keyword
    arguments of umap_project (the script's: {"n_neighbors": 24, "min_dist": 0.25, "seed": 42}); None leaves UMAP out.
    -> {"latents": f32 [F, L], "pca": PCAResult, "tsne": TSNEResult, "labels": int64 array or None} and, with `umap`,
    "umap": UMAPResult"""
    F = frame_count(x)
    z, _ = encode_frames(model, x, hard=False, temperature=temperature, noise_ratio=noise_ratio, u=u)
    labels = None
    if frame_indices is not None and flags is not None:
        labels = frame_labels(frame_indices, flags, F)
    out = {"latents": z, "pca": pca_project(z, 2), "tsne": tsne_project(z, **tsne_kw), "labels": labels}
    if umap is not None:
        out["umap"] = umap_project(z, **umap)
    return out
