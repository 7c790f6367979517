"""Spectral layout of the neighbour graph: the lowest eigenvectors of the symmetric-normalised Laplacian L = I - S,
S = D^-1/2 W D^-1/2, of the fuzzy graph projection.fuzzy_graph leaves on the device, by Lanczos with full
reorthogonalisation on the device (csrc/spectral.hip).  One solver, three uses:
  normalized_graph     the degrees, 1 / sqrt(deg) and the number of connected components of a symmetric CSR graph
  lanczos_eigsh        the k lowest eigenpairs of L: steps enqueued eight at a time, the tridiagonal problem solved on the
                       host (scipy.linalg.eigh_tridiagonal) between two reads of (alpha, beta, state), stopped when every
                       wanted Ritz pair has |beta_m s_mi| <= tol; Ritz vectors and their true residuals on the device
  spectral_layout      umap-learn's spectral_layout of a connected graph: eigenvectors 1..dim of L, not divided by
                       sqrt(deg); the trivial eigenvector sqrt(deg) / |sqrt(deg)| is known in closed form and locked, so
                       the solver looks only for what is wanted (and a regular graph cannot break the run down at step 1)
  spectral_embedding   scikit-learn 1.7.2's sklearn.manifold.spectral_embedding(adjacency, norm_laplacian=True): the
                       eigenvectors times 1 / sqrt(deg), sign-flipped, the first dropped with drop_first
  spectral_clustering  SpectralClustering(affinity="precomputed", assign_labels="kmeans") with n_init = 1: the embedding
                       of n_clusters columns rounded to f32, then symbols.kmeans
  latent_spectral      all of it for the script's data
Deviations: every eigenvector is sign-fixed (its entry of largest magnitude, the lowest index on a
tie, is positive: scikit-learn's _deterministic_vector_sign_flip; ARPACK's sign in umap-learn is arbitrary); k-means runs
once (n_init = 1, scikit-learn's default is 10); a graph of several components is refused by spectral_layout (umap-learn
lays the components out one by one) and single-vector Lanczos finds one copy of a multiple eigenvalue.  Not built: a
block or restarted solver for N m beyond the workspace (m <= 1024 steps).  There is no host path.
"""
from __future__ import annotations

import dataclasses
import warnings
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from ._latents import encode_frames, frame_count, frame_labels

MAX_STEPS, MAX_LOCKED, MAX_COLS = 1024, 8, 32       # rbvae_spectral_ok, rbvae_spectral_ritz
ENQUEUE = 8                                         # steps enqueued between two reads of (alpha, beta, state)


@dataclasses.dataclass
class NormalizedGraph:
    """The CSR graph (device), deg f64 [N] and isd = 1 / sqrt(deg) f64 [N] (device; 0 where deg = 0), and the number of
    connected components of the pattern (scipy.sparse.csgraph.connected_components on the host)"""
    indptr: torch.Tensor
    indices: torch.Tensor
    data: torch.Tensor
    deg: torch.Tensor
    isd: torch.Tensor
    n_components: int

    @property
    def n(self) -> int:
        return self.indptr.numel() - 1


@dataclasses.dataclass
class EigResult:
    """eigenvalues f64 [k'] of L = I - S ascending (host); vectors f64 [N, k'] on the device, unit 2-norm, sign-fixed;
    residuals f64 [k']: |S y - theta y|_2 computed on the device; steps: Lanczos steps taken; why: "tol", "max_steps" or
    "invariant" (breakdown: the Krylov space is invariant, k' may be below k)"""
    eigenvalues: np.ndarray
    vectors: torch.Tensor
    residuals: np.ndarray
    steps: int
    converged: bool
    why: str


def normalized_graph(indptr, indices=None, data=None) -> NormalizedGraph:
    """From a projection.UMAPGraph, a NormalizedGraph (returned as it is) or the three CSR arrays (device tensors or
    numpy): checks that the graph is square, sorted by column within a row without duplicates (as fuzzy_csr writes it),
    finite and non-negative; degrees on the device (rbvae_spectral_degree)."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    if isinstance(indptr, NormalizedGraph):
        return indptr
    if indices is None and hasattr(indptr, "indptr"):
        indptr, indices, data = indptr.indptr, indptr.indices, indptr.data
    host = [x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x) for x in (indptr, indices, data)]
    ip, ix, w = host[0].astype(np.int64), host[1].astype(np.int64), host[2]
    N = len(ip) - 1
    if not L.query("rbvae_spectral_ok", N, 1, 0):
        raise ValueError(f"the graph has {N} rows, outside 2..1048576")
    if ip[0] != 0 or np.any(np.diff(ip) < 0) or ip[-1] != len(ix) or len(w) != len(ix):
        raise ValueError("indptr does not describe the indices and data given")
    if len(ix) and (ix.min() < 0 or ix.max() >= N):
        raise ValueError(f"the graph is not square: column indices outside [0, {N})")
    rows = np.repeat(np.arange(N), np.diff(ip))
    if len(ix) > 1 and np.any((np.diff(ix) <= 0) & (np.diff(rows) == 0)):
        raise ValueError("a row's columns must ascend without duplicates")
    if not np.all(np.isfinite(w)) or np.any(w < 0):
        raise ValueError("the weights must be finite and non-negative")
    ncomp = int(connected_components(csr_matrix((np.ones(len(ix), dtype=np.int8), ix, ip), shape=(N, N)), directed=False,
                                     return_labels=False))
    dev = next((x.device for x in (indptr, indices, data) if isinstance(x, torch.Tensor) and x.is_cuda), torch.device("cuda"))
    d_ip = torch.from_numpy(ip.astype(np.int32)).to(dev)
    d_ix = torch.from_numpy(ix.astype(np.int32)).to(dev)
    d_w = torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32)).to(dev)
    deg = torch.empty(N, dtype=torch.float64, device=dev)
    isd = torch.empty(N, dtype=torch.float64, device=dev)
    L.call("rbvae_spectral_degree", d_ip, d_ix, d_w, N, deg, isd)
    return NormalizedGraph(d_ip, d_ix, d_w, deg, isd, ncomp)


def _workspace(N, m_max, q, dev):
    nbytes = L.query("rbvae_spectral_ws_bytes", N, m_max, q)
    return torch.empty(nbytes // 8, dtype=torch.float64, device=dev), nbytes


def _unit(w: torch.Tensor, ws, nbytes) -> torch.Tensor:
    """w / |w|_2 with the norm taken by the kernels' fixed-order sum"""
    n2 = torch.empty(1, dtype=torch.float64, device=w.device)
    L.call("rbvae_spectral_dots", w, 1, w.numel(), w, n2, ws, nbytes)
    return w / torch.sqrt(n2)


def _orthogonalise(w: torch.Tensor, V: torch.Tensor, q: int, ws, nbytes):
    """two classical Gram-Schmidt passes of w against the first q rows of V, in place"""
    c = torch.empty(max(q, 1), dtype=torch.float64, device=w.device)
    for _ in range(2 if q else 0):
        L.call("rbvae_spectral_dots", V, q, w.numel(), w, c, ws, nbytes)
        L.call("rbvae_spectral_update", V, q, w.numel(), c, w)


def trivial_vector(graph: NormalizedGraph) -> torch.Tensor:
    """sqrt(deg) / |sqrt(deg)|_2: the eigenvector of L for the eigenvalue 0"""
    ws, nbytes = _workspace(graph.n, 1, 0, graph.deg.device)
    return _unit(torch.sqrt(graph.deg), ws, nbytes)


def sign_fix(Y: torch.Tensor) -> torch.Tensor:
    """scikit-learn's _deterministic_vector_sign_flip on the rows of Y f64 [k, N] (device): the decision is taken on the
    host (numpy's argmax keeps the lowest index on a tie), the flip on the device"""
    h = Y.cpu().numpy()
    big = np.argmax(np.abs(h), axis=1)
    sg = np.sign(h[np.arange(len(h)), big])
    sg[sg == 0] = 1.0
    return Y * torch.from_numpy(sg).to(Y.device)[:, None]


def lanczos_eigsh(graph, k: int, tol: float = 1e-10, max_steps: Optional[int] = None, v0=None, seed: int = 0,
                  locked=None) -> EigResult:
    """The k lowest eigenpairs of L = I - S in the orthogonal complement of the locked vectors (f64 [q, N] or [N] for one,
    q <= 8, orthonormal eigenvectors the caller already knows).  v0 None: np.random.RandomState(seed).uniform(-1, 1, N),
    scikit-learn's _init_arpack_v0; it is orthogonalised against the locked vectors and normalised.  max_steps None:
    min(N - q, 1024).  On breakdown with fewer than k pairs it returns what exists, converged False, why "invariant"."""
    from scipy.linalg import eigh_tridiagonal
    g = normalized_graph(graph)
    N, dev, k = g.n, g.deg.device, int(k)
    if locked is None:
        lock = torch.empty((0, N), dtype=torch.float64, device=dev)
    else:
        lock = torch.as_tensor(locked).to(device=dev, dtype=torch.float64).reshape(-1, N).contiguous()
    q = lock.shape[0]
    if q > MAX_LOCKED:
        raise ValueError(f"{q} locked vectors, at most {MAX_LOCKED}")
    if N - q < 1:
        raise ValueError(f"nothing is left of {N} dimensions beside {q} locked vectors")
    m_max = min(N - q, MAX_STEPS) if max_steps is None else int(max_steps)
    if not 1 <= m_max <= MAX_STEPS:
        raise ValueError(f"max_steps={m_max} outside 1..{MAX_STEPS}")
    if not 1 <= k <= m_max:
        raise ValueError(f"k={k} outside 1..max_steps = {m_max}")
    if not tol >= 0:
        raise ValueError(f"tol={tol} must be non-negative")
    ws, nbytes = _workspace(N, m_max, q, dev)
    V = torch.zeros((q + m_max + 1, N), dtype=torch.float64, device=dev)
    V[:q] = lock
    if v0 is None:
        v0 = np.random.RandomState(seed).uniform(-1, 1, N)
    w = torch.as_tensor(v0).to(device=dev, dtype=torch.float64).reshape(-1).contiguous().clone()
    if w.numel() != N or not bool(torch.isfinite(w).all()):
        raise ValueError(f"v0 must be {N} finite numbers")
    _orthogonalise(w, V, q, ws, nbytes)
    V[q] = _unit(w, ws, nbytes)
    alpha = torch.zeros(m_max, dtype=torch.float64, device=dev)
    beta = torch.zeros(m_max, dtype=torch.float64, device=dev)
    state = torch.zeros(2, dtype=torch.int32, device=dev)
    enq = 0
    while True:
        for _ in range(min(ENQUEUE, m_max - enq)):
            L.call("rbvae_spectral_step", g.indptr, g.indices, g.data, g.isd, N, V, q, enq, m_max, alpha, beta, state, ws,
                   nbytes)
            enq += 1
        broken, m = state.cpu().tolist()
        a, b = alpha[:m].cpu().numpy(), beta[:m].cpu().numpy()
        if not (np.all(np.isfinite(a)) and np.all(np.isfinite(b))):
            raise ValueError("the Lanczos coefficients are not finite (is the start vector?)")
        theta, s = (a.copy(), np.ones((1, 1))) if m == 1 else eigh_tridiagonal(
            a, b[:m - 1], select="i", select_range=(max(m - k, 0), m - 1))    # the k largest suffice
        kk = min(k, m)
        pick = np.argsort(-theta, kind="stable")[:kk]       # the largest of S are the lowest of L
        est = np.abs(b[m - 1] * s[m - 1, pick])
        if broken:
            why, converged = "invariant", kk == k
            break
        if kk == k and np.all(est <= tol):
            why, converged = "tol", True
            break
        if m >= m_max:
            why, converged = "max_steps", False
            break
    Y = torch.empty((kk, N), dtype=torch.float64, device=dev)
    res = torch.empty(kk, dtype=torch.float64, device=dev)
    th = torch.from_numpy(np.ascontiguousarray(theta[pick])).to(dev)
    rws, rbytes = _workspace(N, 1, 0, dev)
    for c0 in range(0, kk, MAX_COLS):
        c1 = min(kk, c0 + MAX_COLS)
        sc = torch.from_numpy(np.ascontiguousarray(s[:, pick[c0:c1]])).to(dev)
        L.call("rbvae_spectral_ritz", V, q, m, N, sc, c1 - c0, Y[c0:c1])
        L.call("rbvae_spectral_residuals", g.indptr, g.indices, g.data, g.isd, N, Y[c0:c1], c1 - c0, th[c0:c1], res[c0:c1],
               rws, rbytes)
    return EigResult(1.0 - theta[pick], sign_fix(Y).t().contiguous(), res.cpu().numpy(), int(m), bool(converged), why)


def spectral_layout(graph, dim: int = 2, **solver_kw) -> torch.Tensor:
    """umap-learn's spectral_layout for a connected graph -> f64 [N, dim] on the device: eigenvectors 1..dim of L."""
    return _layout(graph, dim, **solver_kw).vectors


def _layout(graph, dim, **solver_kw) -> EigResult:
    g = normalized_graph(graph)
    if g.n_components > 1:
        raise ValueError(f"the graph has {g.n_components} connected components; the spectral layout is built for a "
                         "connected graph (umap-learn's multi-component layout is not)")
    return lanczos_eigsh(g, int(dim), locked=trivial_vector(g), **solver_kw)


def spectral_embedding(graph, n_components: int = 8, drop_first: bool = True, **solver_kw) -> torch.Tensor:
    """sklearn.manifold.spectral_embedding(adjacency, n_components, norm_laplacian=True, drop_first=drop_first) -> f64
    [N, n_components] on the device.  The trivial eigenvector is the locked closed form; the others come from the solver."""
    g = normalized_graph(graph)
    nc = int(n_components)
    if g.n_components > 1:
        warnings.warn("Graph is not fully connected, spectral embedding may not work as expected.")
    q0 = trivial_vector(g)
    want = nc if drop_first else nc - 1
    if want < 0 or (nc < 1):
        raise ValueError(f"n_components={nc} must be at least 1")
    cols = [] if drop_first else [q0[None]]
    if want:
        r = lanczos_eigsh(g, want, locked=q0, **solver_kw)
        if r.vectors.shape[1] < want:
            raise ValueError(f"only {r.vectors.shape[1]} of {want} eigenvectors exist in the Krylov space ({r.why})")
        cols.append(r.vectors.t())
    return sign_fix(torch.cat(cols, 0) * g.isd[None]).t().contiguous()


def spectral_clustering(graph, n_clusters: int, seed: int = 0, **solver_kw):
    """SpectralClustering(n_clusters, affinity="precomputed", assign_labels="kmeans", n_init=1, random_state=seed) ->
    (symbols.KMeansResult, the embedding f64 [N, n_clusters])"""
    from .symbols import kmeans
    emb = spectral_embedding(graph, int(n_clusters), drop_first=False, **solver_kw)
    return kmeans(emb.float().contiguous(), int(n_clusters), seed=seed), emb


@torch.no_grad()
def latent_spectral(model, x: torch.Tensor, frame_indices: Optional[Sequence[int]] = None,
                    flags: Optional[Sequence[int]] = None, n_neighbors: int = 24, n_clusters: Optional[int] = None,
                    n_components: int = 2, temperature: float = 0.2, noise_ratio: float = 0.3, u=None, seed: int = 0,
                    **solver_kw) -> dict:
    """The script's data in one call, in the mould of symbols.latent_symbols: x [F, C, H, W] frames (or latents) on the
    device are encoded by _latents.encode_frames (the soft pass), then knn_graph(z, n_neighbors - 1), fuzzy_graph,
    spectral_embedding(n_components) and spectral_clustering(n_clusters; default the number of states, len(flags) + 1).
    -> {"latents", "graph": NormalizedGraph, "embedding", "clustering": KMeansResult, "cluster_embedding", "labels" and
        "agreement": clustering_agreement against the states (None without frame_indices and flags)}"""
    from .projection import fuzzy_graph, knn_graph
    from .symbols import clustering_agreement
    F = frame_count(x)
    if n_clusters is None and flags is None:
        raise ValueError("n_clusters or flags must be given")
    K = len(flags) + 1 if n_clusters is None else int(n_clusters)
    z, _ = encode_frames(model, x, hard=False, temperature=temperature, noise_ratio=noise_ratio, u=u)
    k = int(n_neighbors)
    g = normalized_graph(fuzzy_graph(*knn_graph(z, k - 1), k))
    km, cemb = spectral_clustering(g, K, seed=seed, **solver_kw)
    labels = agreement = None
    if frame_indices is not None and flags is not None:
        labels = frame_labels(frame_indices, flags, F)
        agreement = clustering_agreement(labels, km.labels, len(flags) + 1, K)
    return {"latents": z, "graph": g, "embedding": spectral_embedding(g, int(n_components), **solver_kw), "clustering": km,
            "cluster_embedding": cemb, "labels": labels, "agreement": agreement}
