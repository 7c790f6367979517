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
triangle alone and its mirror image, an implicit graph for larger N, OPTICS, assigning new points to a fit, sample weights.
There is no host path: a matrix on the CPU raises.

HDBSCAN* asks the same question at every radius at once (csrc/hdbscan.hip; Campello, Moulavi, Zimek and Sander 2015 in an
order-free form): a hierarchy of density levels, clusters chosen by how long they persist, a membership
strength for every frame (a frame on a transition gets a low one, not a hard -1), and any DBSCAN* cut from the one tree.
  core_distances        the distance to the min_samples-th row, the row itself counted (rbvae_knn)
  mutual_reachability_mst       the minimum spanning tree under the key (w2, lo, hi) by Boruvka rounds on the device
                        (rbvae_mst_start / rbvae_mst_round, the stop decided on the device), sorted by the key
  hdbscan               the tree, then the condensed tree, the selection, labels and probabilities on the host
                        (rbvae_hdbscan_tree); hdbscan_sweep: one tree, one selection per min_cluster_size
  hdbscan_cut           DBSCAN* at one radius from a fit or a tree (rbvae_hdbscan_cut)
  latent_hdbscan        the fit of the script's soft latents, scored as latent_density scores its fits
2 <= N <= 16384 (rbvae_knn's limit), 1 <= L <= 128, 1 <= min_samples <= min(N, 129), 2 <= min_cluster_size <= N.  Not built:
Hamming distance on the hard codes (integer distances make every level one massive tie and duplicate codes give lambda = inf
throughout; dbscan(..., metric="hamming") over bits = 0, 1, 2 ... already is that hierarchy), allow_single_cluster,
cluster_selection_epsilon, max_cluster_size, GLOSH outlier scores, assigning new points, N > 16384.
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
MAX_MST_ROWS = 16384                                # rbvae_mst_ok
MAX_MIN_SAMPLES = 129                               # rbvae_knn's k = min_samples - 1 <= 128
SELECTION_METHODS = ("eom", "leaf")
_MST_LIMITS = "2 <= N <= 16384, 1 <= L <= 128"


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


# ---- HDBSCAN* ------------------------------------------------------------------------------------------------------------------

@dataclass
class MSTResult:
    edges: torch.Tensor                 # int32 [N - 1, 2] on the device, lo < hi, in ascending order of the key (w2, lo, hi)
    d: torch.Tensor                     # f64 [N - 1]: sqrt(w2), the mutual reachability distance of every edge
    w2: torch.Tensor                    # f64 [N - 1]: max(core2_i, core2_j, d2(i, j))
    core_distances: torch.Tensor        # f64 [N]
    n_rounds: int                       # the Boruvka rounds that ran
    min_samples: int

    def __iter__(self):                 # edges, d = mutual_reachability_mst(...)
        return iter((self.edges, self.d))


@dataclass
class HDBSCANResult:
    labels: torch.Tensor                # int32 [N] on the device, -1 for noise; clusters numbered by their smallest row
    probabilities: torch.Tensor         # f64 [N] on the device: the membership strength, 0 for noise
    n_clusters: int
    n_noise: int
    clusters: dict                      # the cluster table on the host, the root first: parent, birth, lambda_max, stability,
                                        # size, selected, min_row (numpy arrays over the clusters of the condensed tree)
    mst: MSTResult
    core_distances: torch.Tensor        # f64 [N] on the device
    min_cluster_size: int
    min_samples: int
    cluster_selection_method: str
    n_rounds: int


def _whole(value, name, lo, hi):
    if isinstance(value, bool) or int(value) != value or not lo <= int(value) <= hi:
        raise ValueError(f"{name} ({value!r}) must be a whole number in [{lo}, {hi}]")
    return int(value)


def _core2(X, N, m):
    from .projection import knn_graph
    if m == 1:
        return torch.zeros(N, dtype=torch.float64, device=X.device)
    return knn_graph(X, m - 1)[1][:, m - 2].contiguous()


def core_distances(X: torch.Tensor, min_samples: int) -> torch.Tensor:
    """f64 [N] on the device, in row order: every row's Euclidean distance to its min_samples-th nearest row, the row itself
    counted as the first (scikit-learn's np.partition(row, m - 1)[m - 1]): sqrt of column m - 2 of rbvae_knn(X, m - 1), zeros
    for min_samples = 1.  k_distances(X, k) is this vector sorted."""
    X, N, _ = checked_matrix(X, "core_distances", "rbvae_mst_ok", _MST_LIMITS)
    m = _whole(min_samples, "min_samples", 1, min(N, MAX_MIN_SAMPLES))
    return torch.sqrt(_core2(X, N, m))


def mutual_reachability_mst(X: torch.Tensor, min_samples: int) -> MSTResult:
    """The minimum spanning tree of the mutual reachability graph w2(i, j) = max(core2_i, core2_j, d2(i, j)) under the strict
    total order (w2, lo, hi) -- so the tree is unique, whatever ties w2 has -- by Boruvka rounds on the device.
    -> MSTResult, which unpacks as (edges, d); sorted by the key on the device, bit-identical between runs, n_rounds included."""
    X, N, Ld = checked_matrix(X, "mutual_reachability_mst", "rbvae_mst_ok", _MST_LIMITS)
    m = _whole(min_samples, "min_samples", 1, min(N, MAX_MIN_SAMPLES))
    dev = X.device
    c2 = _core2(X, N, m)
    comp = torch.empty(N, dtype=torch.int32, device=dev)
    edges = torch.empty((N - 1, 2), dtype=torch.int32, device=dev)
    w2 = torch.empty(N - 1, dtype=torch.float64, device=dev)
    state = torch.empty(4, dtype=torch.int32, device=dev)
    ws = torch.empty(L.query("rbvae_mst_ws_bytes", N) // 8, dtype=torch.int64, device=dev)
    L.call("rbvae_mst_start", N, comp, state, ws)

    def one_round(it):
        L.call("rbvae_mst_round", X, c2, N, Ld, comp, edges, w2, state, ws)

    n_rounds, _, _ = run_until_done(one_round, state, (N - 1).bit_length() + 2)
    done, _, n_comp, n_edges = state.cpu().tolist()
    if not done or n_comp != 1 or n_edges != N - 1:
        raise RuntimeError(f"mutual_reachability_mst: {n_comp} components and {n_edges} edges after {n_rounds} rounds")
    lohi = edges[:, 0].to(torch.int64) * (1 << 32) + edges[:, 1].to(torch.int64)
    order = torch.argsort(lohi, stable=True)
    order = order[torch.argsort(w2[order], stable=True)]
    edges, w2 = edges[order].contiguous(), w2[order].contiguous()
    return MSTResult(edges, torch.sqrt(w2), w2, torch.sqrt(c2), int(n_rounds), m)


def _host_call(name, *args):
    """an entry that takes host pointers and no stream"""
    l = L.lib()
    rc = getattr(l, name)(*[a.ctypes.data if isinstance(a, np.ndarray) else a for a in args])
    if rc != 0:
        msg = l.rbvae_last_error().decode()
        if rc == L.E_INVALID:
            raise ValueError(f"{name}: {msg}")
        raise RuntimeError(f"{name} failed ({rc}): {msg}")


_TABLE = (("parent", np.int32), ("birth", np.float64), ("lambda_max", np.float64), ("stability", np.float64),
          ("size", np.int32), ("selected", np.int32), ("min_row", np.int32))


def _host_tree(edges: np.ndarray, d: np.ndarray, N: int, mcs: int, method: str):
    """rbvae_hdbscan_tree on host arrays -> (labels int32 [N], prob f64 [N], the cluster table)"""
    edges = np.ascontiguousarray(edges, dtype=np.int32)
    d = np.ascontiguousarray(d, dtype=np.float64)
    if edges.shape != (N - 1, 2) or d.shape != (N - 1,):
        raise ValueError(f"the tree of {N} rows has edges [N - 1, 2] and d [N - 1], got {edges.shape} and {d.shape}")
    labels, prob, n = np.empty(N, dtype=np.int32), np.empty(N, dtype=np.float64), np.zeros(1, dtype=np.int32)
    table = {k: np.empty(N, dtype=t) for k, t in _TABLE}
    _host_call("rbvae_hdbscan_tree", edges, d, N, mcs, SELECTION_METHODS.index(method), labels, prob,
               *[table[k] for k, _ in _TABLE], n)
    return labels, prob, {k: v[:int(n[0])].copy() for k, v in table.items()}


def _checked_mst(mst, N=None) -> MSTResult:
    if not isinstance(mst, MSTResult):
        raise ValueError("mst must be mutual_reachability_mst's result")
    if N is not None and mst.core_distances.shape[0] != N:
        raise ValueError(f"mst: built from {mst.core_distances.shape[0]} rows, X has {N}")
    return mst


def _select(mst: MSTResult, tree_host, mcs, method) -> HDBSCANResult:
    N = mst.core_distances.shape[0]
    mcs = _whole(mcs, "min_cluster_size", 2, N)
    if method not in SELECTION_METHODS:
        raise ValueError(f"cluster_selection_method must be one of {SELECTION_METHODS}, got {method!r}")
    labels, prob, table = _host_tree(tree_host[0], tree_host[1], N, mcs, method)
    dev = mst.edges.device
    return HDBSCANResult(torch.from_numpy(labels).to(dev), torch.from_numpy(prob).to(dev), int(table["selected"].sum()),
                         int((labels < 0).sum()), table, mst, mst.core_distances, mcs, mst.min_samples, method, mst.n_rounds)


def hdbscan(X: torch.Tensor, min_cluster_size: int = 5, min_samples: Optional[int] = None,
            cluster_selection_method: str = "eom", mst: Optional[MSTResult] = None) -> HDBSCANResult:
    """HDBSCAN* of the rows of a device matrix, Euclidean distance; min_samples (default: min_cluster_size) counts the row
    itself.  The answer is the order-free one of the module's docstring: it does not change under a permutation of the rows, and
    equals sklearn.cluster.HDBSCAN's (1.7.2) wherever that one is well defined -- the tree's weights, every cut, and the fits
    without ties among the mutual reachabilities (min_samples = 1 as a rule); with ties scikit-learn's answer depends on the
    order of the rows and the number of clusters is what the two have in common.  mst: mutual_reachability_mst's result for the
    same X and min_samples, to select again without building it; X may then be None."""
    if cluster_selection_method not in SELECTION_METHODS:
        raise ValueError(f"cluster_selection_method must be one of {SELECTION_METHODS}, got {cluster_selection_method!r}")
    if isinstance(X, torch.Tensor) and X.dim() == 2 and X.shape[0] >= 2:       # before the tree is built, not after
        _whole(min_cluster_size, "min_cluster_size", 2, X.shape[0])
    if mst is None:
        m = min_cluster_size if min_samples is None else min_samples
        mst = mutual_reachability_mst(X, m)
    else:
        mst = _checked_mst(mst, None if X is None else X.shape[0])
        if min_samples is not None and int(min_samples) != mst.min_samples:
            raise ValueError(f"mst was built with min_samples = {mst.min_samples}, not {min_samples}")
    return _select(mst, (mst.edges.cpu().numpy(), mst.d.cpu().numpy()), min_cluster_size, cluster_selection_method)


def hdbscan_sweep(X: torch.Tensor, min_cluster_sizes: Sequence[int], min_samples: int,
                  cluster_selection_method: str = "eom") -> List[HDBSCANResult]:
    """One tree, one selection per entry of min_cluster_sizes -> the results in the list's order, each equal to
    hdbscan(X, mcs, min_samples).  min_samples must be given: the tree depends on it."""
    if min_samples is None:
        raise ValueError("hdbscan_sweep: min_samples must be given (the tree depends on it)")
    mst = mutual_reachability_mst(X, min_samples)
    host = (mst.edges.cpu().numpy(), mst.d.cpu().numpy())
    return [_select(mst, host, mcs, cluster_selection_method) for mcs in min_cluster_sizes]


def hdbscan_cut(fit_or_mst, cut_distance: float, min_cluster_size: int = 5) -> Tuple[torch.Tensor, int]:
    """DBSCAN* at one radius from the tree of a fit (or from mutual_reachability_mst's result): the components of the edges
    with d <= cut_distance; a component with fewer than min_cluster_size rows is -1, the others are numbered by their smallest
    row (sklearn's HDBSCAN.dbscan_clustering as a partition) -> (labels int32 [N] on the device, n_clusters)."""
    mst = _checked_mst(fit_or_mst.mst if isinstance(fit_or_mst, HDBSCANResult) else fit_or_mst)
    N = mst.core_distances.shape[0]
    mcs = _whole(min_cluster_size, "min_cluster_size", 2, N)
    cut_distance = float(cut_distance)
    if not cut_distance >= 0.0:
        raise ValueError(f"cut_distance ({cut_distance}) must be non-negative")
    labels, n = np.empty(N, dtype=np.int32), np.zeros(1, dtype=np.int32)
    _host_call("rbvae_hdbscan_cut", np.ascontiguousarray(mst.edges.cpu().numpy()), np.ascontiguousarray(mst.d.cpu().numpy()), N,
               cut_distance, mcs, labels, n)
    return torch.from_numpy(labels).to(mst.edges.device), int(n[0])


@torch.no_grad()
def latent_hdbscan(model, x: torch.Tensor, frame_indices: Sequence[int], flags: Sequence[int], min_cluster_size: int = 5,
                   min_samples: Optional[int] = None, cluster_selection_method: str = "eom", tolerance: int = 2,
                   projections: Optional[dict] = None, temperature: float = 0.2, noise_ratio: float = 0.3, u=None) -> dict:
    """latent_density's counterpart without a radius: x [F, C, H, W] frames (or latents) on the device in time order, encoded
    by _latents.encode_frames (projections["latents"] serves as the soft latents when present); soft latents only.
    -> {"latents", "labels" (the states), "fit": HDBSCANResult, "agreement", "noise_fraction", "noise_near_change",
        "noise_runs", "boundaries"} with the scores of latent_density's two fits."""
    labels = frame_labels(frame_indices, flags, frame_count(x))
    z, _ = encode_frames(model, x, hard=False, latents=projections.get("latents") if projections is not None else None,
                         temperature=temperature, noise_ratio=noise_ratio, u=u)
    fit = hdbscan(z, min_cluster_size, min_samples, cluster_selection_method)
    return {"latents": z, "labels": labels, **_density_scores(fit, labels, len(flags) + 1, tolerance)}
