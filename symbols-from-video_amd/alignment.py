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

Many videos aligned: the sequences stacked in one matrix with their lengths, all (or chosen) pairs filled together, one launch
per tile anti-diagonal for the whole batch, every pair's result bit for bit that of dtw on the pair alone.
  dtw_pairs                 a list of pairs of one or two stacks -> [DTWResult], chunked under max_bytes
  dtw_distance_matrix       all pairs a < b mirrored: cost, path_len, normalized [S, S] and the results
  dtw_medoid                the most typical sequence and every sequence's mean cost to the others (host)
  dtw_barycenter            DTW barycenter averaging of the soft latents: a template of fixed length, updated on the device
  vote_labels               several transfer_labels results on the same rows -> the majority (host)
  latent_alignment_videos   all of it for the script's data, and a held-out video's states three ways
No band and no subsequence mode there; squared Euclidean only for the barycenter.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from ._latents import device_matrix, encode_frames, frame_count, frame_labels, require_finite
from .bernoulli import pack_codes
from .density import _host_call
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


# ---- many videos: batched pairs, the distance matrix, the medoid and the DBA barycenter ---------------------------------------------------

PAIR_LIMITS = "1 <= every length <= 16384, 1 <= L <= 128, pairs inside the stacks"


@dataclass
class DTWBarycenter:
    template: torch.Tensor          # f32 [T, L] on the device
    inertia: list                   # the sum of the S costs of every template that was aligned, in order
    n_iter: int                     # the updates made
    converged: bool
    reason: str                     # "converged", "increased" or "max_iter"
    results: list                   # one DTWResult per sequence: the returned template (rows i) against sequence s (rows j)
    count: torch.Tensor             # int32 [T] on the device: the rows of all sequences aligned with every template row


def _checked_stack(X, lengths, name, what):
    X = device_matrix(X, name)
    lengths = np.ascontiguousarray(np.asarray(lengths, dtype=np.int64).reshape(-1).astype(np.int32))
    if lengths.size < 1 or int(lengths.astype(np.int64).sum()) != X.shape[0]:
        raise ValueError(f"{what}: the {lengths.size} lengths of {name} add to {int(lengths.astype(np.int64).sum())}, "
                         f"{name} has {X.shape[0]} rows")
    return X, lengths


def _pair_bytes(n, m, TI, TJ):
    """the device bytes of one pair's blocks, the plan row, state and cost"""
    tiles = -(-n // TI) * -(-m // TJ)
    return ((n * ((m + 3) // 4) + 15) & ~15) + 8 * m + 8 * (n + m + tiles) + 8 * (n + m - 1) + 80 + 12 + 8


class _PairBatch:
    """One batch of pairs on the device: the plan (rbvae_dtw_pairs_plan, built once) and every output, filled and traced as often
    as asked; the stacks may change between fills, their lengths may not."""

    def __init__(self, len_x, len_y, pairs, dev):
        self.len_x, self.len_y, self.pairs, self.P = len_x, len_y, np.ascontiguousarray(pairs, dtype=np.int32), len(pairs)
        P = self.P
        self.off = {k: np.zeros(P + 1, dtype=np.int64) for k in ("dirs", "last", "ws", "path")}
        totals = np.zeros(4, dtype=np.uint64)
        _host_call("rbvae_dtw_pairs_sizes", len_x, len(len_x), len_y, len(len_y), self.pairs, P, *self.off.values(), totals)
        self.dirs_bytes, self.last_n, self.ws_bytes, self.path_rows = (int(t) for t in totals)
        nbytes = L.query("rbvae_dtw_pairs_plan_bytes", P)
        self.plan = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
        launch = np.zeros(2, dtype=np.int32)
        L.call("rbvae_dtw_pairs_plan", len_x.ctypes.data, len(len_x), len_y.ctypes.data, len(len_y), self.pairs.ctypes.data, P,
               self.plan, nbytes, launch.ctypes.data)
        self.n_diag, self.max_tiles = int(launch[0]), int(launch[1])
        self.dirs = torch.empty(self.dirs_bytes, dtype=torch.uint8, device=dev)
        self.last_row = torch.empty(self.last_n, dtype=torch.float64, device=dev)
        self.ws = torch.empty(self.ws_bytes // 8, dtype=torch.float64, device=dev)
        self.path = torch.empty((self.path_rows, 2), dtype=torch.int32, device=dev)
        self.state = torch.empty((P, 3), dtype=torch.int32, device=dev)
        self.cost = torch.empty(P, dtype=torch.float64, device=dev)

    def align(self, X, Y, Ld, metric):
        """fill and trace; X and Y are the f32 stacks, or the packed ones for "hamming" """
        a = (self.plan, self.P, self.n_diag, self.max_tiles, self.dirs, self.dirs_bytes, self.last_row, self.last_n, self.ws,
             self.ws_bytes)
        if metric == "hamming":
            L.call("rbvae_dtw_pairs_fill_bits", X, X.shape[0], Y, Y.shape[0], Ld, *a)
        else:
            L.call("rbvae_dtw_pairs_fill", X, X.shape[0], Y, Y.shape[0], Ld, METRICS[metric], *a)
        L.call("rbvae_dtw_pairs_trace", self.dirs, self.dirs_bytes, self.last_row, self.last_n, self.plan, self.P, self.path,
               self.path_rows, self.state, self.cost)

    def ranges(self, p, lo, hi):
        """rbvae_dtw_path_ranges of pair p into lo, hi int32 [n]"""
        a, b = self.pairs[p]
        r0 = int(self.off["path"][p])
        L.call("rbvae_dtw_path_ranges", self.path[r0:], self.state[p], int(self.len_x[a]), int(self.len_y[b]), lo, hi)

    def results(self):
        state, cost, path = self.state.cpu().numpy(), self.cost.cpu().numpy(), self.path.cpu().numpy()
        out = []
        for p in range(self.P):
            n, start, end = (int(v) for v in state[p])
            if n < 1:
                raise RuntimeError(f"dtw_pairs: the directions of pair {tuple(self.pairs[p])} do not lead to the first row")
            r0, l0, l1 = int(self.off["path"][p]), int(self.off["last"][p]), int(self.off["last"][p + 1])
            c = float(cost[p])
            out.append(DTWResult(c, path[r0:r0 + n].astype(np.int64), n, c / n, start, end, self.last_row[l0:l1], None))
        return out


def _chunks(len_x, len_y, pairs, max_bytes):
    """pair order kept; a chunk's device buffers stay under max_bytes (a pair larger than that is a chunk of its own)"""
    TI, TJ, cap = L.query("rbvae_dtw_tile_rows"), L.query("rbvae_dtw_tile_cols"), 65535
    out, cur, used = [], [], 0
    for a, b in pairs:
        need = _pair_bytes(int(len_x[a]), int(len_y[b]), TI, TJ)
        if cur and (used + need > max_bytes or len(cur) == cap):
            out.append(cur)
            cur, used = [], 0
        cur.append((a, b))
        used += need
    return out + [cur]


def _checked_pairs(X, lengths, pairs, Y, lengths_y, metric, what):
    if metric not in METRICS:
        raise ValueError(f"{what}: metric must be one of {sorted(METRICS)}, got {metric!r}")
    if (Y is None) != (lengths_y is None):
        raise ValueError(f"{what}: Y and lengths_y come together")
    X, lx = _checked_stack(X, lengths, "X", what)
    Y, ly = (X, lx) if Y is None else _checked_stack(Y, lengths_y, "Y", what)
    if X.device != Y.device:
        raise ValueError(f"{what}: X is on {X.device} and Y on {Y.device}")
    if X.shape[1] != Y.shape[1]:
        raise ValueError(f"{what}: X has L={X.shape[1]} columns and Y has L={Y.shape[1]}")
    if pairs is None:
        if Y is not X:
            raise ValueError(f"{what}: pairs=None means all a < b of one stack; two stacks need a pair list")
        pairs = [(a, b) for a in range(len(lx)) for b in range(a + 1, len(lx))]
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if len(pairs) and (pairs.min() < 0 or pairs[:, 0].max() >= len(lx) or pairs[:, 1].max() >= len(ly)):
        raise ValueError(f"{what}: a pair names no sequence; {PAIR_LIMITS}")
    p32 = np.ascontiguousarray(pairs[:1] if len(pairs) else np.zeros((1, 2)), dtype=np.int32)
    if L.query("rbvae_dtw_pairs_ok", lx.ctypes.data, len(lx), ly.ctypes.data, len(ly), p32.ctypes.data, 1, X.shape[1],
               METRICS[metric]) != 1:
        raise ValueError(f"{what}: (lengths {lx.min()} .. {lx.max()} and {ly.min()} .. {ly.max()}, L={X.shape[1]}) outside "
                         f"{PAIR_LIMITS}")
    require_finite(X)
    if Y is not X:
        require_finite(Y)
    return X, lx, Y, ly, [(int(a), int(b)) for a, b in pairs]


def dtw_pairs(X: torch.Tensor, lengths, pairs=None, *, Y: Optional[torch.Tensor] = None, lengths_y=None,
              metric: str = "sqeuclidean", max_bytes: int = 2 ** 31) -> list:
    """Many pairs of sequences aligned together.  X [sum(lengths), L] stacks the sequences (f32 on the device, every sequence's
    rows contiguous and in time order), Y with lengths_y another stack (default: X itself); pairs is a list of (a, b): sequence a
    of X against sequence b of Y, pairs=None all a < b of one stack.  One launch per tile anti-diagonal serves all pairs of a chunk
    (rbvae_dtw_pairs_fill); the pairs are processed in pair order in chunks whose device buffers stay under max_bytes, and every
    pair's result is what dtw(X_a, Y_b, metric=metric) returns, bit for bit, whatever the chunking (there is no band, no
    subsequence mode and no stored table here).  -> [DTWResult] in pair order"""
    X, lx, Y, ly, pairs = _checked_pairs(X, lengths, pairs, Y, lengths_y, metric, "dtw_pairs")
    if not pairs:
        return []
    Ld = X.shape[1]
    Xs, Ys = X, Y
    if metric == "hamming":
        Xs = pack_codes(X)
        Ys = Xs if Y is X else pack_codes(Y)
    out = []
    for chunk in _chunks(lx, ly, pairs, int(max_bytes)):
        batch = _PairBatch(lx, ly, chunk, X.device)
        batch.align(Xs, Ys, Ld, metric)
        out += batch.results()
    return out


def dtw_distance_matrix(X: torch.Tensor, lengths, *, metric: str = "sqeuclidean", max_bytes: int = 2 ** 31) -> dict:
    """All pairs of the S sequences stacked in X.  The pairs a < b are computed (dtw_pairs) and mirrored: the cost is symmetric bit
    for bit (the minimum over paths of sums added in path order, and the transposed table has the same paths), path_len may differ
    under transposition where predecessors tie, so the matrix holds the a < b orientation's.  The diagonal has cost 0 and path
    length n.  -> {"cost": f64 [S, S], "path_len": int64 [S, S], "normalized": cost / path_len f64 [S, S], "results": {(a, b):
    DTWResult for a < b}} on the host"""
    res = dtw_pairs(X, lengths, None, metric=metric, max_bytes=max_bytes)
    lengths = [int(n) for n in np.asarray(lengths).reshape(-1)]
    S = len(lengths)
    cost, plen = np.zeros((S, S), dtype=np.float64), np.diag(np.array(lengths, dtype=np.int64))
    results = {}
    for (a, b), r in zip(((a, b) for a in range(S) for b in range(a + 1, S)), res):
        cost[a, b] = cost[b, a] = r.cost
        plen[a, b] = plen[b, a] = r.path_len
        results[(a, b)] = r
    return {"cost": cost, "path_len": plen, "normalized": cost / plen, "results": results}


def dtw_medoid(cost) -> dict:
    """The most typical sequence of a distance matrix cost [S, S] and every sequence's outlier score.
    -> {"index": the row with the smallest total, the lowest index on a tie; "total": f64 [S] = sum_b cost[a][b] added with b
    ascending; "mean_to_others": total / (S - 1) (0 for S = 1), large for the odd one out}"""
    cost = np.asarray(cost, dtype=np.float64)
    if cost.ndim != 2 or cost.shape[0] != cost.shape[1] or cost.shape[0] < 1:
        raise ValueError(f"cost must be [S, S] with S >= 1, got {cost.shape}")
    S = cost.shape[0]
    total = np.zeros(S, dtype=np.float64)
    for b in range(S):
        total = total + cost[:, b]
    return {"index": int(np.argmin(total)), "total": total, "mean_to_others": total / (S - 1) if S > 1 else np.zeros(S)}


def vote_labels(per_source_labels) -> np.ndarray:
    """Several sources label the same M rows (each a transfer_labels result): every source casts one vote per row, -1 abstains;
    the most frequent label wins, the smallest on a tie, -1 where nobody votes.  -> int64 [M]"""
    votes = [np.asarray(v).astype(np.int64).reshape(-1) for v in per_source_labels]
    if not votes or any(v.shape != votes[0].shape for v in votes):
        raise ValueError("vote_labels needs at least one label vector, all of one length")
    v = np.stack(votes)
    if v.min() < -1:
        raise ValueError("labels must be non-negative, or -1 to abstain")
    K = max(int(v.max()) + 1, 1)
    counts = np.zeros((v.shape[1], K), dtype=np.int64)
    for row in v:
        ok = row >= 0
        np.add.at(counts, (np.nonzero(ok)[0], row[ok]), 1)
    out = counts.argmax(axis=1).astype(np.int64)            # the first maximum: the smallest label
    out[counts.sum(axis=1) == 0] = -1
    return out


def dtw_barycenter(X: torch.Tensor, lengths, *, init="medoid", max_iter: int = 10, tol: float = 1e-6,
                   max_bytes: int = 2 ** 31) -> DTWBarycenter:
    """DTW barycenter averaging (Petitjean et al. 2011) of the S sequences stacked in X under squared Euclidean distance: a
    template of fixed length T whose summed DTW cost to the sequences (the inertia) the iteration lowers.  init: "medoid" (the
    medoid of dtw_distance_matrix), the index of a sequence, or a tensor [T, L].  Every template is aligned with all sequences
    (rbvae_dtw_pairs_fill / _trace, the template on the row side) before it is judged: it >= 1 and its inertia above the best so
    far stops with "increased" and returns the best template; a drop of at most tol times the previous inertia stops with
    "converged"; it == max_iter with "max_iter"; otherwise row i becomes the mean of all rows aligned with it
    (rbvae_dtw_barycenter_update: an f64 sum in sequence and row order, one division, one rounding to f32).  The returned
    results are the returned template's own alignments.  The host reads S costs per iteration."""
    what = "dtw_barycenter"
    X, lx = _checked_stack(X, lengths, "X", what)
    S, Ld, dev = len(lx), X.shape[1], X.device
    max_iter, tol = int(max_iter), float(tol)
    if max_iter < 0 or not tol >= 0:
        raise ValueError(f"{what}: max_iter ({max_iter}) and tol ({tol}) must be non-negative")
    rows = np.concatenate([[0], np.cumsum(lx.astype(np.int64))])
    if isinstance(init, torch.Tensor):
        tmpl = device_matrix(init, "init").clone()
        if tmpl.shape[1] != Ld or tmpl.device != dev:
            raise ValueError(f"{what}: init is {tuple(tmpl.shape)} on {tmpl.device}, X has L={Ld} on {dev}")
    else:
        if isinstance(init, str):
            if init != "medoid":
                raise ValueError(f"{what}: init must be 'medoid', an index or a tensor [T, L], got {init!r}")
            k = dtw_medoid(dtw_distance_matrix(X, lx, max_bytes=max_bytes)["cost"])["index"]
        else:
            k = int(init)
            if not 0 <= k < S:
                raise ValueError(f"{what}: init={k} names none of the {S} sequences")
        tmpl = X[int(rows[k]):int(rows[k + 1])].clone()
    T = tmpl.shape[0]
    lt = np.array([T], dtype=np.int32)
    _, _, _, _, pairs = _checked_pairs(tmpl, lt, [(0, s) for s in range(S)], X, lx, "sqeuclidean", what)
    chunks = _chunks(lt, lx, pairs, int(max_bytes))
    batches = [_PairBatch(lt, lx, c, dev) for c in chunks]
    whole = batches[0] if len(batches) == 1 else _PairBatch(lt, lx, pairs, dev)      # the update's plan: all pairs
    lo = torch.empty((S, T), dtype=torch.int32, device=dev)
    hi = torch.empty((S, T), dtype=torch.int32, device=dev)
    count = torch.empty(T, dtype=torch.int32, device=dev)

    def align(t):
        s, costs = 0, []
        for b in batches:
            b.align(t, X, Ld, "sqeuclidean")
            for p in range(b.P):
                b.ranges(p, lo[s + p], hi[s + p])
            costs += b.cost.cpu().tolist()
            s += b.P
        total = 0.0
        for c in costs:
            total = total + c
        return total

    history, best, best_t, it = [], None, None, 0
    while True:
        inertia = align(tmpl)
        history.append(inertia)
        if it >= 1 and inertia > best:
            reason, tmpl = "increased", best_t
            align(tmpl)                                     # the best template's own paths, the same bits as before
            break
        best, best_t = inertia, tmpl
        if it >= 1 and history[it - 1] - inertia <= tol * history[it - 1]:
            reason = "converged"
            break
        if it == max_iter:
            reason = "max_iter"
            break
        new = torch.empty_like(tmpl)
        L.call("rbvae_dtw_barycenter_update", X, X.shape[0], Ld, whole.plan, S, lo, hi, T, new, count)
        tmpl, it = new, it + 1
    results = [r for b in batches for r in b.results()]
    count = (hi - lo + 1).sum(dim=0, dtype=torch.int32)     # of the returned template's paths
    return DTWBarycenter(tmpl, history, it, reason == "converged", reason, results, count)


def _scored_transfer(got, lb, true_b, S, dev, tolerance):
    bounds = np.nonzero(got[1:] != got[:-1])[0].astype(np.int64) + 1
    return {"labels": got, "accuracy": float((got == lb).mean()),
            "label_agreement": clustering_agreement(lb, torch.from_numpy(got).to(dev), S, S), "boundaries": bounds,
            "boundary_agreement": boundary_agreement(bounds, true_b, tolerance)}


def template_labels(paths, labels, sources) -> np.ndarray:
    """the template's rows labelled by the vote of the sequences `sources`: paths[s] is s's path against the template (template
    rows first), labels[s] its states -> int64 [T]"""
    T = int(paths[sources[0]][-1, 0]) + 1
    return vote_labels([transfer_labels(paths[s][:, ::-1], labels[s], T) for s in sources])


def transfer_three_ways(matrix: dict, labels, paths, fitted, t: int) -> dict:
    """Sequence t takes the others' states three ways: matrix is dtw_distance_matrix of all sequences, labels[v] the states of
    sequence v, paths[v] its path against a template (template rows first, dtw_barycenter's results or a later dtw_pairs),
    fitted the sequences the template averages.  -> {"source": the nearest other sequence (the smallest cost, the lowest index
    on a tie), "nearest": its states carried along the pair's path, "vote": vote_labels over all others' carried states (the
    path of (t, a) serves (a, t) with its columns swapped), "barycenter": the template's rows labelled by the vote of the fitted
    sequences other than t, carried along t's own path}, each int64 [len_t]"""
    V, n_t = matrix["cost"].shape[0], int(paths[t][-1, 1]) + 1
    others = [v for v in range(V) if v != t]
    res = matrix["results"]
    carried = {a: transfer_labels(res[(a, t)].path if a < t else res[(t, a)].path[:, ::-1], labels[a], n_t) for a in others}
    near = min(others, key=lambda a: (matrix["cost"][t, a], a))
    via = transfer_labels(paths[t], template_labels(paths, labels, [s for s in fitted if s != t]), n_t)
    return {"source": near, "nearest": carried[near], "vote": vote_labels(list(carried.values())), "barycenter": via}


@torch.no_grad()
def latent_alignment_videos(model, videos: Sequence[torch.Tensor], frame_indices: Sequence[Sequence[int]],
                            flags: Sequence[Sequence[int]], holdout: Optional[int] = None, *, latents: Optional[Sequence] = None,
                            u: Optional[Sequence] = None, tolerance: int = 2, temperature: float = 0.2,
                            noise_ratio: float = 0.3, max_iter: int = 10) -> dict:
    """Several recordings of one task aligned in one call: videos[v] [F_v, C, H, W] frames on the device in frame order, each
    encoded as latent_alignment encodes its two (u[v] its uniforms, latents[v] given soft latents), with frame_indices[v] and
    flags[v] their own.  All pairs are aligned on the soft latents ("sqeuclidean") and on the hard codes ("hamming"); the
    barycenter is that of the soft latents of all videos, or of all but videos[holdout].  For the held-out video, or for every
    video in turn without one, the others' states are transferred three ways along the soft paths -- from the nearest other
    recording alone, by vote_labels over all others, and through the barycenter, whose rows are labelled by the others' vote and
    then carried along the target's own path -- and each is scored as latent_alignment scores its transfer.
    -> {"latents", "codes", "labels": per video, "lengths", "soft", "hard": dtw_distance_matrix of each, "medoid": {"soft",
        "hard": dtw_medoid}, "outlier_scores": the soft mean_to_others, "fitted": the videos the barycenter averages,
        "barycenter": DTWBarycenter, "paths": per video its path against the template (template rows first), "warp": per video
        warp_map of that path, "template_labels": the fitted videos' vote on the template's rows,
        "transfers": {t: {"nearest": {"source", ...}, "vote": {...}, "barycenter": {...}}} with "labels", "accuracy",
        "label_agreement", "boundaries" and "boundary_agreement" in each}"""
    what = "latent_alignment_videos"
    V = len(videos)
    if V < 2 or len(frame_indices) != V or len(flags) != V or any(x is not None and len(x) != V for x in (u, latents)):
        raise ValueError(f"{what}: at least two videos with as many frame_indices, flags (and u, latents), got {V}, "
                         f"{len(frame_indices)}, {len(flags)}")
    if holdout is not None and not (0 <= int(holdout) < V and V >= 3):
        raise ValueError(f"{what}: holdout ({holdout}) must name one of at least three videos")
    labels = [frame_labels(frame_indices[v], flags[v], frame_count(videos[v])) for v in range(V)]
    enc = [encode_frames(model, videos[v], hard=True, latents=None if latents is None else latents[v],
                         u=None if u is None else u[v], temperature=temperature, noise_ratio=noise_ratio) for v in range(V)]
    z, c = [e[0] for e in enc], [e[1] for e in enc]
    lengths = [int(x.shape[0]) for x in z]
    dev, S = z[0].device, max(len(f) for f in flags) + 1
    soft = dtw_distance_matrix(torch.cat(z).contiguous(), lengths, metric="sqeuclidean")
    hard = dtw_distance_matrix(torch.cat(c).contiguous(), lengths, metric="hamming")
    medoid = {"soft": dtw_medoid(soft["cost"]), "hard": dtw_medoid(hard["cost"])}
    fitted = [v for v in range(V) if v != holdout]
    bary = dtw_barycenter(torch.cat([z[v] for v in fitted]).contiguous(), [lengths[v] for v in fitted], init="medoid",
                          max_iter=max_iter)
    T = bary.template.shape[0]
    paths = dict(zip(fitted, (r.path for r in bary.results)))
    if holdout is not None:
        paths[holdout] = dtw_pairs(bary.template, [T], [(0, 0)], Y=z[holdout], lengths_y=[lengths[holdout]])[0].path

    transfers = {}
    for t in ([int(holdout)] if holdout is not None else range(V)):
        true_t = np.nonzero(labels[t][1:] != labels[t][:-1])[0].astype(np.int64) + 1
        got = transfer_three_ways(soft, labels, paths, fitted, t)
        score = lambda g: _scored_transfer(g, labels[t], true_t, S, dev, tolerance)          # noqa: E731
        transfers[t] = {"nearest": dict(score(got["nearest"]), source=got["source"]), "vote": score(got["vote"]),
                        "barycenter": score(got["barycenter"])}
    return {"latents": z, "codes": c, "labels": labels, "lengths": lengths, "soft": soft, "hard": hard, "medoid": medoid,
            "outlier_scores": medoid["soft"]["mean_to_others"], "fitted": fitted, "barycenter": bary,
            "paths": [paths[v] for v in range(V)], "warp": [warp_map(paths[v], T, lengths[v]) for v in range(V)],
            "template_labels": template_labels(paths, labels, fitted), "transfers": transfers}
