"""The numpy restatement of csrc/dbscan.hip: scikit-learn 1.7.2's DBSCAN in its order-free form, and the FastSV round that finds
the components on the device.  Everything behind the distance comparison is integer, so the device equals this bit for bit.

  1. j in N(i) iff d(i, j) <= eps, and i in N(i)            adjacency / hamming_adjacency -> bool [N, N]
  2. row i is core iff |N(i)| >= min_samples                core_rows
  3. clusters = components of the core rows under j in N(i) components (a breadth-first search: independent of the rounds)
  4. ids in ascending order of the smallest core index      labels_from_roots
  5. a non-core row with a core neighbour takes the lowest id among its core neighbours' clusters
  6. any other non-core row is -1
The round (rounds / run_rounds), Jacobi: gf[u] = f[f[u]]; mn[u] = min of gf[v] over the core v in N(u), v != u (N without one);
out = f; then out[f[u]] = min(., mn[u]), out[u] = min(., mn[u]), out[u] = min(., gf[u]) for every core u.  f = i for a core row
and N for the others at the start; the fixed point is the smallest core index of the row's component.  n_rounds counts every
round that ran, the last one (which changes nothing) included, as state[1] does on the device.

d2 is rbvae_knn's: the f32 values widened to f64, l ascending, the difference exact, the square and the addition rounded once
each (numpy never fuses the two).
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dbscan.npz")


def d2_matrix(X):
    """f64 [N, N] of the f32 matrix X [N, L]"""
    X = np.asarray(X, dtype=np.float32).astype(np.float64)
    N, L = X.shape
    s = np.zeros((N, N))
    with np.errstate(invalid="ignore", over="ignore"):
        for l in range(L):
            df = X[:, None, l] - X[None, :, l]
            s += df * df
    return s


def adjacency(X, eps2):
    """bool [N, N]: d2 <= eps2 (NaN compares false)"""
    with np.errstate(invalid="ignore"):
        return d2_matrix(X) <= np.float64(eps2)


def hamming_matrix(X):
    """int64 [N, N]: the number of positions where the bits X > 0.5 of two rows differ"""
    B = (np.asarray(X) > 0.5).astype(np.float64)        # products of 0 / 1 and sums below 2^53: exact
    return (B @ (1.0 - B).T + (1.0 - B) @ B.T).astype(np.int64)


def hamming_adjacency(X, max_bits):
    return hamming_matrix(X) <= int(max_bits)


def words(N):
    return (N + 63) // 64


def pack_adj(A):
    """bool [N, M] -> uint64 [N, ceil(M / 64)]: bit j % 64 of word j / 64; the padding bits are zero"""
    A = np.asarray(A, dtype=bool)
    N, M = A.shape
    W = words(M)
    full = np.zeros((N, W * 64), dtype=np.uint8)
    full[:, :M] = A
    return np.packbits(full, axis=1, bitorder="little").view("<u8").reshape(N, W)


def unpack_adj(adj, N):
    """uint64 / int64 [N, W] -> (bool [N, N], bool [N, 64 W - N]: the padding)"""
    a = np.ascontiguousarray(adj).view(np.uint8).reshape(adj.shape[0], -1)
    full = np.unpackbits(a, axis=1, bitorder="little").astype(bool)
    return full[:, :N], full[:, N:]


def core_rows(A, min_samples):
    cnt = A.sum(axis=1).astype(np.int32)
    return cnt, cnt >= int(min_samples)


def start(core):
    N = len(core)
    return np.where(core, np.arange(N), N).astype(np.int32)


def core_graph(A, core):
    Ac = A & core[None, :] & core[:, None]
    Ac = Ac.copy()
    np.fill_diagonal(Ac, False)
    return Ac


def one_round(Ac, core, f):
    """-> f_out of one Jacobi round"""
    N = len(f)
    fe = np.append(f, N).astype(np.int64)                # fe[N] = N: a non-core row's parent leads nowhere
    gf = fe[fe[:N]]
    mn = np.where(Ac, gf[None, :], N).min(axis=1)
    out = f.astype(np.int64).copy()
    cu = np.flatnonzero(core)
    hooked = mn[cu] < N
    np.minimum.at(out, f[cu][hooked], mn[cu][hooked])    # hooking
    out[cu] = np.minimum(out[cu], mn[cu])                # aggressive
    out[cu] = np.minimum(out[cu], gf[cu])                # shortcut
    return out.astype(np.int32)


def run_rounds(A, core, limit=None):
    """-> (the list of f after every round, n_rounds): the rounds run until one changes nothing, and that one counts"""
    Ac = core_graph(A, core)
    f = start(core)
    out = []
    while True:
        g = one_round(Ac, core, f)
        out.append(g)
        if np.array_equal(g, f):
            return out, len(out)
        f = g
        assert limit is None or len(out) < limit, "the rounds do not settle"


def components(A, core):
    """f int32 [N] by a breadth-first search: the smallest core index of a core row's component, N for the others"""
    N = len(core)
    Ac = core_graph(A, core)
    f = np.full(N, N, dtype=np.int32)
    for r in range(N):
        if not core[r] or f[r] != N:
            continue
        f[r] = r                                        # r ascends: the first row of a component is its smallest
        todo = [r]
        while todo:
            u = todo.pop()
            for v in np.flatnonzero(Ac[u] & (f == N)):
                f[v] = r
                todo.append(v)
    return f


def labels_from_roots(A, core, f):
    """-> (labels int32 [N], n_clusters)"""
    N = len(core)
    roots = np.flatnonzero(core & (f == np.arange(N)))
    cid = np.full(N + 1, -1, dtype=np.int32)
    cid[roots] = np.arange(len(roots))
    best = np.where(A & core[None, :], f[None, :].astype(np.int64), N).min(axis=1)      # the smallest root among the core neighbours
    best[core] = f[core]
    return cid[best], len(roots)


def dbscan(A, min_samples, by_rounds=False):
    """-> {"labels", "core" (bool), "core_sample_indices", "counts", "f", "n_clusters", "n_rounds" (by_rounds)} of the
    neighbourhood matrix A (its diagonal set)"""
    cnt, core = core_rows(A, min_samples)
    out = {"counts": cnt, "core": core, "core_sample_indices": np.flatnonzero(core)}
    if by_rounds:
        fs, out["n_rounds"] = run_rounds(A, core)
        f = fs[-1]
    else:
        f = components(A, core)
    out["f"] = f
    out["labels"], out["n_clusters"] = labels_from_roots(A, core, f)
    return out


def noise_runs(labels):
    """the maximal runs of -1 as (start, stop) pairs, stop exclusive"""
    runs, t, N = [], 0, len(labels)
    while t < N:
        if labels[t] == -1:
            s = t
            while t < N and labels[t] == -1:
                t += 1
            runs.append((s, t))
        else:
            t += 1
    return runs


# ---- the graphs of the component tests ---------------------------------------------------------------------------------------

def path_graph(N, seed=None):
    """a path over N rows, its diagonal set; seed: the rows' indices randomly permuted"""
    p = np.arange(N) if seed is None else np.random.RandomState(seed).permutation(N)
    A = np.eye(N, dtype=bool)
    A[p[:-1], p[1:]] = True
    A[p[1:], p[:-1]] = True
    return A


def interleaved_chains(N):
    """two paths, over the even and over the odd rows"""
    A = np.eye(N, dtype=bool)
    i = np.arange(N - 2)
    A[i, i + 2] = True
    A[i + 2, i] = True
    return A


# name -> (neighbourhood matrix, min_samples)
GRAPHS = {"path": lambda: (path_graph(1000), 2), "path_permuted": lambda: (path_graph(1000, seed=0), 2),
          "interleaved": lambda: (interleaved_chains(301), 2), "isolated": lambda: (np.eye(130, dtype=bool), 1),
          "no_core": lambda: (path_graph(130, seed=1), 4), "one_cluster": lambda: (np.ones((200, 200), dtype=bool), 5)}


def planted_chain(N, L, K, seed, spread=0.05, bridge=6, dwell=40):
    """f32 latents [N, L] in time order: the chain dwells about `dwell` rows in one of K states (centres 4 e_k, 5.7 apart, rows
    within about 0.15 of them), then crosses to another over `bridge` evenly spaced transition rows (0.8 apart) along a path bent
    by a draw of its own, so that two crossings of one pair do not coincide -> (X, states int64 [N], transition bool [N])"""
    assert K <= L
    r = np.random.RandomState(seed)
    centres = 4.0 * np.eye(K, L)
    X = np.zeros((N, L))
    s = np.zeros(N, dtype=np.int64)
    tr = np.zeros(N, dtype=bool)
    t, k = 0, 0
    while t < N:
        n = min(N - t, dwell + int(r.randint(-dwell // 4, dwell // 4 + 1)))
        X[t:t + n] = centres[k] + spread * r.randn(n, L)
        s[t:t + n] = k
        t += n
        nxt = (k + 1 + int(r.randint(K - 1))) % K
        m = min(N - t, bridge)
        bend = r.randn(L)
        for b in range(m):
            a = (b + 1.0) / (bridge + 1.0)
            X[t + b] = (1 - a) * centres[k] + a * centres[nxt] + 4.0 * a * (1 - a) * bend + spread * r.randn(L)
            s[t + b] = k if a < 0.5 else nxt
            tr[t + b] = True
        t += m
        k = nxt
    return X.astype(np.float32), s, tr


def golden():
    return np.load(GOLDEN)


def golden_cases(g=None):
    """-> [(name, X f32 [N, L], metric, eps (Euclidean) or bits (Hamming), min_samples, labels, core_sample_indices)]"""
    g = golden() if g is None else g
    out = []
    for name in str(g["names"]).split(","):
        metric = "euclidean" if name + "/eps" in g.files else "hamming"
        out.append((name, g[name + "/X"], metric, float(g[name + "/eps"]) if metric == "euclidean" else int(g[name + "/bits"]),
                    int(g[name + "/min_samples"]), g[name + "/labels"], g[name + "/core_sample_indices"]))
    return out


def case_adjacency(X, metric, eps):
    return adjacency(X, float(eps) * float(eps)) if metric == "euclidean" else hamming_adjacency(X, eps)
