"""The f64 restatement of csrc/hdbscan.hip: HDBSCAN* (Campello, Moulavi, Zimek, Sander 2015, Algorithm 1 with "edges of equal
weight are removed simultaneously") in an order-free form.  scikit-learn 1.7.2 is the reference wherever its answer is well
defined -- the MST weights, every cut, the cases without structural ties -- and tests/golden/hdbscan.npz records it.

  d2(i, j)        _dbscan_ref.d2_matrix: rbvae_knn's f64 sum
  core2_i         the (m - 1)-th smallest d2(i, j) over j != i; 0 for m = 1 (min_samples = m counts the row itself)
  w2(i, j)        max(core2_i, core2_j, d2(i, j)); edges ordered by the key (w2, lo, hi): a strict total order, so the minimum
                  spanning tree is unique (mst: Kruskal under that key)
  levels          the distinct d = sqrt(w2) of the tree's edges, ascending; lambda = 1 / d, inf at d = 0
  dendrogram      all edges of a level at once; a component that absorbed r >= 2 older ones is one node with r children
  condensed tree  top down from the root cluster (born at 0): a child is big when it has >= mcs rows; >= 2 big children end C
                  and each starts a cluster born at lambda; exactly 1 continues C; 0 end C; the other children's rows leave C
  stability       sum over C's levels, lambda ascending, of (lambda - birth) * n, n the whole number of rows leaving (the big
                  children's at a split included): one product and one add per level
  lambda_max      C's last level
  selection       "eom": deepest first, root excluded: children summing to MORE than C drop C, which takes the sum; otherwise C
                  is selected and its descendants dropped.  "leaf": the clusters without children.  The root is never selected
  labels          the nearest selected cluster from the one a row left upwards, else -1; ids by ascending smallest row
  probability     0 for -1; 1 if lambda_max == 0 or the row's lambda is inf; else min(lambda_row, lambda_max) / lambda_max
  cut             the components of the edges with d <= cut; fewer than mcs rows: -1; ids by ascending smallest row
The cluster table stands in (birth, smallest row) order, the root first.  `defect` switches one rule to a named wrong form, for
the tests that show the gates reject it.
"""
import math
import os

import numpy as np

import _dbscan_ref as D

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hdbscan.npz")
DEFECTS = ("binary", "eom_ge", "lmax_descendants", "core_off_by_one")
TABLE = ("parent", "birth", "lambda_max", "stability", "size", "selected", "min_row")


def core2(D2, m, defect=None):
    """f64 [N]: column m - 2 of rbvae_knn(X, m - 1)"""
    if defect == "core_off_by_one":
        m = m + 1
    N = len(D2)
    if m == 1:
        return np.zeros(N)
    off = D2.copy()
    np.fill_diagonal(off, np.inf)
    return np.sort(off, axis=1)[:, m - 2]


def mutual_reachability2(D2, c2):
    return np.maximum(np.maximum(c2[:, None], c2[None, :]), D2)


def _find(f, x):
    while f[x] != x:
        f[x] = f[f[x]]
        x = f[x]
    return x


def mst(W2):
    """Kruskal under (w2, lo, hi) -> (edges int32 [N - 1, 2] with lo < hi, w2 f64 [N - 1]) in ascending key order"""
    N = len(W2)
    lo, hi = np.triu_indices(N, 1)
    w = W2[lo, hi]
    k = min(len(w), 8 * N)
    while True:                                         # Kruskal over the edges up to a bound is a prefix of the whole run
        bound = np.partition(w, k - 1)[k - 1] if k < len(w) else np.inf
        some = np.flatnonzero(w <= bound)
        order = some[np.lexsort((hi[some], lo[some], w[some]))]
        f = list(range(N))
        E, Wt = [], []
        for e in order:
            a, b = _find(f, int(lo[e])), _find(f, int(hi[e]))
            if a != b:
                f[a] = b
                E.append((int(lo[e]), int(hi[e])))
                Wt.append(w[e])
                if len(E) == N - 1:
                    break
        if len(E) == N - 1 or k >= len(w):
            break
        k = min(len(w), 4 * k)
    assert len(E) == N - 1
    return np.array(E, dtype=np.int32).reshape(-1, 2), np.array(Wt, dtype=np.float64)


def mst_of(X, m, defect=None):
    """-> (edges, w2, core2) of the f32 matrix X"""
    D2 = D.d2_matrix(X)
    c2 = core2(D2, m, defect)
    return mst(mutual_reachability2(D2, c2)) + (c2,)


def _dendrogram(edges, d, N, binary=False):
    """-> (size, minrow, children, dist, root): nodes 0 .. N - 1 are the rows"""
    size, minrow, children, dist = [1] * N, list(range(N)), [[] for _ in range(N)], [0.0] * N
    f, nodeof = list(range(N)), list(range(N))
    e = 0
    while e < N - 1:
        g = e + 1
        while not binary and g < N - 1 and d[g] == d[e]:
            g += 1
        olds, seen = [], set()
        for k in range(e, g):
            for x in edges[k]:
                r = _find(f, int(x))
                if r not in seen:
                    seen.add(r)
                    olds.append(r)
        oldnodes = [nodeof[r] for r in olds]
        for k in range(e, g):
            a, b = _find(f, int(edges[k][0])), _find(f, int(edges[k][1]))
            f[a] = b
        new = {}
        for r, ch in zip(olds, oldnodes):
            nr = _find(f, r)
            if nr not in new:
                new[nr] = len(size)
                size.append(0)
                minrow.append(N)
                children.append([])
                dist.append(float(d[e]))
            v = new[nr]
            size[v] += size[ch]
            minrow[v] = min(minrow[v], minrow[ch])
            children[v].append(ch)
        for nr, v in new.items():
            nodeof[nr] = v
        e = g
    return size, minrow, children, dist, len(size) - 1


def tree(edges, d, N, mcs, method="eom", defect=None):
    """-> {"labels" int32 [N], "prob" f64 [N], "n_clusters", "table": {name: array over the clusters, TABLE's names}}"""
    assert method in ("eom", "leaf") and 2 <= mcs <= N and len(edges) == N - 1
    size, minrow, children, dist, root = _dendrogram(edges, d, N, binary=defect == "binary")
    parent, csize, cmin, birth, lmax, stab = [-1], [N], [0], [0.0], [0.0], [0.0]
    row_cl, row_lam = [0] * N, [0.0] * N
    todo = [(root, 0)]
    while todo:
        v, C = todo.pop()
        lam = math.inf if dist[v] == 0.0 else 1.0 / dist[v]
        leaving, big = 0, []
        for ch in children[v]:
            if size[ch] >= mcs:
                big.append(ch)
                continue
            leaving += size[ch]
            walk = [ch]
            while walk:
                x = walk.pop()
                if x < N:
                    row_cl[x], row_lam[x] = C, lam
                walk.extend(children[x])
        if len(big) >= 2:
            for ch in big:
                leaving += size[ch]
                todo.append((ch, len(parent)))
                parent.append(C)
                csize.append(size[ch])
                cmin.append(minrow[ch])
                birth.append(lam)
                lmax.append(0.0)
                stab.append(0.0)
        elif len(big) == 1:
            todo.append((big[0], C))
        stab[C] = stab[C] + (lam - birth[C]) * float(leaving)
        lmax[C] = lam
    K = len(parent)
    order = sorted(range(K), key=lambda c: (birth[c], cmin[c]))
    rank = {c: k for k, c in enumerate(order)}
    tp = [-1 if parent[c] < 0 else rank[parent[c]] for c in order]
    kids = [[] for _ in range(K)]
    for k in range(1, K):
        kids[tp[k]].append(k)
    sel = [0] * K
    tl = [lmax[c] for c in order]
    if defect == "lmax_descendants":
        for k in range(K - 1, 0, -1):
            tl[tp[k]] = max(tl[tp[k]], tl[k])
    if method == "eom":
        s = [stab[c] for c in order]
        for k in range(K - 1, 0, -1):
            sel[k] = 1
            if kids[k]:
                total = 0.0
                for q in kids[k]:
                    total = total + s[q]
                if total > s[k] or (defect == "eom_ge" and total == s[k]):
                    s[k], sel[k] = total, 0
        covered = [False] * K
        for k in range(1, K):
            covered[k] = bool(sel[tp[k]]) or covered[tp[k]]
            if covered[k]:
                sel[k] = 0
    else:
        for k in range(1, K):
            sel[k] = int(not kids[k])
    anc = [-1] * K
    for k in range(1, K):
        anc[k] = k if sel[k] else anc[tp[k]]
    chosen = sorted((k for k in range(1, K) if sel[k]), key=lambda k: cmin[order[k]])
    cid = {k: q for q, k in enumerate(chosen)}
    labels, prob = np.full(N, -1, dtype=np.int32), np.zeros(N)
    for i in range(N):
        a = anc[rank[row_cl[i]]]
        if a < 0:
            continue
        labels[i] = cid[a]
        lm, lr = tl[a], row_lam[i]
        prob[i] = 1.0 if lm == 0.0 or math.isinf(lr) else min(lr, lm) / lm
    table = {"parent": np.array(tp, dtype=np.int32), "birth": np.array([birth[c] for c in order]),
             "lambda_max": np.array(tl), "stability": np.array([stab[c] for c in order]),
             "size": np.array([csize[c] for c in order], dtype=np.int32), "selected": np.array(sel, dtype=np.int32),
             "min_row": np.array([cmin[c] for c in order], dtype=np.int32)}
    return {"labels": labels, "prob": prob, "n_clusters": len(chosen), "table": table}


def cut(edges, d, N, cut_distance, mcs):
    """-> (labels int32 [N], n_clusters)"""
    f, size = list(range(N)), [1] * N
    for (a, b), w in zip(edges, d):
        if not w <= cut_distance:
            break
        a, b = _find(f, int(a)), _find(f, int(b))
        f[a] = b
        size[b] += size[a]
    labels, ids = np.full(N, -1, dtype=np.int32), {}
    for i in range(N):
        r = _find(f, i)
        if size[r] >= mcs:
            labels[i] = ids.setdefault(r, len(ids))
    return labels, len(ids)


def hdbscan(X, mcs, m=None, method="eom", defect=None):
    """the whole fit of the f32 matrix X -> tree()'s dict with "edges", "d", "core2" added"""
    m = mcs if m is None else m
    edges, w2, c2 = mst_of(X, m, defect)
    d = np.sqrt(w2)
    out = tree(edges, d, len(X), mcs, method, defect)
    out.update(edges=edges, d=d, core2=c2)
    return out


def same_partition(a, b):
    """two label vectors name the same partition, -1 meaning the same rows in both"""
    a, b = np.asarray(a), np.asarray(b)
    if not np.array_equal(a < 0, b < 0):
        return False
    fwd, back = {}, {}
    for x, y in zip(a.tolist(), b.tolist()):
        if fwd.setdefault(x, y) != y or back.setdefault(y, x) != x:
            return False
    return True


def same_fit(a, b):
    """labels, probabilities and the cluster table bit for bit"""
    return (np.array_equal(a["labels"], b["labels"]) and np.array_equal(a["prob"].view(np.int64), b["prob"].view(np.int64)) and
            all(np.array_equal(np.ascontiguousarray(a["table"][k]).view(np.uint8), np.ascontiguousarray(b["table"][k]).view(np.uint8))
                and a["table"][k].dtype == b["table"][k].dtype for k in TABLE))


# ---- the data of the tests -----------------------------------------------------------------------------------------------

def blobs(N, L, K, seed, bridges=2):
    """f32 [N, L]: K planted blobs of unequal spread, `bridges` thin rows of points between consecutive centres, rows shuffled"""
    r = np.random.RandomState(seed)
    centres = 6.0 * r.randn(K, L) / np.sqrt(L) * np.sqrt(max(L, 2) / 2.0)
    nb = min(bridges, K - 1) * 8
    which = r.randint(K, size=N - nb)
    X = centres[which] + (0.3 + 0.5 * r.rand(K))[which, None] * r.randn(N - nb, L) / np.sqrt(L)
    B = []
    for b in range(min(bridges, K - 1)):
        a = (np.arange(8) + 1.0) / 9.0
        B.append((1 - a)[:, None] * centres[b] + a[:, None] * centres[b + 1] + 0.02 * r.randn(8, L))
    X = np.concatenate([X] + B) if B else X
    return X[r.permutation(len(X))].astype(np.float32)


def pairing_gaps(N, seed=0):
    """f32 [N, 1], rows shuffled: gap i of the sorted positions is 1 + trailing_zeros(i + 1) + i / 2^20 before the positions
    round to f32, so the components pair up round by round (the reference is mst_of on the rounded matrix)"""
    i = np.arange(N - 1)
    tz = np.array([(int(v) & -int(v)).bit_length() - 1 for v in i + 1], dtype=np.float64)
    pos = np.concatenate(([0.0], np.cumsum(1.0 + tz + i / 2.0 ** 20)))
    X = np.empty((N, 1), dtype=np.float32)
    X[np.random.RandomState(seed).permutation(N), 0] = pos.astype(np.float32)
    return X


def increasing_gaps(N, seed=0):
    """f32 [N, 1], rows shuffled: the sorted positions are 1.005^k rounded to f32, whose gaps (exact in f64) still increase
    strictly, so for m = 1 the tree is the consecutive pairs -> (X, edges, w2) in key order, in closed form"""
    x32 = (1.005 ** np.arange(N)).astype(np.float32)
    pos = x32.astype(np.float64)
    gap = pos[1:] - pos[:-1]
    assert (gap[1:] > gap[:-1]).all() and gap[0] > 0
    perm = np.random.RandomState(seed).permutation(N)
    X = np.empty((N, 1), dtype=np.float32)
    X[perm, 0] = x32                                    # sorted position k sits in row perm[k]
    a, b = perm[:-1], perm[1:]
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    return X, np.stack([lo, hi], axis=1).astype(np.int32), gap * gap      # the gaps ascend: this is the key order


def chain_tree(N):
    """a chain dendrogram N deep: edge e joins row e + 1 to the rows before it at distance e + 1"""
    e = np.arange(N - 1, dtype=np.int32)
    return np.stack([e, e + 1], axis=1), (e + 1).astype(np.float64)


def golden():
    return np.load(GOLDEN)


def golden_cases(g=None):
    """-> [dict(name, X, m, mcs, agrees, labels, prob, n_clusters, mst_w, cuts=[(cut_distance, labels)])]"""
    g = golden() if g is None else g
    out = []
    for name in str(g["names"]).split(","):
        c = {k: g[f"{name}/{k}"] for k in ("X", "labels", "prob", "mst_w")}
        c.update(name=name, m=int(g[name + "/m"]), mcs=int(g[name + "/mcs"]), agrees=bool(g[name + "/agrees"]),
                 n_clusters=int(g[name + "/n_clusters"]),
                 cuts=[(float(e), g[f"{name}/cut{q}"]) for q, e in enumerate(g[name + "/cut_distances"])])
        out.append(c)
    return out
