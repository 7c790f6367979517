"""Reference and element-wise bounds for the UMAP tests (csrc/umap.hip, projection.py's fuzzy_graph / umap_optimise).

An f64 numpy restatement of UMAP's fuzzy simplicial set and of one synchronous layout epoch (McInnes, Healy, Melville
2018, Algorithms 2-5, with umap-learn's published defaults), written independently of the package, and
layout_sequential: umap-learn's edge-by-edge loop in f64, moving both ends, with RandomState negatives, which
tools/make_umap_golden.py runs to record what the stochastic layout is held to.  Some functions take a `defect` name: the
restatement with one named mistake, which tests/test_umap_cpu.py uses to show that each bound below rejects it.

Formulation.  n_neighbors = k counts the point itself: the graph is knn(X, k - 1), K1 = k - 1 columns, and
d = (double)(float)sqrt(d2).
  smooth kNN   rho_i = the smallest d_ir > 0 (0 if none).  Bisection on sigma from lo = 0, hi = inf, mid = 1, at most 64
               evaluations of psum = sum_r (d_ir - rho_i > 0 ? exp(-(d_ir - rho_i) / mid) : 1) towards log2(k), stopping
               at |psum - log2 k| < 1e-5; sigma_i = max(mid, 1e-3 m), m = (sum_r d_ir) / k where rho_i > 0 and
               (sum_ir d_ir) / (N k) where rho_i = 0;  w_ir = 1 where d_ir - rho_i <= 0 or sigma_i = 0, else
               exp(-(d_ir - rho_i) / sigma_i).  rho, sigma, w are stored as f32.
  union        W = A + A^T - A o A^T, A[i, idx[i, r]] = w_ir, products in f64 from the f32 memberships, data f32.
  schedule     entries below max(W) / n_epochs dropped; period = max(W) / W, neg_period = period / negative_sample_rate,
               next = period, next_neg = neg_period, all f32.
  epoch n      alpha = 1 - n / n_epochs (f32).  Vertex i, from the epoch-start map only, adds over its active edges
               (next_e <= n)  2 clip(c D, +-4), D = y_i - y_j, c = -2ab r2^(b-1) / (a r2^b + 1) (0 at r2 = 0), and for
               q = clamp((int)((n - next_neg_e) / neg_period_e), 0, 32) samples m = (hash_u32(seed, n << 40 | e << 8 | p)
               N) >> 32, m != i:  clip(c D, +-4), D = y_i - y_m, c = 2 gamma b / ((0.001 + r2)(a r2^b + 1)) (0 at
               r2 = 0);  y_i' = y_i + alpha sum;  next_e += period_e, next_neg_e += q neg_period_e.

Bounds.  u = 2^-53 and v = 2^-24 are the unit roundoffs; every count is a worst-case first-order one, nothing was chosen
by looking at device output.
  smooth kNN   the device runs the same f64 recurrence; exp is within a few ulp and the sum over <= 127 terms has another
               order: sigma and w within 1e-12 relative of the f64 values, plus v relative for their f32 storage; rho is
               a selection, bit-equal; steps equal, except on a row where some evaluation had | |psum - target| - 1e-5 |
               or |psum - target| below 1e-12 (undecided: the stop test or the direction could go either way).  An
               evaluation with no exp term (every d_ir <= rho_i) is an exact count and decides on any implementation:
               at k = 2 psum = 1 = log2 k exactly, and the search stops at its first evaluation.
  a term       f32: dx, dy round once (v); r2 = fma(dy, dy, dx dx): 4 v.  pow(r2, e) moves by |e| 4 v through r2 and is
               itself taken at 4 ulp = 8 v.  Attraction: numerator fl(-2ab) pow(r2, b - 1): (4 |b - 1| + 8 + 1) v;
               denominator fl(fl(a pow(r2, b)) + 1): (4 b + 8 + 2) v; the division v; the product with D 2 v:
               c_term = (4 |b - 1| + 4 b + 22) v relative to the term.  A negative sample's term has fewer roundings
               ((4 b + 19) v) and is held to the same c_term.  The coefficients fl(-2ab), fl(2 gamma b), fl(b - 1),
               fl(0.001) and alpha are formed here in f32 exactly as the kernel forms them.  The clip is 1-Lipschitz.
  the sum      a lane adds an edge's attraction and its <= 32 samples from zero (33 terms), a butterfly adds the chunk of
               64 lanes (6 more), the chunk sums are added in order: chain = 33 + 6 + ceil(deg / 64).
                 b_sum = (c_term + chain v) S + tiny,  S = the same sum over |terms|
  y'           fl(y + fl(alpha sum)):  b_y = alpha b_sum + v |alpha sum| + v |y'| + tiny
  next, next_neg, the sample indices: exact f32 / integer arithmetic, bit-equal.
"""
import numpy as np

U = 2.0 ** -53
V = 2.0 ** -24
TINY = 1e-300
TINY32 = 1e-37
F32 = np.float32
MAX_SAMPLES = 32
SMOOTH_ITERS = 64
SMOOTH_TOL = 1e-5
MIN_K_DIST_SCALE = 1e-3
SMOOTH_DEFECTS = ("self_in_psum", "mean_over_k_minus_1")
EPOCH_DEFECTS = ("attraction_once", "negatives_from_new_map", "sample_may_be_self", "no_clip", "alpha_off_by_one")


# ---- curve ---------------------------------------------------------------------------------------------------------------

def find_ab(spread=1.0, min_dist=0.1):
    """umap-learn's find_ab_params: a, b of 1 / (1 + a x^(2b)) fitted to the offset exponential"""
    from scipy.optimize import curve_fit
    x = np.linspace(0.0, 3.0 * spread, 300)
    y = np.where(x < min_dist, 1.0, np.exp(-(x - min_dist) / spread))
    (a, b), _ = curve_fit(lambda x, a, b: 1.0 / (1.0 + a * x ** (2 * b)), x, y)
    return float(a), float(b)


# ---- smooth kNN distances ------------------------------------------------------------------------------------------------

def knn_dist(d2):
    return np.sqrt(np.asarray(d2, dtype=np.float64)).astype(F32).astype(np.float64)


def _psum(d, rho, mid):
    diff = d - rho[:, None]
    t = np.where(diff > 0, np.exp(-np.where(diff > 0, diff, 0.0) / mid[:, None]), 1.0)
    return np.cumsum(t, axis=1)[:, -1]


def smooth_knn(d2, defect=None):
    """-> dict: rho, sigma, w (f64, before the f32 storage), steps, mid (the bisection's last value), floored [N] bool,
    undecided [N] bool, target.  defects: "self_in_psum" (the point's own membership 1 counted in psum),
    "mean_over_k_minus_1" (the floor's mean taken over the k - 1 neighbours, not the k entries)."""
    d = knn_dist(d2)
    N, K1 = d.shape
    k = K1 + 1
    target = float(np.log2(float(k)))
    pos = d > 0
    rho = np.where(pos.any(1), np.where(pos, d, np.inf).min(1), 0.0)
    lo, hi, mid = np.zeros(N), np.full(N, np.inf), np.ones(N)
    steps, undecided = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=bool)
    extra = 1.0 if defect == "self_in_psum" else 0.0
    act = np.arange(N)
    for n in range(SMOOTH_ITERS):
        if act.size == 0:
            break
        ps = _psum(d[act], rho[act], mid[act]) + extra
        steps[act] = n + 1
        gap = np.abs(ps - target)
        rounded = (d[act] - rho[act, None] > 0).any(1)      # with no exp term psum is an exact count on any implementation
        undecided[act] |= rounded & ((np.abs(gap - SMOOTH_TOL) < 1e-12) | (gap < 1e-12))
        go = ~(gap < SMOOTH_TOL)
        up, dn = go & (ps > target), go & ~(ps > target)
        a = act[up]
        hi[a] = mid[a]
        mid[a] = (lo[a] + hi[a]) / 2.0
        a = act[dn]
        lo[a] = mid[a]
        mid[a] = np.where(np.isinf(hi[a]), 2.0 * mid[a], (lo[a] + hi[a]) / 2.0)
        act = act[go]
    kdiv = K1 if defect == "mean_over_k_minus_1" else k
    row_sum = d.astype(np.longdouble).sum(1)
    m = np.where(rho > 0, (row_sum / kdiv).astype(np.float64), float(row_sum.sum() / (N * kdiv)))
    floor = MIN_K_DIST_SCALE * m
    sigma = np.maximum(mid, floor)
    diff = d - rho[:, None]
    one = (diff <= 0) | (sigma[:, None] == 0)
    w = np.where(one, 1.0, np.exp(-np.where(one, 0.0, diff) / np.where(sigma == 0, 1.0, sigma)[:, None]))
    return {"rho": rho, "sigma": sigma, "w": w, "steps": steps, "mid": mid, "floored": mid < floor,
            "undecided": undecided, "target": target, "d": d}


def psum_at(d2, rho, sigma):
    """psum of the membership form at a given sigma: what a converged, non-floored row holds within 1e-5 of log2 k"""
    return _psum(knn_dist(d2), np.asarray(rho, dtype=np.float64), np.asarray(sigma, dtype=np.float64))


def stored(x):
    """(f64 value, bound) of an f64 quantity the device keeps within 1e-12 relative and stores as f32"""
    x = np.asarray(x, dtype=np.float64)
    return x, (1e-12 + V) * np.abs(x) + 1e-45


# ---- fuzzy union ---------------------------------------------------------------------------------------------------------

def fuzzy_dense(idx, w, defect=None):
    """W = A + A^T - A o A^T through a dense matrix, from the f32 memberships.  defect "union_is_sum": A + A^T."""
    N, K1 = idx.shape
    A = np.zeros((N, N))
    A[np.repeat(np.arange(N), K1), idx.reshape(-1)] = np.asarray(w, dtype=F32).astype(np.float64).reshape(-1)
    return A + A.T if defect == "union_is_sum" else (A + A.T) - A * A.T


def dense_to_csr(W):
    N = len(W)
    r, c = np.nonzero(W)
    indptr = np.zeros(N + 1, dtype=np.int64)
    np.add.at(indptr, r + 1, 1)
    return np.cumsum(indptr).astype(np.int32), c.astype(np.int32), W[r, c].astype(F32)


def fuzzy_csr(idx, w, defect=None):
    return dense_to_csr(fuzzy_dense(idx, w, defect))


def default_epochs(N):
    return 500 if N <= 10000 else 200


def schedule(indptr, indices, data, n_epochs, negative_sample_rate=5):
    """-> (indptr, indices, period f32, next f32, next_neg f32) of the entries that survive max(W) / n_epochs"""
    data = np.asarray(data, dtype=F32)
    N = len(indptr) - 1
    mx = data.max()
    keep = ~(data < mx / F32(n_epochs))
    rows = np.repeat(np.arange(N), np.diff(indptr))[keep]
    ip = np.zeros(N + 1, dtype=np.int64)
    np.add.at(ip, rows + 1, 1)
    period = (mx / data[keep]).astype(F32)
    neg = (period / F32(negative_sample_rate)).astype(F32)
    return np.cumsum(ip).astype(np.int32), np.asarray(indices)[keep].astype(np.int32), period, period.copy(), neg


# ---- one epoch -----------------------------------------------------------------------------------------------------------

def hash_u32(seed, idx):
    """csrc/common.h's hash_u32 on uint64 arrays"""
    idx = np.asarray(idx, dtype=np.uint64)
    C1, C2, S = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xD6E8FEB86659FD93), np.uint64(32)
    with np.errstate(over="ignore"):
        x = (idx + np.uint64(1)) * C1 + np.uint64(seed)
        x ^= x >> S
        x *= C2
        x ^= x >> S
        x *= C2
        x ^= x >> S
    return x & np.uint64(0xFFFFFFFF)


def sample_index(seed, n, e, p, N):
    key = (np.uint64(n) << np.uint64(40)) | (np.asarray(e, dtype=np.uint64) << np.uint64(8)) | np.asarray(p, dtype=np.uint64)
    return ((hash_u32(seed, key) * np.uint64(N)) >> np.uint64(32)).astype(np.int64)


def coefficients(a, b, gamma):
    """the f32 constants as the kernel forms them -> (a, b, fl(-2ab), fl(2 gamma b), fl(b - 1), fl(0.001)) as floats"""
    af, bf, gf = F32(a), F32(b), F32(gamma)
    return (float(af), float(bf), float(F32(F32(-2.0) * af) * bf), float(F32(F32(2.0) * gf) * bf),
            float(bf - F32(1.0)), float(F32(0.001)))


def epoch(Y, indptr, indices, period, nxt, nxt_neg, n, n_epochs, a, b, gamma=1.0, negative_sample_rate=5, seed=42,
          defect=None):
    """One synchronous epoch from the f32 map Y -> dict: Y (f64 reference of Y_out), b_y (its bound), next, next_neg
    (f32, exact), q [E] and samples [E, 32] (the sampled vertex, -1 for an unused slot or a skipped self), alpha, S.
    defects: EPOCH_DEFECTS."""
    Y32 = np.asarray(Y, dtype=F32)
    Yd = Y32.astype(np.float64)
    N = len(Yd)
    indptr, indices = np.asarray(indptr), np.asarray(indices).astype(np.int64)
    deg = np.diff(indptr)
    rows = np.repeat(np.arange(N), deg)
    E = len(indices)
    a_, b_, m2ab, g2b, bm1, milli = coefficients(a, b, gamma)
    nf = F32(n)
    alpha = float(F32(1.0) - F32(n + 1 if defect == "alpha_off_by_one" else n) / F32(n_epochs))
    period, nxt, nxt_neg = (np.asarray(x, dtype=F32) for x in (period, nxt, nxt_neg))
    active = nxt <= nf
    negp = (period / F32(negative_sample_rate)).astype(F32)
    with np.errstate(invalid="ignore", divide="ignore"):
        qf = ((nf - nxt_neg).astype(F32) / negp).astype(F32)
    qf = np.where(np.isnan(qf), F32(0.0), qf)
    q = np.where(active, np.clip(qf, 0.0, float(MAX_SAMPLES)).astype(np.int64), 0)
    clip = (lambda t: t) if defect == "no_clip" else (lambda t: np.clip(t, -4.0, 4.0))

    def attract(src):
        d = Yd[rows] - src[indices]
        r2 = (d * d).sum(1)
        s = np.where(r2 > 0, r2, 1.0)
        c = np.where(r2 > 0, m2ab * s ** bm1 / (a_ * s ** b_ + 1.0), 0.0)
        return (1.0 if defect == "attraction_once" else 2.0) * clip(c[:, None] * d) * active[:, None]

    samples = np.full((E, MAX_SAMPLES), -1, dtype=np.int64)
    e_all = np.arange(E)
    for p in range(MAX_SAMPLES):
        use = p < q
        m = sample_index(seed, n, e_all, p, N)
        if defect != "sample_may_be_self":
            use = use & (m != rows)
        samples[use, p] = m[use]

    def repel(src):
        tot, S = np.zeros((E, 2)), np.zeros((E, 2))
        for p in range(MAX_SAMPLES):
            use = samples[:, p] >= 0
            if not use.any():
                continue
            d = Yd[rows] - src[np.where(use, samples[:, p], 0)]
            r2 = (d * d).sum(1)
            s = np.where(r2 > 0, r2, 1.0)
            c = np.where(r2 > 0, g2b / ((milli + s) * (a_ * s ** b_ + 1.0)), 0.0)
            t = clip(c[:, None] * d) * use[:, None]
            tot += t
            S += np.abs(t)
        return tot, S

    def total(src_neg):
        att = attract(Yd)
        rep, S_rep = repel(src_neg)
        tot, S = np.zeros((N, 2)), np.zeros((N, 2))
        np.add.at(tot, rows, att + rep)
        np.add.at(S, rows, np.abs(att) + S_rep)
        return tot, S

    tot, S = total(Yd)
    if defect == "negatives_from_new_map":
        tot, S = total(Yd + alpha * tot)
    Yn = Yd + alpha * tot
    c_term = (4.0 * abs(bm1) + 4.0 * b_ + 22.0) * V
    chain = (33.0 + 6.0 + np.ceil(deg / 64.0))[:, None]
    b_sum = (c_term + chain * V) * S + TINY32
    b_y = alpha * b_sum + V * np.abs(alpha * tot) + V * np.abs(Yn) + TINY32
    new_next = np.where(active, (nxt + period).astype(F32), nxt).astype(F32)
    new_neg = np.where(active, (nxt_neg + (q.astype(F32) * negp).astype(F32)).astype(F32), nxt_neg).astype(F32)
    return {"Y": Yn, "b_y": b_y, "next": new_next, "next_neg": new_neg, "q": q, "samples": samples, "alpha": alpha,
            "S": S, "active": active}


def activations(period, n_epochs):
    """next after running the f32 state of every edge through epochs 0 .. n_epochs - 1, and the activation counts"""
    period = np.asarray(period, dtype=F32)
    nxt, count = period.copy(), np.zeros(len(period), dtype=np.int64)
    for n in range(n_epochs):
        act = nxt <= F32(n)
        count += act
        nxt = np.where(act, (nxt + period).astype(F32), nxt).astype(F32)
    return nxt, count


# ---- the whole layout ----------------------------------------------------------------------------------------------------

def initial_map(pca_embedding, seed=42):
    """the exact PCA scaled by 10 / max |.|, plus RandomState(seed).normal(scale=1e-4), each column min-max scaled to
    [0, 10], in f64, cast to f32"""
    Y = np.asarray(pca_embedding, dtype=np.float64)
    Y = Y * (10.0 / np.abs(Y).max())
    Y = Y + np.random.RandomState(seed).normal(scale=1e-4, size=Y.shape)
    lo, hi = Y.min(0), Y.max(0)
    return (10.0 * (Y - lo) / (hi - lo)).astype(F32)


def layout_sequential(Y0, indptr, indices, period, n_epochs, a, b, gamma=1.0, negative_sample_rate=5, seed=42):
    """umap-learn's optimize_layout_euclidean, single thread, in f64: edge by edge on the live map, both ends of an edge
    moved, negatives from RandomState(seed).  Plain Python floats: well under a minute for the 320-row fixture."""
    N = len(Y0)
    x, y = [float(v) for v in Y0[:, 0]], [float(v) for v in Y0[:, 1]]
    head = np.repeat(np.arange(N), np.diff(indptr)).tolist()
    tail = [int(j) for j in indices]
    eps = [float(p) for p in period]
    epn = [p / negative_sample_rate for p in eps]
    nxt, nneg = list(eps), list(epn)
    E = len(tail)
    rs = np.random.RandomState(seed)
    m2ab, g2b, bm1 = -2.0 * a * b, 2.0 * gamma * b, b - 1.0

    def clip(t):
        return 4.0 if t > 4.0 else (-4.0 if t < -4.0 else t)

    for n in range(n_epochs):
        alpha = 1.0 - n / n_epochs
        draws, dp = rs.randint(0, N, size=8 * E).tolist(), 0
        for e in range(E):
            if nxt[e] > n:
                continue
            i, j = head[e], tail[e]
            dx, dy = x[i] - x[j], y[i] - y[j]
            r2 = dx * dx + dy * dy
            c = m2ab * r2 ** bm1 / (a * r2 ** b + 1.0) if r2 > 0.0 else 0.0
            gx, gy = clip(c * dx) * alpha, clip(c * dy) * alpha
            x[i] += gx
            y[i] += gy
            x[j] -= gx
            y[j] -= gy
            nxt[e] += eps[e]
            q = int((n - nneg[e]) / epn[e])
            for _ in range(q):
                if dp == len(draws):
                    draws, dp = rs.randint(0, N, size=8 * E).tolist(), 0
                m = draws[dp]
                dp += 1
                if m == i:
                    continue
                dx, dy = x[i] - x[m], y[i] - y[m]
                r2 = dx * dx + dy * dy
                if r2 > 0.0:
                    c = g2b / ((0.001 + r2) * (a * r2 ** b + 1.0))
                    x[i] += clip(c * dx) * alpha
                    y[i] += clip(c * dy) * alpha
            nneg[e] += q * epn[e]
    return np.stack([np.array(x), np.array(y)], axis=1)


def cross_entropy(Y, indptr, indices, data, a, b):
    """sum_{i<j} [w log(w / v) + (1 - w) log((1 - w) / (1 - v))], v = 1 / (1 + a r^(2b)), over all pairs in f64; a term
    with w = 0 or w = 1 keeps its other half only, and v is kept below 1 - 2^-53 (a coincident pair costs a finite 36.7)"""
    Y = np.asarray(Y, dtype=np.float64)
    N = len(Y)
    W = np.zeros((N, N))
    W[np.repeat(np.arange(N), np.diff(indptr)), indices] = np.asarray(data, dtype=np.float64)
    d = Y[:, None, :] - Y[None, :, :]
    r2 = (d * d).sum(-1)
    v = np.minimum(1.0 / (1.0 + a * r2 ** b), 1.0 - U)
    iu = np.triu_indices(N, 1)
    w, v = W[iu], v[iu]
    t1 = np.where(w > 0, w * np.log(np.where(w > 0, w, 1.0) / v), 0.0)
    t2 = np.where(w < 1, (1.0 - w) * np.log(np.where(w < 1, 1.0 - w, 1.0) / (1.0 - v)), 0.0)
    return float((t1 + t2).sum())


# ---- helpers -------------------------------------------------------------------------------------------------------------

def star_graph(N, seed=0):
    """vertex 0 joined to every other vertex, and a ring through the others: the hub's row has N - 1 edges (several
    chunks of 64), symmetric weights in (0, 1] with the largest exactly 1"""
    r = np.random.RandomState(seed)
    W = np.zeros((N, N))
    W[0, 1:] = 0.2 + 0.8 * r.rand(N - 1)
    for i in range(1, N):
        W[i, 1 + i % (N - 1)] = 0.2 + 0.8 * r.rand()
    W = np.maximum(W, W.T)
    np.fill_diagonal(W, 0.0)
    W[0, 1] = W[1, 0] = 1.0
    return dense_to_csr(W.astype(F32).astype(np.float64))


def state_at(period, n, negative_sample_rate=5):
    """(next, next_neg) f32 as they stand before epoch n: the schedule's arithmetic alone, which no position enters"""
    period = np.asarray(period, dtype=F32)
    negp = (period / F32(negative_sample_rate)).astype(F32)
    nxt, neg = period.copy(), negp.copy()
    for m in range(n):
        mf = F32(m)
        act = nxt <= mf
        q = np.clip(((mf - neg).astype(F32) / negp).astype(F32), 0.0, float(MAX_SAMPLES)).astype(np.int64)
        neg = np.where(act, (neg + (q.astype(F32) * negp).astype(F32)).astype(F32), neg).astype(F32)
        nxt = np.where(act, (nxt + period).astype(F32), nxt).astype(F32)
    return nxt, neg


def hard_codes_k15():
    """_projection_ref.hard_codes(): 160 hard 0/1 codes, 9 distinct: at n_neighbors = 15 some rows have 14 exact duplicates
    (rho = 0) and others enough ties at their smallest positive distance to be floored by their own mean"""
    from _projection_ref import hard_codes
    return hard_codes()
