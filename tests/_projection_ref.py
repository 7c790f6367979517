"""Reference and element-wise bounds for the projection tests (csrc/project.hip, projection.py).

An f64 numpy restatement of the kNN graph, t-SNE's perplexity search, joint distribution, gradient and update, and the
exact PCA, written independently of the package; tests/golden/projection.npz (tools/make_projection_golden.py) pins it
to scikit-learn 1.7.2.  Some functions take a `defect` name: the restatement with one named mistake, which
tests/test_projection_cpu.py uses to show that each bound below rejects that mistake.

Bounds.  u = 2^-53 (f64) and v = 2^-24 (f32) are the unit roundoffs; a sum of n terms in ANY order is off by at most
(n - 1) x roundoff x sum |terms| to first order.  Every constant below is a worst-case first-order count (each rounding
taken at its full half ulp, all with the same sign); the second-order terms are of the size (300 v)^2 ~ 3e-10 relative
and sit far inside that pessimism.  Nothing was chosen by looking at device output.
  d2          sum_l (x_il - x_jl)^2: the differences are exact in f64, each square rounds once, L additions of positive
              terms: |got - ref| <= (L + 1) u ref.  Neighbour order is only required where it is decided: consecutive
              sorted distances of a row, among its first k + 1, are equal or differ by >= 1e-12 relative (decided_rows).
  perplexity  the restatement runs the same f64 recurrence; exp / log are within a few ulp and the two sums over k <= 128
              terms have another order: P and beta within 1e-12 relative, steps equal, except on a row where an
              evaluation came within 1e-9 of the tolerance test's threshold (near_tolerance), which may stop one step
              apart.
  repulsion   per pair, f32: dx, dy round once (v each, relative to themselves), dx^2 (v), the fma (v), 1 + d (v): the
              denominator is off by <= 5 v relative; the hardware reciprocal is within 1 ulp = 2 v, so q within 7 v; a term
              of Z is q: 7 v.  A term of R is q^2 dx: 14 v + v (the square) + v (dx): 16 v; its fma rounding belongs to
              the chain.  c_rcp = 16 v.  Chain: a lane adds the <= 256 pairs of a chunk from zero, then the chunk sums of
              its slice, and the step kernel adds the slices: c_chain = (256 + chunks_per_slice + splits) v.
                |got - ref| <= (c_chain + c_rcp) S + tiny,   S = the same sum over |terms|
  gradient    from the device's own partial sums and Z.  A term p q dx of the attraction: p = exaggeration x data (v), q
              by an IEEE division of a 5 v denominator (6 v), the product (v), dx (v): 9 v; a lane adds <= ceil(deg / 64)
              terms, the wave 6 more.  R adds `splits` f32 partials.  g = 4 fl32(A - R / Z), the inner expression in f64:
              the rounding to f32 costs v |g|, the f64 operations inside are below v^2:
                b_g = 4 [(9 + ceil(deg / 64) + 6) v S_A + splits v S_R / Z] + v |g| + tiny
  update      gains are exact f32 arithmetic once the sign of update x g is known: identical unless |g| <= b_g (and
              update != 0).  update' = fl(fl(m u) - fl(lr fl(gains g))): m u rounds once, gains g and its product with lr
              once each, and the difference once, by v (|m u| + |lr gains g|):
              b_u = lr gains b_g + v (2 |m u| + 3 |lr gains g|);  y' = fl(y + update'): b_y = b_u + v |y'|.
  KL, |g|^2   a KL term p log(p Z / q) moves by 6 v p through q and by v p (|log| + 1) through p:
              b_KL = v sum p (7 + |log|) + n u sum |terms|;  b_gg = sum (2 |g| b_g + b_g^2) + n u sum g^2; the sum of
              |gains g|^2 likewise, with 2 v more for the f32 product gains g that is squared.
  moments     from the device's own mean: centring rounds once per value, the product once, N additions, one division:
              (N + 2) u S with S = sum |a b| / (N - 1); the mean itself: (N + 1) u sum |x| / N.
"""
import numpy as np

U = 2.0 ** -53
V = 2.0 ** -24
TINY = 1e-300
TINY32 = 1e-37
LD = np.longdouble
FLT_MIN = float(np.finfo(np.float32).tiny)
RP_TI = RP_JC = 256                     # the repulsion kernel's tile of i rows and chunk of j points


# ---- kNN -------------------------------------------------------------------------------------------------------------

def sqdist(X):
    """[N, N] f64: sum_l (x_il - x_jl)^2 with l ascending, each square rounded once (the kernel's order)"""
    X = np.asarray(X, dtype=np.float32).astype(np.float64)
    D = np.zeros((len(X), len(X)))
    for l in range(X.shape[1]):
        df = X[:, None, l] - X[None, :, l]
        D += df * df
    return D


def knn(X, k, defect=None, D=None):
    """-> (idx [N, k], d2 [N, k], decided [N] bool): neighbours sorted by (d2, j), self excluded.
    defect "tie_high": ties go to the higher index."""
    D = sqdist(X) if D is None else D
    N = len(D)
    Dx = D.copy()
    Dx[np.arange(N), np.arange(N)] = np.inf
    j = np.broadcast_to(np.arange(N), (N, N))
    order = np.lexsort(((-j if defect == "tie_high" else j), Dx), axis=1)
    srt = np.take_along_axis(Dx, order, axis=1)
    head = srt[:, :min(k + 1, N - 1)]
    gap = np.diff(head, axis=1)
    decided = np.all((gap == 0) | (gap >= 1e-12 * head[:, 1:]), axis=1)
    return order[:, :k].astype(np.int32), srt[:, :k], decided


def smallest_relative_gap(X, k):
    """the smallest non-zero relative gap between consecutive sorted distances among each row's first k + 1"""
    D = sqdist(X)
    np.fill_diagonal(D, np.inf)
    head = np.sort(D, axis=1)[:, :k + 1]
    gap = np.diff(head, axis=1) / head[:, 1:]
    return float(gap[gap > 0].min())


# ---- perplexity search -------------------------------------------------------------------------------------------------

def _seqsum(a):
    return np.cumsum(a, axis=1)[:, -1]                      # j ascending, as the .pyx adds


def perplexity_search(d2, perplexity):
    """sklearn.manifold._utils._binary_search_perplexity restated on all rows at once.
    -> (P [N, k], beta [N] (the value P was evaluated at), steps [N] (entropy evaluations), near_tolerance [N] bool)"""
    d = np.asarray(d2).astype(np.float32).astype(np.float64)
    N, k = d.shape
    want = np.log(np.float64(np.float32(perplexity)))
    tol, eps = float(np.float32(1e-5)), float(np.float32(1e-8))
    beta, bmin, bmax = np.ones(N), np.full(N, -np.inf), np.full(N, np.inf)
    P, used = np.zeros((N, k)), np.ones(N)
    steps, near = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=bool)
    act = np.arange(N)
    for l in range(100):
        if act.size == 0:
            break
        b = beta[act]
        p = np.exp(-d[act] * b[:, None])
        s = _seqsum(p)
        s[s == 0.0] = eps
        p = p / s[:, None]
        diff = (np.log(s) + b * _seqsum(d[act] * p)) - want
        P[act], used[act], steps[act] = p, b, l + 1
        near[act] |= np.abs(np.abs(diff) - tol) < 1e-9
        go = np.abs(diff) > tol
        up = go & (diff > 0)
        dn = go & ~(diff > 0)
        a_up, a_dn = act[up], act[dn]
        bmin[a_up] = beta[a_up]
        beta[a_up] = np.where(np.isinf(bmax[a_up]), beta[a_up] * 2.0, (beta[a_up] + bmax[a_up]) / 2.0)
        bmax[a_dn] = beta[a_dn]
        beta[a_dn] = np.where(np.isinf(bmin[a_dn]), beta[a_dn] / 2.0, (beta[a_dn] + bmin[a_dn]) / 2.0)
        act = act[go]
    return P, used, steps, near


def joint_csr(idx, P):
    """_joint_probabilities_nn's symmetrised, normalised P through a dense matrix -> (indptr, indices, data f64)"""
    N, k = idx.shape
    M = np.zeros((N, N))
    M[np.repeat(np.arange(N), k), idx.reshape(-1)] = P.reshape(-1)
    J = M + M.T
    J /= max(J.sum(), np.finfo(np.float64).eps)
    r, c = np.nonzero(J)
    indptr = np.zeros(N + 1, dtype=np.int32)
    np.add.at(indptr, r + 1, 1)
    return np.cumsum(indptr).astype(np.int32), c.astype(np.int32), J[r, c]


# ---- repulsion ---------------------------------------------------------------------------------------------------------

def repulse_shape(N):
    """(splits, slice length, chunks per slice) as rbvae_tsne_repulse_splits lays the j range out"""
    tiles, chunks = -(-N // RP_TI), -(-N // RP_JC)
    s = min(-(-1024 // tiles), chunks)
    per = -(-chunks // s)
    return -(-chunks // per), per * RP_JC, per


def repulsion(Y, defect=None):
    """-> (R [N, 2], Zi [N], S_R [N, 2], S_Z [N]) in f64 from the f32 map Y; S_* the sums over |terms|.
    defects: "self_in_z" (the j = i term counted in Z), "drop_tail" (the last partial chunk of j left out),
    "drop_split" (the last j slice left out of the combination)."""
    Y = np.asarray(Y, dtype=np.float32).astype(np.float64)
    N = len(Y)
    d = Y[:, None, :] - Y[None, :, :]
    q = 1.0 / (1.0 + (d * d).sum(-1))
    keep = np.ones((N, N))
    if defect != "self_in_z":
        np.fill_diagonal(keep, 0.0)
    if defect == "drop_tail":
        keep[:, (N // RP_JC) * RP_JC:] = 0.0
    if defect == "drop_split":
        splits, slc, _ = repulse_shape(N)
        keep[:, (splits - 1) * slc:] = 0.0
    q = q * keep
    R = ((q * q)[:, :, None] * d).sum(1)
    S_R = ((q * q)[:, :, None] * np.abs(d)).sum(1)
    Zi = q.sum(1)
    return R, Zi, S_R, Zi.copy()


def repulsion_bound(N, S):
    splits, _, per = repulse_shape(N)
    return ((RP_JC + per + splits) * V + 16.0 * V) * S + TINY32


# ---- gradient and update -----------------------------------------------------------------------------------------------

def attraction(Y, indptr, indices, data, exaggeration, Z):
    """-> (A [N, 2], S_A [N, 2], kl terms per edge, p per edge, deg [N]) in f64; p = fl32(exaggeration x data)"""
    Y = np.asarray(Y, dtype=np.float32).astype(np.float64)
    N = len(Y)
    rows = np.repeat(np.arange(N), np.diff(indptr))
    p = (np.float32(exaggeration) * np.asarray(data, dtype=np.float32)).astype(np.float64)
    d = Y[rows] - Y[indices]
    q = 1.0 / (1.0 + (d * d).sum(-1))
    w = (p * q)[:, None] * d
    A, S_A = np.zeros((N, 2)), np.zeros((N, 2))
    np.add.at(A, rows, w)
    np.add.at(S_A, rows, np.abs(w))
    klt = p * np.log(np.maximum(p, FLT_MIN) / np.maximum(q / Z, FLT_MIN))
    return A, S_A, klt, p, np.diff(indptr)


def gradient(Y, indptr, indices, data, exaggeration=1.0, R=None, Z=None):
    """-> (g [N, 2], KL) in f64: _kl_divergence_bh(angle=0)'s gradient and error.  R, Z default to the exact f64
    repulsion of Y."""
    if R is None:
        R, Zi, _, _ = repulsion(Y)
        Z = Zi.sum()
    A, _, klt, _, _ = attraction(Y, indptr, indices, data, exaggeration, Z)
    return 4.0 * (A - R / Z), float(klt.sum())


def step(Y, update, gains, indptr, indices, data, sched, part, Z, defect=None):
    """One rbvae_tsne_step from the device's own partial sums part [splits, N, 3] (f32) and Z.
    -> dict of references (g, gains, update, Y, gg, sgg, kl) and bounds (b_g, b_u, b_y, b_gg, b_kl), and `free`: where
    the sign of update x g is not decided.  defect "wrong_sign": gains grow where update x g > 0."""
    f32 = np.float32
    exag, mom, lr = (float(f32(s)) for s in sched)
    Y32, u32, gn32 = (np.asarray(a, dtype=f32) for a in (Y, update, gains))
    part = np.asarray(part, dtype=f32).astype(np.float64)
    splits = part.shape[0]
    R, S_R = part[:, :, :2].sum(0), np.abs(part[:, :, :2]).sum(0)
    A, S_A, klt, p, deg = attraction(Y32, indptr, indices, data, exag, Z)
    g = 4.0 * (A - R / Z)
    chain = (9.0 + np.ceil(deg / 64.0) + 6.0)[:, None]
    b_g = 4.0 * (chain * V * S_A + splits * V * S_R / Z) + V * np.abs(g) + TINY32
    prod = u32.astype(np.float64) * g
    inc = prod > 0 if defect == "wrong_sign" else prod < 0
    gn = np.where(inc, gn32 + f32(0.2), gn32 * f32(0.8)).astype(f32)
    gn = np.maximum(gn, f32(0.01))
    free = (np.abs(g) <= b_g) & (u32 != 0)
    gnd = gn.astype(np.float64)
    upd = mom * u32.astype(np.float64) - lr * gnd * g
    b_u = lr * gnd * b_g + V * (2.0 * np.abs(mom * u32) + 3.0 * np.abs(lr * gnd * g)) + TINY32
    Yn = Y32.astype(np.float64) + upd
    b_y = b_u + V * np.abs(Yn) + TINY32
    gg, sgg = float((g * g).sum()), float((gnd * g * gnd * g).sum())
    n = g.size
    b_gg = float((2.0 * np.abs(g) * b_g + b_g * b_g).sum() + n * U * gg)
    b_sgg = float((gnd * gnd * (2.0 * np.abs(g) * b_g + b_g * b_g)).sum() + n * U * sgg + 2.0 * V * sgg)
    logt = np.where(p > 0, klt / np.where(p > 0, p, 1.0), 0.0)
    b_kl = float(V * (p * (7.0 + np.abs(logt))).sum() + len(p) * U * np.abs(klt).sum()) + TINY
    return {"g": g, "gains": gn, "update": upd, "Y": Yn, "gg": gg, "sgg": sgg, "kl": float(klt.sum()),
            "b_g": b_g, "b_u": b_u, "b_y": b_y, "b_gg": b_gg, "b_sgg": b_sgg, "b_kl": b_kl, "free": free}


def kl_of(Y, indptr, indices, data):
    """the sparse KL of a map under the joint P, in f64 (what TSNE.kl_divergence_ reports, exact Z)"""
    return gradient(Y, indptr, indices, data, 1.0)[1]


# ---- PCA ---------------------------------------------------------------------------------------------------------------

def moments(X, mean=None):
    """-> (mean, cov, bound_mean, bound_cov); with `mean` given (the device's), cov is centred on it"""
    X = np.asarray(X, dtype=np.float32).astype(np.float64)
    N = len(X)
    m = (X.astype(LD).sum(0) / N).astype(np.float64)
    b_m = (N + 1) * U * np.abs(X).sum(0) / N + TINY
    c = (X - (m if mean is None else np.asarray(mean))).astype(LD)
    cov = (c.T @ c / (N - 1)).astype(np.float64)
    S = (np.abs(c).T @ np.abs(c) / (N - 1)).astype(np.float64)
    return m, cov, b_m, (N + 2) * U * S + TINY


def pca(X, n_components=2):
    """exact PCA in f64 -> (embedding [N, nc], components [nc, L], explained variance [nc], mean [L])"""
    X = np.asarray(X).astype(np.float64)
    m, cov, _, _ = moments(X.astype(np.float32) if X.dtype == np.float32 else X)
    w, v = np.linalg.eigh(cov)
    order = np.argsort(w, kind="stable")[::-1][:n_components]
    comp = v[:, order].T.copy()
    for c in comp:
        if c[np.argmax(np.abs(c))] < 0:
            c *= -1.0
    return (X - m) @ comp.T, comp, w[order], m


def within(got, ref, bnd, what):
    """Assert |got - ref| <= bnd element-wise (NaN fails); returns the worst |err| / bound."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    bnd = np.broadcast_to(np.asarray(bnd, dtype=np.float64), ref.shape)
    err = np.abs(got - ref)
    ratio = np.where(np.isnan(err), np.inf, err / bnd)
    bad = ~(err <= bnd)
    if bad.any():
        i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements outside the bound; worst |err|/bound = "
                             f"{ratio[i]:.3g} at {i}: got {got[i]!r}, ref {ref[i]!r}, bound {bnd[i]:.3g}")
    return float(ratio.max()) if ratio.size else 0.0


def rejects(got, ref, bnd):
    """True when at least one element is outside the bound"""
    return bool(np.any(~(np.abs(np.asarray(got, dtype=np.float64) - ref) <= bnd)))


def hard_codes(N=160, L=12, distinct=9, seed=5):
    """hard 0/1 codes with many duplicates: integer distances, zero distances, exact ties"""
    r = np.random.RandomState(seed)
    return r.randint(0, 2, (distinct, L))[r.randint(0, distinct, N)].astype(np.float32)
