"""Reference and bounds for the spectral tests (csrc/spectral.hip, spectral.py).

An f64 numpy restatement of the kernels with their sum orders, of the Lanczos solver around them and of umap-learn's and
scikit-learn's conventions, written independently of the package.  Functions that take a `defect` name restate the
algorithm with one named mistake; tests/test_spectral_cpu.py shows that the gates the GPU tests use reject each.

Formulation.  W symmetric CSR with f32 weights, deg_i = sum_e w_e (e ascending, f64), isd_i = 1 / sqrt(deg_i) (0 at
deg_i = 0), S = D^-1/2 W D^-1/2, L = I - S.
  product      y_i = isd_i sum_e t_e, t_e = w_e (isd_j x_j); the row's edges in chunks of 64, a chunk added by the butterfly
               (the halving tree lane l += lane l + h, h = 32 .. 1), the chunks added in order from zero.
  dots         c_k = V_k . w: rows in blocks of 1024; thread t of 256 adds its rows t + 256 s, s = 0..3, from zero; the
               butterfly adds each wave of 64 threads; the four waves are added in order; the blocks in order from zero.
  update       w_i -= s_i, s_i = sum_k c_k V_k[i], k ascending from zero.
  step j       w = S v_j; twice: c = V_{0..q+j}^T w, w -= V^T c; alpha_j = c'_{q+j} + c''_{q+j}; beta_j = sqrt(w . w) by
               the dots' sum; v_{j+1} = w / beta_j; beta_j <= 2^-40: breakdown.
  solver       steps in blocks of 8; T = tridiag(alpha, beta); the k largest Ritz values theta of S (the lowest 1 - theta
               of L); stop when every |beta_{m-1} s_{m-1,i}| <= tol, on breakdown, or at max_steps.  Ritz vectors
               y_i = sum_j V[q+j] s_ji, j ascending; true residuals |S y - theta y|_2 by the product and the dots' sum.

Bounds.  u = 2^-53; every count is a worst-case first-order one, nothing was chosen by looking at device output.  Against
values computed in extended precision (numpy longdouble, any order):
  deg          d = the row's entries: at most d roundings, b = d u deg.  isd: half of that relatively, the square root and
               the division one rounding each: b = (d + 3) u isd.
  product      t_e rounds twice; 6 butterfly levels; ceil(d / 64) chunk additions; the product with isd_i:
               b_y = (9 + ceil(d / 64)) u isd_i sum_e |t_e| + tiny.
  dots         the product rounds once; 4 additions in a thread, 6 butterfly levels, 3 wave additions, B blocks:
               b_c = (14 + B) u sum_i |V_k[i] w_i| + tiny.
  update       each product rounds once, nv additions, the subtraction: b_w = (nv + 1) u sum_k |c_k V_k[i]| + u |w_i'| + tiny.
One step, device against this restatement (both run the same recurrence in f64; each deviates from the recurrence in exact
arithmetic by at most the following, so the two differ by at most twice it).  With V orthonormal the maps w -> V^T w and
(w, c) -> w - V c have norm 1, so in 2-norms, e_y = |b_y|, e_c = |b_c| (over k) and e_u = |b_w| of each pass:
  after the product d0 = e_y; after a pass d' = 2 d + e_c + e_u; so d2 = 4 e_y + 2 (e_c1 + e_u1) + e_c2 + e_u2 and
  D_w = 2 d2.   alpha: D_a = 2 (e_y + b_c1[q+j] + (2 e_y + e_c1 + e_u1) + b_c2[q+j] + u |alpha|).
  beta: D_b = D_w + (16 + B) u beta.   v_{j+1}: every element within D_v = (D_w + D_b) / beta + 2 u.
Whole solves.  For a symmetric matrix every Ritz pair has an eigenvalue within its residual, so eigenvalues are held to
tol + N 2^-52 against a dense eigh (its own rounding), and by Davis-Kahan an eigenvector, sign-fixed on both sides, to
sqrt(2) (res_i + N 2^-52) / gap_i in 2-norm, gap_i = the distance from lambda_i to the nearest other reference eigenvalue.
Returned vectors: Y = V s with V orthonormal to (q + m) u 4 after two Gram-Schmidt passes and s orthonormal to m u:
|Y^T Y - I|_max <= 8 (q + m + N) u, stated with N for the dots' own rounding.  A residual recomputed on the host in f64
differs from the device's by both sides' product rounding: <= 2 |b_y|_2 + (16 + B) u res.  residual_cap states how far
a true residual may exceed tol.
"""
import numpy as np

U = 2.0 ** -53
TINY = 1e-300
BLOCK = 1024
BREAKDOWN = 2.0 ** -40
ENQUEUE = 8
DEFECTS = ("no_reorth", "single_pass_gs", "unnormalised_laplacian", "divide_by_deg", "keeps_first", "sign_by_first_entry",
           "alpha_first_pass_only", "chunk_tail_dropped")


def tree64(a):
    """the butterfly's sum of the last axis (64 long) as lane 0 holds it"""
    for h in (32, 16, 8, 4, 2, 1):
        a = a[..., :h] + a[..., h:2 * h]
    return a[..., 0]


def rows_of(indptr):
    return np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))


def degree(indptr, indices, data):
    """-> deg, isd, b_deg, b_isd: the row's entries added in ascending order; columns outside [0, N) skipped"""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    N = len(indptr) - 1
    w = np.where((indices >= 0) & (indices < N), np.asarray(data, dtype=np.float32).astype(np.float64), 0.0)
    cnt = np.diff(indptr)
    deg = np.zeros(N)
    for t in range(int(cnt.max()) if N else 0):
        r = np.nonzero(cnt > t)[0]
        deg[r] = deg[r] + w[indptr[r] + t]
    with np.errstate(divide="ignore"):
        isd = np.where(deg == 0, 0.0, 1.0 / np.sqrt(np.where(deg == 0, 1.0, deg)))
    return deg, isd, cnt * U * deg, (cnt + 3) * U * isd


def matvec(indptr, indices, data, isd, x, defect=None, batch=1 << 15):
    """-> y, b_y (the bound against exact arithmetic on the same inputs)"""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    N = len(indptr) - 1
    ok = (indices >= 0) & (indices < N)
    j = np.where(ok, indices, 0)
    t = np.where(ok, np.asarray(data, dtype=np.float32).astype(np.float64) * (isd[j] * x[j]), 0.0)
    cnt = np.diff(indptr)
    rows = rows_of(indptr)
    off = np.arange(len(indices)) - indptr[rows]
    if defect == "chunk_tail_dropped":
        t = np.where(off < (cnt[rows] // 64) * 64, t, 0.0)
    acc, S = np.zeros(N), np.zeros(N)
    np.add.at(S, rows, np.abs(t))
    nch = -(-cnt // 64)
    for r0 in range(0, N, batch):
        r1 = min(N, r0 + batch)
        e0, e1 = indptr[r0], indptr[r1]
        width = int(nch[r0:r1].max()) if r1 > r0 else 0
        if width == 0:
            continue
        pad = np.zeros((r1 - r0, width * 64))
        pad[rows[e0:e1] - r0, off[e0:e1]] = t[e0:e1]
        sums = tree64(pad.reshape(r1 - r0, width, 64))
        a = np.zeros(r1 - r0)
        for c in range(width):
            a = a + sums[:, c]
        acc[r0:r1] = a
    y = isd * acc
    return y, (9 + nch) * U * isd * S + TINY


def matvec_exact(indptr, indices, data, isd, x):
    """the same product in extended precision, any order"""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    N = len(indptr) - 1
    ok = (indices >= 0) & (indices < N)
    j = np.where(ok, indices, 0)
    ld = np.longdouble
    t = np.where(ok, np.asarray(data, dtype=np.float32).astype(ld) * (isd[j].astype(ld) * x[j].astype(ld)), ld(0))
    acc = np.zeros(N, dtype=ld)
    np.add.at(acc, rows_of(indptr), t)
    return isd.astype(ld) * acc


def dots(V, w):
    """-> c [nv], b_c [nv]"""
    V = np.atleast_2d(V)
    nv, N = V.shape
    B = -(-N // BLOCK)
    P = np.zeros((nv, B * BLOCK))
    P[:, :N] = V * w
    P = P.reshape(nv, B, 4, 4, 64)                          # row = 1024 b + 256 s + 64 wave + lane
    t = ((P[:, :, 0] + P[:, :, 1]) + P[:, :, 2]) + P[:, :, 3]
    wv = tree64(t)
    part = ((wv[..., 0] + wv[..., 1]) + wv[..., 2]) + wv[..., 3]
    c = np.zeros(nv)
    for b in range(B):
        c = c + part[:, b]
    return c, (14 + B) * U * np.abs(V * w).sum(1) + TINY


def update(V, c, w):
    """-> w', b_w"""
    V = np.atleast_2d(V)
    T = np.asarray(c)[:len(V), None] * V
    s = np.cumsum(T, axis=0)[-1] if len(V) else np.zeros(V.shape[1])      # one addition after the other, k ascending
    S = np.abs(T).sum(0)
    out = w - s
    return out, (len(V) + 1) * U * S + U * np.abs(out) + TINY


def norm(w):
    return float(np.sqrt(dots(w[None], w)[0][0]))


def unit(w):
    return w / np.sqrt(dots(w[None], w)[0][0])


def step_fast(S, V, q, j):
    """the same step with BLAS sums (another order, no bounds): for the long closed-form runs of the CPU tests"""
    Vn = V[:q + j + 1]
    w = S @ V[q + j]
    alpha = 0.0
    for _ in range(2):
        c = Vn @ w
        w = w - c @ Vn
        alpha += float(c[-1])
    beta = float(np.sqrt(w @ w))
    with np.errstate(divide="ignore", invalid="ignore"):
        return {"w": w, "v": w / beta, "alpha": alpha, "beta": beta}


def step(csr, isd, V, q, j, defect=None):
    """Lanczos step j on V [>= q + j + 1][N] -> dict: w (before the scaling), v (after), alpha, beta and the bounds
    D_w, D_a, D_b, D_v of the docstring"""
    nv = q + j + 1
    Vn = V[:nv]
    w, b_y = matvec(*csr, isd, V[q + j], defect=defect)
    e_y = float(np.linalg.norm(b_y))
    alpha, d, D_a = 0.0, e_y, 0.0
    passes = 1 if defect == "single_pass_gs" else 2
    for p in range(passes):
        if defect == "no_reorth":                           # the three-term recurrence alone
            Vp = V[max(q + j - 1, 0):nv] if p == 0 else V[:0]
            if p == 1:
                break
        else:
            Vp = Vn
        c, b_c = dots(Vp, w)
        w, b_w = update(Vp, c, w)
        if p == 0 or defect != "alpha_first_pass_only":
            alpha += float(c[-1])
        e_c, e_u = float(np.linalg.norm(b_c)), float(np.linalg.norm(b_w))
        D_a += d + float(b_c[-1])
        d = 2 * d + e_c + e_u
    B = -(-len(w) // BLOCK)
    beta = norm(w)
    D_w = 2 * d
    D_a = 2 * (D_a + U * abs(alpha))
    D_b = D_w + (16 + B) * U * beta
    with np.errstate(divide="ignore", invalid="ignore"):
        v = w / beta
    return {"w": w, "v": v, "alpha": alpha, "beta": beta, "D_w": D_w, "D_a": D_a, "D_b": D_b,
            "D_v": (D_w + D_b) / max(beta, TINY) + 2 * U}


def sign_fix(Y, defect=None):
    """_deterministic_vector_sign_flip on the rows of Y [k, N]"""
    Y = np.atleast_2d(Y)
    big = np.zeros(len(Y), dtype=np.int64) if defect == "sign_by_first_entry" else np.argmax(np.abs(Y), axis=1)
    sg = np.sign(Y[np.arange(len(Y)), big])
    sg[sg == 0] = 1.0
    return Y * sg[:, None]


def tridiag_eigh(a, b, k):
    """the k largest eigenpairs of tridiag(a, b), ascending"""
    from scipy.linalg import eigh_tridiagonal
    m = len(a)
    if m == 1:
        return np.array(a, dtype=np.float64), np.ones((1, 1))
    return eigh_tridiagonal(a, b, select="i", select_range=(max(m - k, 0), m - 1))


def lanczos(indptr, indices, data, k, tol=1e-10, max_steps=None, v0=None, seed=0, locked=None, defect=None,
            keep_basis=False, fast=False):
    """spectral.lanczos_eigsh restated -> dict: eigenvalues [k'] ascending (of L), vectors [N, k'], residuals, steps,
    converged, why, est (the stopping estimates), and with keep_basis V, alpha, beta, q"""
    csr = (indptr, indices, data)
    N = len(indptr) - 1
    _, isd, _, _ = degree(*csr)
    lock = np.zeros((0, N)) if locked is None else np.asarray(locked, dtype=np.float64).reshape(-1, N)
    q = len(lock)
    m_max = min(N - q, 1024) if max_steps is None else int(max_steps)
    V = np.zeros((q + m_max + 1, N))
    V[:q] = lock
    w = np.random.RandomState(seed).uniform(-1, 1, N) if v0 is None else np.asarray(v0, dtype=np.float64).copy()
    for _ in range(2 if q else 0):
        w = update(V[:q], dots(V[:q], w)[0], w)[0]
    V[q] = unit(w)
    alpha, beta = np.zeros(m_max), np.zeros(m_max)
    m, broken = 0, False
    if fast:
        from scipy.sparse import csr_matrix
        Sm = csr_matrix((np.asarray(data, dtype=np.float64), indices, indptr), shape=(N, N))
        Sm = csr_matrix(Sm.multiply(isd[:, None]).multiply(isd[None, :]))
    while True:
        for _ in range(min(ENQUEUE, m_max - m)):
            if broken:
                break
            r = step_fast(Sm, V, q, m) if fast else step(csr, isd, V, q, m, defect=defect)
            alpha[m], beta[m] = r["alpha"], r["beta"]
            broken = not r["beta"] > BREAKDOWN
            V[q + m + 1] = r["w"] if broken else r["v"]
            m += 1
        theta, s = tridiag_eigh(alpha[:m], beta[:m - 1], k)
        kk = min(k, m)
        pick = np.argsort(-theta, kind="stable")[:kk]
        est = np.abs(beta[m - 1] * s[m - 1, pick])
        if broken:
            why, converged = "invariant", kk == k
            break
        if kk == k and np.all(est <= tol):
            why, converged = "tol", True
            break
        if m >= m_max:
            why, converged = "max_steps", False
            break
    Y = np.zeros((kk, N))
    for jj in range(m):
        Y = Y + V[q + jj][None, :] * s[jj, pick][:, None]
    res = np.array([norm(matvec(*csr, isd, y)[0] - t * y) for y, t in zip(Y, theta[pick])])
    out = {"eigenvalues": 1.0 - theta[pick], "vectors": sign_fix(Y, defect).T.copy(), "residuals": res, "steps": m,
           "converged": bool(converged), "why": why, "est": est, "isd": isd}
    if keep_basis:
        out.update(V=V, alpha=alpha, beta=beta, q=q)
    return out


def trivial_vector(indptr, indices, data):
    return unit(np.sqrt(degree(indptr, indices, data)[0]))


def spectral_layout(indptr, indices, data, dim=2, defect=None, **kw):
    """umap-learn's spectral_layout of a connected graph -> (vectors [N, dim], the solver's dict)"""
    if defect == "unnormalised_laplacian":                  # D - W: its eigenvectors are D^-1/2-free
        Lm = -dense_S(indptr, indices, data, normalise=False)
        np.fill_diagonal(Lm, degree(indptr, indices, data)[0])
        lam, vec = np.linalg.eigh(Lm)
        return sign_fix(vec[:, 1:dim + 1].T).T, {"eigenvalues": lam[1:dim + 1]}
    if defect == "keeps_first":
        r = lanczos(indptr, indices, data, dim, defect=defect, **kw)
        return r["vectors"], r
    r = lanczos(indptr, indices, data, dim, locked=trivial_vector(indptr, indices, data), defect=defect, **kw)
    return r["vectors"], r


def spectral_embedding(indptr, indices, data, n_components=8, drop_first=True, defect=None, **kw):
    """sklearn.manifold.spectral_embedding(W, n_components, norm_laplacian=True, drop_first=drop_first)"""
    deg, isd, _, _ = degree(indptr, indices, data)
    q0 = trivial_vector(indptr, indices, data)
    want = n_components if drop_first else n_components - 1
    rows = [] if drop_first else [q0[None]]
    r = None
    if want:
        r = lanczos(indptr, indices, data, want, locked=q0, defect=defect, **kw)
        rows.append(r["vectors"].T)
    scale = isd * isd if defect == "divide_by_deg" else isd
    return sign_fix(np.concatenate(rows, 0) * scale[None], defect).T.copy(), r


def dense_S(indptr, indices, data, normalise=True):
    N = len(indptr) - 1
    W = np.zeros((N, N))
    W[rows_of(indptr), indices] = np.asarray(data, dtype=np.float64)
    if not normalise:
        return W
    isd = degree(indptr, indices, data)[1]
    return isd[:, None] * W * isd[None, :]


def dense_eigh(indptr, indices, data, k):
    """the k lowest eigenpairs of L = I - S by numpy.linalg.eigh -> (lambda [k'], vectors [N, k'] sign-fixed, all lambda)"""
    lam, vec = np.linalg.eigh(np.eye(len(indptr) - 1) - dense_S(indptr, indices, data))
    return lam[:k], sign_fix(vec[:, :k].T).T.copy(), lam


def gaps(lam_all, idx):
    """the distance from lambda_i to the nearest other eigenvalue"""
    lam_all = np.asarray(lam_all)
    return np.array([np.min(np.abs(np.delete(lam_all, i) - lam_all[i])) for i in idx])


def davis_kahan(res, gap, N):
    return np.sqrt(2.0) * (np.asarray(res) + N * 2.0 ** -52) / gap


def orth_bound(q, m, N):
    return 8.0 * (q + m + N) * U


def residual_cap(tol, q, m, N, max_deg):
    """what a true residual may reach when the stopping estimate is at tol: the Lanczos relation S V = V T + beta v e^T
    holds to the basis' orthonormality (|S| <= 1), and the product that recomputes the residual rounds (twice |b_y|_2 <=
    (9 + chunks) u sqrt(N) for a unit vector: once in the solver's estimate, once in the recomputation)"""
    return tol + orth_bound(q, m, N) + 2.0 * (9 + -(-max_deg // 64)) * U * np.sqrt(N)


# ---- graphs --------------------------------------------------------------------------------------------------------------

def to_csr(W):
    W = np.asarray(W, dtype=np.float64)
    N = len(W)
    r, c = np.nonzero(W)
    indptr = np.zeros(N + 1, dtype=np.int64)
    np.add.at(indptr, r + 1, 1)
    return np.cumsum(indptr).astype(np.int32), c.astype(np.int32), W[r, c].astype(np.float32)


def path_graph(n):
    """P_n with unit weights as CSR without a dense matrix; eigenvalues of L: 1 - cos(pi k / (n - 1)), all simple"""
    cnt = np.full(n, 2, dtype=np.int64)
    cnt[0] = cnt[-1] = 1
    indptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    i = np.arange(n)
    keep = np.stack([i - 1 >= 0, i + 1 < n], axis=1).reshape(-1)
    cols = np.stack([i - 1, i + 1], axis=1).reshape(-1)[keep]
    return indptr, cols.astype(np.int32), np.ones(len(cols), dtype=np.float32)


def path_eigenvalues(n, k):
    return 1.0 - np.cos(np.pi * np.arange(k) / (n - 1))


def complete_graph(n):
    return to_csr(np.ones((n, n)) - np.eye(n))


def cycle_graph(n):
    W = np.zeros((n, n))
    i = np.arange(n)
    W[i, (i + 1) % n] = W[(i + 1) % n, i] = 1.0
    return to_csr(W)


def two_cliques(n):
    """two disjoint K_n"""
    W = np.zeros((2 * n, 2 * n))
    W[:n, :n] = W[n:, n:] = 1.0
    np.fill_diagonal(W, 0.0)
    return to_csr(W)


def fuzzy_fixture(X, n_neighbors):
    """the fuzzy graph of X as tests/_umap_ref.py builds it"""
    import _projection_ref as P
    import _umap_ref as R
    idx, d2, _ = P.knn(X, n_neighbors - 1)
    return R.fuzzy_csr(idx, R.smooth_knn(d2)["w"].astype(np.float32))


# ---- gates (shared by the CPU and the GPU tests): the worst |error| / bound, to be held at or below 1 ---------------------

def eigenvalue_gate(lam, ref, tol, N):
    lam, ref = np.asarray(lam), np.asarray(ref)
    if lam.shape != ref.shape:
        return np.inf
    return float(np.max(np.abs(lam - ref) / (tol + N * 2.0 ** -52)))


def vector_gate(vec, res, ref_vec, ref_lam, idx, N, extra=0.0, scale=1.0):
    """columns of vec [N, k] against ref_vec[:, idx], both sign-fixed; gaps from the reference eigenvalues ref_lam"""
    vec, ref = np.asarray(vec), np.asarray(ref_vec)[:, list(idx)]
    if vec.shape != ref.shape:
        return np.inf
    bound = scale * davis_kahan(np.asarray(res) + extra, gaps(ref_lam, idx), N)
    return float(np.max(np.linalg.norm(vec - ref, axis=0) / bound))


def orth_gate(Y, q, m):
    Y = np.asarray(Y)
    return float(np.abs(Y.T @ Y - np.eye(Y.shape[1])).max() / orth_bound(q, m, len(Y)))
