"""Reference and bounds for the hidden-Markov-model tests (csrc/hmm.hip, hmm.py).

An f64 numpy restatement of the emissions, the scaled forward and backward recursions (sequentially, and blocked in the
three launches' order), the posterior, the transition update, Viterbi and the whole fit in the orders include/rbvae_hip.h
states, written independently of the package; every function also runs in long double (dtype=LD), and brute() enumerates
all K^N paths of a tiny case.  Functions take a `defect` name: the restatement with one named mistake, which
tests/test_hmm_cpu.py uses to show that the check meant to catch that mistake does.

Bounds.  u = 2^-53; every count is first order; exp and log are taken as accurate to 2 ulp = 4 u relative, as in _gmm_ref.
Given e, every alpha, beta, gamma and Xi is a sum of products of non-negative numbers, so a relative error of its inputs
and the roundings on its longest path add up and never amplify.  References are long double rounded to f64 (ROUND).
  alpha    The scale of a row is common to its K values and cancels in the next normalisation, so alpha_t is the normalised
           unscaled product of t + 1 rows; a path through one row takes the product with A (1), K additions, the product
           with e (1) and the division (1): P = K + 4 with one to spare.  After n rows the unscaled value is off by n P u;
           the last normalisation divides by a sum that is off by as much and by the butterfly's 6 additions:
           rho(n) = 2 n P u + 8 u, relative.  Forward n = t + 1, backward n = N - 1 - t (beta_(N-1) = 1 / K: one division).
  blocked  a path still passes every row once, in launch (i) or (iii).  A block it passes in launch (ii) adds the error of
           the weight w_i = v_i exp(s_i - max s): every log z of the block's R rows is off by 4 u |log z| and every partial
           sum by u |s|, the difference by u |s_i - max s|, exp by 4 u, the product by u; then K additions, the product with
           u_ij and the normalisation (8): E_b = u ((5 R + 1) Lmax_b + K + 14), Lmax_b the largest |log z|, |partial s| or
           |s_i - max s| of the block's live start vectors (block_scales).  rho_blocked = rho(n) + 2 sum of E_b over the
           blocks passed.
  ll       c_t sums y_t, computed from alpha_(t-1): rho(t) + (K + 8) u relative, so log c_t is off by that plus 4 u |log c_t|,
           and the sum with m_t rounds: b_ll = rho(t) + (K + 8) u + 4 u |log c_t| + u |ll_t|.
  gamma    a term alpha beta: rho_a + rho_b + u; g adds K of them; the division: gamma (2 (rho_a + rho_b) + (K + 3) u).
  Xi       a term is off by rho_a(t) + rho_b(t + 1) + 3 u, Z_t by that and its K^2 additions, the quotient rounds, N - 1 terms
           are added: Xi (2 max_t (rho_a(t) + rho_b(t + 1)) + (K^2 + N + 7) u).  A_new = (Xi + eps / K) / (sum_j Xi + eps):
           twice that and (K + 3) u.
  sums     sum_k gamma_kt = 1 within 2 K u (K quotients of one g, added in long double); sum_ij Xi_ij = N - 1 within
           (N - 1) (K^2 + N + 3) u: a row's K^2 quotients add to 1 within (K^2 + 2) u and N - 1 rows are added.
  lb       the mixture's bound for q: (L + 5) u q / 2; c_k = sum_l log s_kl - L / 2 log 2 pi: 4 u |log s| each, L + 2
           roundings on values below sum |log s| + c; the difference rounds: b_lb = (L + 5) u q / 2 + u ((L + 6) sum_l
           |log s_kl| + 3 c) + u |lb|.  e = exp(lb - m): the argument is off by b_lb of both and rounds, exp 4 u:
           e (b_lb_k + b_lb_max + u |lb - m| + 4 u), with an absolute 1e-300 where e passes through the subnormal range.
Values below 1e-290 take an absolute term of 1e-300 throughout (TINY through ROUND, SUBNORMAL where a product may underflow).
"""
import functools
import itertools

import numpy as np

import _gmm_ref as G
import _kmeans_ref as Km
from _projection_ref import TINY, U, rejects, within  # noqa: F401

LD = np.longdouble
EPS = 10.0 * np.finfo(np.float64).eps
LOG_2PI = G.LOG_2PI
BLOCK_ROWS = 64
NO_ROW = 2 ** 31 - 1
SUBNORMAL = 1e-300
DEFECTS = ("block_boundary_reset", "transfer_scale_dropped", "beta_uses_e_t", "xi_without_emission", "A_column_normalised",
           "pi_not_updated", "loglik_without_rowmax", "viterbi_sum_for_max", "viterbi_tie_high", "bic_param_count_gmm")
ROUND = G.ROUND


def ws_bytes(N, K, R):
    blocks = -(-N // R)
    return 8 * max(blocks * (K * K + 2 * K), N + G.blocks_rows(N)[0] * K * K)


def ok(N, L, K):
    return 1 <= L <= 128 and 1 <= K <= 64 and max(K, 2) <= N <= 1 << 20 and N * K <= 1 << 26


# ---- emissions ---------------------------------------------------------------------------------------------------------------

def emit(X, means, prec, dtype=np.float64):
    """-> (lb [N, K], m [N], e [N, K]): lb = c - q / 2, c_k = sum_l log s_kl - L / 2 log 2 pi (l ascending), e = exp(lb - m)"""
    q = G.quad(X, means, prec, dtype)
    Ld = np.asarray(X).shape[1]
    logs = np.log(np.asarray(prec).astype(dtype))
    t = np.zeros(len(logs), dtype=dtype)
    for l in range(Ld):
        t = t + logs[:, l]
    c = t - dtype(0.5) * Ld * dtype(LOG_2PI)
    lb = c[None, :] - dtype(0.5) * q
    m = lb.max(axis=1)
    with np.errstate(under="ignore"):
        e = np.exp(lb - m[:, None])
    return lb, m, e


def emit_bounds(X, means, prec):
    Ld = np.asarray(X).shape[1]
    q = G.quad(X, means, prec, LD)
    lb, m, e = emit(X, means, prec, LD)
    sal = np.abs(np.log(np.asarray(prec).astype(LD))).sum(axis=1)
    c = 0.5 * Ld * LOG_2PI
    b_lb = ((Ld + 5) * U * 0.5 * q + U * ((Ld + 6) * sal[None, :] + 3 * c) + U * np.abs(lb)).astype(np.float64)
    f = lambda v: v.astype(np.float64)  # noqa: E731
    b_e = f(e) * (b_lb + b_lb.max(axis=1)[:, None] + U * f(np.abs(lb - m[:, None])) + 4 * U) + SUBNORMAL
    return {"lb": f(lb), "m": f(m), "e": f(e), "b_lb": b_lb + ROUND(f(lb)), "b_m": b_lb.max(axis=1) + ROUND(f(m)),
            "b_e": b_e + ROUND(f(e))}


# ---- the recurrence ----------------------------------------------------------------------------------------------------------

def wsum(y):
    """SUM over the last axis: the butterfly over 64 lanes, the lanes from K on zero"""
    K = y.shape[-1]
    p = np.zeros(y.shape[:-1] + (64,), dtype=y.dtype)
    p[..., :K] = y
    for o in (32, 16, 8, 4, 2, 1):
        p = p[..., :o] + p[..., o:2 * o]
    return p[..., 0]


def dot(x, M):
    """sum_i x_i M[i, :] over the last axis of x, i ascending from zero, every product rounded before it is added (long
    double: a reference, whose order does not matter)"""
    if M.dtype == LD:
        return x @ M
    s = np.zeros(x.shape[:-1] + (M.shape[1],), dtype=M.dtype)
    for i in range(M.shape[0]):
        s = s + x[..., i, None] * M[i]
    return s


def _step(v, ev, A, fwd):
    return dot(v, A) * ev if fwd else dot(ev * v, A.T)


def _status(bad_rows):
    bad_rows = sorted(bad_rows)
    return [len(bad_rows), bad_rows[0] if bad_rows else NO_ROW]


def _bad(z):
    return not (z > 0) or np.isinf(z)


def forward(e, m, pi, A, defect=None, dtype=np.float64, R=None):
    """-> (alpha [N, K], ll [N], status).  R: blocked in the three launches' order (None: the plain recursion).
    defects: "loglik_without_rowmax", "block_boundary_reset", "transfer_scale_dropped" """
    return _recurrence(e, m, pi, A, True, defect, dtype, R)


def backward(e, A, defect=None, dtype=np.float64, R=None):
    """-> (beta [N, K], status).  defects: "beta_uses_e_t", "block_boundary_reset", "transfer_scale_dropped" """
    out, _, st = _recurrence(e, None, None, A, False, defect, dtype, R)
    return out, st


def _rows(N, fwd, lo, hi):
    """the rows a block [lo, hi) writes after a given vector, in the order they are taken, with the row whose e they read"""
    if fwd:
        return [(t, t) for t in range(lo, hi)]
    return [(t, t + 1) for t in range(hi - 1, lo - 1, -1)]


def _recurrence(e, m, pi, A, fwd, defect, dtype, R):
    e, A = np.asarray(e).astype(dtype), np.asarray(A).astype(dtype)
    N, K = e.shape
    out, ll, bad = np.zeros((N, K), dtype=dtype), np.zeros(N, dtype=dtype), []
    esrc = (lambda t, r: e[t]) if (not fwd and defect == "beta_uses_e_t") else (lambda t, r: e[r])
    if fwd:
        pi = np.asarray(pi).astype(dtype)
        m = np.asarray(m).astype(dtype)

    def first_row():
        """the recursion's own first row -> the vector after it"""
        if fwd:
            y = pi * e[0]
            z = wsum(y)
            return y, z, 0
        return np.full(K, 1 / dtype(K), dtype=dtype), None, N - 1

    def plain(v, rows):
        for t, r in rows:
            y = _step(v, esrc(t, r), A, fwd)
            z = wsum(y)
            with np.errstate(all="ignore"):
                v = y / z
                out[t] = v
                if fwd:
                    ll[t] = np.log(z) + (0 if defect == "loglik_without_rowmax" else m[t])
            if _bad(z):
                bad.append(t)
        return v

    def begin():
        y, z, t0 = first_row()
        if fwd:
            with np.errstate(all="ignore"):
                v = y / z
                ll[0] = np.log(z) + (0 if defect == "loglik_without_rowmax" else m[0])
            if _bad(z):
                bad.append(0)
        else:
            v = y
        out[t0] = v
        return v

    if R is None or R >= N:
        v = begin()
        plain(v, _rows(N, fwd, 1, N) if fwd else _rows(N, fwd, 0, N - 1))
        return out, ll, _status(bad)
    blocks = -(-N // R)
    span = [(b * R, min(N, (b + 1) * R)) for b in range(blocks)]
    own = 0 if fwd else blocks - 1
    order = list(range(blocks)) if fwd else list(range(blocks - 1, -1, -1))

    def block_rows(b):
        lo, hi = span[b]
        if b == own:
            return _rows(N, fwd, 1, hi) if fwd else _rows(N, fwd, lo, N - 1)
        return _rows(N, fwd, lo, hi)

    # launch (i): the carried unit vectors and their log scales
    Us, Ss = {}, {}
    for b in order[:-1]:
        if b == own:
            y, z, _ = first_row()
            with np.errstate(all="ignore"):
                V = (y / z if z > 0 else np.zeros(K, dtype=dtype)) if fwd else y
            V, s = V[None, :], np.zeros(1, dtype=dtype)
        else:
            V, s = np.eye(K, dtype=dtype), np.zeros(K, dtype=dtype)
        for t, r in block_rows(b):
            Y = _step(V, esrc(t, r), A, fwd)
            z = wsum(Y)
            with np.errstate(all="ignore"):
                V = np.where(z[:, None] > 0, Y / z[:, None], 0)
                s = s + np.log(z)
        Us[b], Ss[b] = V, s
    # launch (ii): the vector that enters every block
    vin = {}
    v = Us[own][0]
    vin[order[1]] = v
    for n in range(1, blocks - 1):
        b = order[n]
        s = Ss[b]
        with np.errstate(all="ignore"):
            w = v if defect == "transfer_scale_dropped" else np.where(np.isneginf(s), 0, v * np.exp(s - s.max()))
            y = dot(w, Us[b])
            z = wsum(y)
            v = y / z if z > 0 else np.zeros(K, dtype=dtype)
        vin[order[n + 1]] = v
    if defect == "block_boundary_reset":
        for b in vin:
            vin[b] = pi if fwd else np.full(K, 1 / dtype(K), dtype=dtype)
    # launch (iii)
    for b in order:
        plain(begin() if b == own else vin[b], block_rows(b))
    return out, ll, _status(bad)


def block_scales(e, A, R, fwd):
    """Lmax_b of every block of the blocked recurrence (0 for a block no transfer is taken of): the largest |log z|,
    |partial s| and |s_i - max s| over its live start vectors.  Products by matmul: the order does not matter here."""
    e, A = np.asarray(e, dtype=np.float64), np.asarray(A, dtype=np.float64)
    N, K = e.shape
    blocks = -(-N // R)
    lmax = np.zeros(blocks)
    for b in (range(1, blocks - 1)):
        lo, hi = b * R, min(N, (b + 1) * R)
        V, s, big = np.eye(K), np.zeros(K), 0.0
        for t, r in _rows(N, fwd, lo, hi):
            Y = (V @ A) * e[r] if fwd else (V * e[r]) @ A.T
            z = Y.sum(axis=1)
            with np.errstate(all="ignore"):
                V = np.where(z[:, None] > 0, Y / z[:, None], 0)
                lz = np.log(z)
                s = s + lz
            live = np.isfinite(s)
            if live.any():
                big = max(big, float(np.abs(lz[live]).max()), float(np.abs(s[live]).max()))
        live = np.isfinite(s)
        if live.any():
            big = max(big, float((s[live].max() - s[live]).max()))
        lmax[b] = big
    return lmax


def rho(N, K, fwd, R=None, lmax=None):
    """[N]: the relative bound of alpha_t (fwd) or beta_t; R and lmax (block_scales): of the blocked form"""
    t = np.arange(N)
    n = (t + 1) if fwd else (N - 1 - t)
    r = 2 * n * (K + 4) * U + 8 * U
    if R is not None and R < N:
        blocks = -(-N // R)
        E = U * ((5 * R + 1) * np.asarray(lmax) + K + 14)
        E[0] = E[-1] = U * (K + 14)
        passed = np.cumsum(E) - E if fwd else (np.cumsum(E[::-1]) - E[::-1])[::-1]
        r = r + 2 * passed[np.minimum(t // R, blocks - 1)]
    return r


def ld_passes(e, m, pi, A):
    """the long double recursions, to be shared by several calls of recurrence_bounds"""
    with np.errstate(all="ignore"):
        return forward(e, m, pi, A, dtype=LD) + backward(e, A, dtype=LD)


def recurrence_bounds(e, m, pi, A, R=None, ld=None):
    """long double references of the recursions given e and the bounds of the docstring -> dict(alpha, beta, ll, b_alpha,
    b_beta, b_ll, rho_a, rho_b, status_a, status_b)"""
    N, K = np.asarray(e).shape
    al, ll, sa, be, sb = ld_passes(e, m, pi, A) if ld is None else ld
    blocked = R is not None and R < N
    ra = rho(N, K, True, R, block_scales(e, A, R, True) if blocked else None)
    rb = rho(N, K, False, R, block_scales(e, A, R, False) if blocked else None)
    f = lambda v: np.asarray(v).astype(np.float64)  # noqa: E731
    c = np.exp(f(ll - np.asarray(m).astype(LD)))
    prev = np.concatenate([[0.0], ra[:-1]])
    with np.errstate(all="ignore"):
        b_ll = prev + (K + 8) * U + 4 * U * np.abs(np.log(c)) + U * np.abs(f(ll))
    return {"alpha": f(al), "beta": f(be), "ll": f(ll), "b_alpha": f(al) * ra[:, None] + ROUND(f(al)) + SUBNORMAL,
            "b_beta": f(be) * rb[:, None] + ROUND(f(be)) + SUBNORMAL, "b_ll": b_ll + ROUND(f(ll)), "rho_a": ra, "rho_b": rb,
            "status_a": sa, "status_b": sb}


# ---- the posterior -----------------------------------------------------------------------------------------------------------

def posterior(alpha, beta, e, A, defect=None, dtype=np.float64):
    """-> (gamma [N, K], Xi [K, K], A_new [K, K], pi_new [K], status).  defects: "xi_without_emission", "A_column_normalised" """
    alpha, beta, e, A = (np.asarray(a).astype(dtype) for a in (alpha, beta, e, A))
    N, K = alpha.shape
    bad = []
    with np.errstate(all="ignore"):
        g = np.zeros(N, dtype=dtype)
        for k in range(K):
            g = g + alpha[:, k] * beta[:, k]
        gamma = (alpha * beta) / g[:, None]
        w = beta[1:] if defect == "xi_without_emission" else e[1:] * beta[1:]
        Z = np.zeros(N - 1, dtype=dtype)
        for i in range(K):
            for j in range(K):
                Z = Z + (alpha[:-1, i] * A[i, j]) * w[:, j]
        blocks, rows = G.blocks_rows(N)
        Xi = np.zeros((K, K), dtype=dtype)
        for b in range(blocks):
            lo, hi = b * rows, min(N - 1, (b + 1) * rows)
            part = np.zeros((K, K), dtype=dtype)
            if hi > lo:
                terms = ((alpha[lo:hi, :, None] * A[None]) * w[lo:hi, None, :]) / Z[lo:hi, None, None]
                for r in range(hi - lo):
                    part = part + terms[r]
            Xi = Xi + part
        if defect == "A_column_normalised":
            rs = np.zeros(K, dtype=dtype)
            for i in range(K):
                rs = rs + Xi[i, :]
            A_new = (Xi + dtype(EPS) / K) / (rs[None, :] + dtype(EPS))
        else:
            rs = np.zeros(K, dtype=dtype)
            for j in range(K):
                rs = rs + Xi[:, j]
            A_new = (Xi + dtype(EPS) / K) / (rs[:, None] + dtype(EPS))
    bad = [t for t in range(N) if _bad(g[t])] + [t for t in range(N - 1) if _bad(Z[t])]
    return gamma, Xi, A_new, gamma[0].copy(), [len(bad), min(bad) if bad else NO_ROW]


def posterior_bounds(alpha, beta, e, A, rho_a, rho_b):
    """long double references of the posterior from the long double alpha and beta (recurrence_bounds'), and the bounds of the
    docstring with their rho"""
    N, K = np.asarray(alpha).shape
    with np.errstate(all="ignore"):
        gamma, Xi, A_new, pi_new, _ = posterior(alpha, beta, e, A, dtype=LD)
    f = lambda v: np.asarray(v).astype(np.float64)  # noqa: E731
    rg = 2 * (rho_a + rho_b) + (K + 3) * U
    rx = 2 * float((rho_a[:-1] + rho_b[1:]).max()) + (K * K + N + 7) * U
    return {"gamma": f(gamma), "xi": f(Xi), "A_new": f(A_new), "pi_new": f(pi_new),
            "b_gamma": f(gamma) * rg[:, None] + ROUND(f(gamma)) + SUBNORMAL, "b_xi": f(Xi) * rx + ROUND(f(Xi)) + SUBNORMAL,
            "b_A_new": f(A_new) * (2 * rx + (K + 3) * U) + ROUND(f(A_new)) + SUBNORMAL,
            "b_pi_new": f(gamma[0]) * rg[0] + ROUND(f(gamma[0])) + SUBNORMAL,
            "b_gamma_sum": 2 * K * U, "b_xi_sum": (N - 1) * (K * K + N + 3) * U}


# ---- Viterbi -----------------------------------------------------------------------------------------------------------------

def viterbi(logb, lpi, lA, defect=None):
    """logb [N, K], log pi [K], log A [K, K] -> (path [N] int32, score, back [N, K] uint8).  defects: "viterbi_sum_for_max",
    "viterbi_tie_high" """
    logb, lpi, lA = (np.asarray(a, dtype=np.float64) for a in (logb, lpi, lA))
    N, K = logb.shape
    back = np.zeros((N, K), dtype=np.uint8)
    cols = np.arange(K)
    with np.errstate(all="ignore"):
        d = lpi + logb[0]
        for t in range(1, N):
            cand = d[:, None] + lA
            arg = (K - 1 - np.argmax(cand[::-1], axis=0)) if defect == "viterbi_tie_high" else np.argmax(cand, axis=0)
            best = cand[arg, cols]
            if defect == "viterbi_sum_for_max":
                mx = np.where(np.isfinite(best), best, 0.0)
                best = mx + np.log(np.exp(cand - mx[None, :]).sum(axis=0))
            d = best + logb[t]
            back[t] = arg
    s = int(K - 1 - np.argmax(d[::-1])) if defect == "viterbi_tie_high" else int(np.argmax(d))
    score = float(d[s])
    path = np.zeros(N, dtype=np.int32)
    for t in range(N - 1, -1, -1):
        path[t] = s
        s = int(back[t, s])
    return path, score, back


def log0(a):
    with np.errstate(divide="ignore"):
        return np.log(np.asarray(a, dtype=np.float64))


# ---- all paths ---------------------------------------------------------------------------------------------------------------

def brute(logb, pi, A):
    """every one of the K^N paths in long double (K <= 3, N <= 8) -> (log-likelihood, gamma [N, K], Xi [K, K], the best path,
    the margin of its log-probability over the runner-up's)"""
    b, pi, A = np.exp(np.asarray(logb).astype(LD)), np.asarray(pi).astype(LD), np.asarray(A).astype(LD)
    N, K = b.shape
    assert K <= 3 and N <= 8
    total, gamma, Xi, probs = LD(0), np.zeros((N, K), dtype=LD), np.zeros((K, K), dtype=LD), []
    for path in itertools.product(range(K), repeat=N):
        p = pi[path[0]] * b[0, path[0]]
        for t in range(1, N):
            p = p * A[path[t - 1], path[t]] * b[t, path[t]]
        total += p
        for t in range(N):
            gamma[t, path[t]] += p
        for t in range(1, N):
            Xi[path[t - 1], path[t]] += p
        probs.append((p, path))
    probs.sort(key=lambda x: -x[0])
    margin = float(np.log(probs[0][0]) - np.log(probs[1][0])) if len(probs) > 1 and probs[1][0] > 0 else np.inf
    return float(np.log(total)), (gamma / total).astype(np.float64), (Xi / total).astype(np.float64), np.array(probs[0][1]), margin


# ---- the fit -----------------------------------------------------------------------------------------------------------------

def n_parameters(K, L, defect=None):
    """(K - 1) + K (K - 1) + 2 K L; defect "bic_param_count_gmm": the mixture's 2 K L + K - 1"""
    return 2 * K * L + K - 1 if defect == "bic_param_count_gmm" else (K - 1) + K * (K - 1) + 2 * K * L


def criteria(score, N, K, L, defect=None):
    p = n_parameters(K, L, defect)
    return -2.0 * score * N + p * np.log(N), -2.0 * score * N + 2.0 * p


def initial_transitions(labels, K):
    n = np.zeros((K, K))
    np.add.at(n, (labels[:-1], labels[1:]), 1)
    return (n + 1) / (n.sum(axis=1, keepdims=True) + K)


def _mstep(X, gamma, reg_covar, dtype):
    """means, variances and precision roots from gamma [N, K]: _gmm_ref's ordered M-step in f64, plain sums in long double"""
    if dtype == np.float64:
        _, mu, var, s, _, _ = G.mstep(X, gamma, reg_covar)
        return mu, var, s
    Xl = np.asarray(X).astype(LD)
    nk = gamma.sum(axis=0) + LD(EPS)
    mu = (gamma.T @ Xl) / nk[:, None]
    d = Xl[:, None, :] - mu[None, :, :]
    var = np.einsum("ik,ikl->kl", gamma, d * d) / nk[:, None] + LD(reg_covar)
    return mu, var, 1 / np.sqrt(var)


def _mean(ll, dtype):
    return G.lower_bound(ll) if dtype == np.float64 else float(ll.sum() / len(ll))


def estep(X, pi, A, mu, s, defect=None, dtype=np.float64, R=None):
    lb, m, e = emit(X, mu, s, dtype)
    alpha, ll, sa = forward(e, m, pi, A, defect, dtype, R)
    beta, sb = backward(e, A, defect, dtype, R)
    gamma, Xi, A_new, pi_new, sp = posterior(alpha, beta, e, A, defect, dtype)
    return {"lb": lb, "m": m, "e": e, "alpha": alpha, "beta": beta, "ll": ll, "gamma": gamma, "xi": Xi, "A_new": A_new,
            "pi_new": pi_new, "bad": sa[0] + sb[0] + sp[0]}


def fit(X, labels, K, max_iter=100, tol=1e-3, reg_covar=1e-6, defect=None, dtype=np.float64, R=None):
    """Baum-Welch from a labelling, with the mixture's stopping rule -> dict(pi, A, means, covars, prec, n_iter, converged,
    why, log_likelihood, log_likelihoods, gamma, path, path_score, score, bic, aic, changes).  defects: the recursions', the
    posterior's, Viterbi's, "pi_not_updated", "bic_param_count_gmm" """
    X = np.asarray(X)
    N, Ld = X.shape
    labels = np.asarray(labels)
    mu, var, s = _mstep(X, G.one_hot(labels, K).astype(dtype), reg_covar, dtype)
    A = initial_transitions(labels, K).astype(dtype)
    pi = np.full(K, 1 / dtype(K), dtype=dtype)
    prev, history, why = -np.inf, [], "max_iter"
    for it in range(1, max_iter + 1):
        E = estep(X, pi, A, mu, s, defect, dtype, R)
        A = E["A_new"]
        if defect != "pi_not_updated":
            pi = E["pi_new"]
        mu, var, s = _mstep(X, E["gamma"], reg_covar, dtype)
        now = _mean(E["ll"], dtype)
        history.append(now)
        if E["bad"]:
            why = "degenerate"
            break
        if abs(now - prev) < tol:
            why = "converged"
            break
        prev = now
    E = estep(X, pi, A, mu, s, defect, dtype, R)
    f = lambda v: np.asarray(v).astype(np.float64)  # noqa: E731
    path, pscore, _ = viterbi(f(E["lb"]), log0(f(pi)), log0(f(A)), defect)
    score = _mean(E["ll"], dtype)
    bic, aic = criteria(score, N, K, Ld, defect)
    hist = np.array(history, dtype=np.float64)
    return {"pi": f(pi), "A": f(A), "means": f(mu), "covars": f(var), "prec": f(s), "n_iter": it, "converged": why == "converged",
            "why": why, "log_likelihood": float(hist[-1]), "log_likelihoods": hist, "gamma": f(E["gamma"]), "path": path,
            "path_score": pscore, "score": score, "bic": bic, "aic": aic,
            "changes": np.abs(np.diff(np.concatenate([[-np.inf], hist])))}


QUANTITIES = ("pi", "A", "means", "covars", "log_likelihoods", "gamma")
GATE_FACTOR = 64


def differences(a, b):
    """the largest absolute difference of every quantity of two fits (inf where the histories differ in length)"""
    out = {}
    for q in QUANTITIES:
        x, y = np.atleast_1d(a[q]), np.atleast_1d(b[q])
        out[q] = float(np.abs(x - y).max()) if x.shape == y.shape else np.inf
    out["n_iter"] = abs(a["n_iter"] - b["n_iter"])
    out["converged"] = int(a["converged"] != b["converged"])
    out["path"] = float((np.asarray(a["path"]) != np.asarray(b["path"])).mean())
    return out


def outside(diff, gates):
    """the quantities of `diff` outside the measured gates: GATE_FACTOR times the f64 / long double difference, n_iter and
    converged equal, the path equal on at least 99 % of the rows"""
    bad = [q for q in QUANTITIES if not diff[q] <= GATE_FACTOR * gates[q]]
    return bad + [q for q in ("n_iter", "converged") if diff[q] != 0] + (["path"] if not diff["path"] <= 0.01 else [])


# ---- cases -------------------------------------------------------------------------------------------------------------------

def ari(a, b):
    return Km.agreement(Km.contingency(a, b))["ari"]


def sticky_chain(N=1500, K=4, Ld=3, stay=0.95, sd=0.35, seed=0, spread=1.5):
    """a planted sticky chain with overlapping states -> (X f32 [N, L], the states [N]): state means uniform in a cube of
    side `spread`, the chain stays with probability `stay` and otherwise moves to another state uniformly"""
    r = np.random.RandomState(seed)
    mu = spread * r.rand(K, Ld)
    z = np.zeros(N, dtype=np.int64)
    z[0] = r.randint(K)
    for t in range(1, N):
        z[t] = z[t - 1] if r.rand() < stay or K == 1 else (z[t - 1] + 1 + r.randint(K - 1)) % K
    return (mu[z] + sd * r.randn(N, Ld)).astype(np.float32), z


def kmeans_labels(X, K, seed=42):
    """scikit-learn's KMeans(n_clusters=K, n_init=1, random_state=seed) as _kmeans_ref restates it"""
    X64 = np.asarray(X).astype(np.float64)
    return Km.lloyd(X, X64[Km.kmeans_pp(X, K, seed)])["labels"]


# seeds at which the restatement alone takes k-means' ARI of 0.66 and 0.60 to a Viterbi ARI of 0.97 and 0.93 (6 and 9 iterations)
PLANTED = {"sticky_a": dict(N=1500, K=4, Ld=3, stay=0.95, sd=0.35, seed=3),
           "sticky_b": dict(N=1500, K=4, Ld=3, stay=0.95, sd=0.35, seed=5)}


@functools.lru_cache(maxsize=None)
def planted(name):
    """-> (X, states, the k-means start, the f64 fit, the long double fit, the gates: their differences)"""
    X, z = sticky_chain(**PLANTED[name])
    K = PLANTED[name]["K"]
    start = kmeans_labels(X, K)
    f64, ld = fit(X, start, K), fit(X, start, K, dtype=LD)
    return X, z, start, f64, ld, differences(f64, ld)


@functools.lru_cache(maxsize=None)
def latents_case(K, seed):
    """the latents of tests/golden/latent_scores.npz from the recorded k-means start of tests/golden/gmm.npz -> (X, the start,
    the f64 fit, the long double fit, the gates)"""
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    X = np.load(os.path.join(here, "golden", "latent_scores.npz"))["X"]
    start = np.load(os.path.join(here, "golden", "gmm.npz"))[f"init_{K}_{seed}"]
    f64, ld = fit(X, start, K), fit(X, start, K, dtype=LD)
    return X, start, f64, ld, differences(f64, ld)


def random_chain(N, K, seed, kind="dense"):
    """-> (e [N, K] with a 1 in every row, m [N], pi, A): "dense", "sticky" (stay 0.95, emissions that overlap),
    "left_to_right" (A upper bidiagonal: zeros)"""
    r = np.random.RandomState(seed * 7919 + N * 64 + K)
    if kind == "left_to_right":
        A = np.zeros((K, K))
        for i in range(K):
            A[i, i] = 0.9 if i + 1 < K else 1.0
            if i + 1 < K:
                A[i, i + 1] = 0.1
        pi = np.full(K, 1.0 / K)
    elif kind == "sticky":
        A = np.full((K, K), 0.05 / max(K - 1, 1)) + (0.95 - 0.05 / max(K - 1, 1)) * np.eye(K) if K > 1 else np.ones((1, 1))
        pi = r.rand(K) + 0.1
        pi /= pi.sum()
    else:
        A = r.rand(K, K) + 0.01
        A /= A.sum(axis=1, keepdims=True)
        pi = r.rand(K) + 0.1
        pi /= pi.sum()
    lb = (1.0 if kind == "sticky" else 3.0) * r.randn(N, K)
    m = lb.max(axis=1)
    e = np.exp(lb - m[:, None])
    return e, m + 0.25 * r.randn(N), pi, A
