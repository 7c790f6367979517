"""Reference and bounds for the tests of the Bernoulli models of the hard codes (csrc/bernoulli.hip, bernoulli.py).

An f64 numpy restatement of the packing, the emissions, the E-step, the M-step and both fits in the orders include/rbvae_hip.h
states (blocked sums, l ascending, k ascending), written independently of the package; the recursions, the posterior, Viterbi
and the mean in the decision's order are tests/_hmm_ref.py's and tests/_gmm_ref.py's, which the kernels behind them were pinned
to.  Every function also runs in long double (dtype=LD), with plain sums.  tests/golden/bernoulli.npz
(tools/make_bernoulli_golden.py) pins one M-step and one E-step to scikit-learn's BernoulliNB.

Bounds.  u = 2^-53; every count is first order; the device's exp and log are taken as accurate to 2 ulp = 4 u relative, the
allowance of _gmm_ref and _hmm_ref.  References are long double rounded to f64 (ROUND).  X is 0/1, so a "product" r x is r or
0 exactly and a selected table entry is exact: only additions, quotients, exp and log round.
  lb       L additions of exact table entries, the first onto zero exact: |got - ref| <= (L - 1) u T, T = sum_l |the selected
           entries| (the partial sums of entries of one sign never exceed T; of mixed signs T still bounds them).
  lp       lb + log w rounds once: b_lp = (L - 1) u T + u |lp|.
  lognorm, resp, label      _gmm_ref's derivation with this b_lp:  b_ln = max_k b_lp + u (K + 4 + W + 4 |log S| + |lognorm|),
           b_r = resp_k (b_lp_k + b_ln + u |lp_k - lognorm| + 4 u).
  e        exp(lb_k - m): the argument is off by b_lb of both and rounds, exp 4 u: e (b_lb_k + b_lb_max + u |lb - m| + 4 u), with an
           absolute 1e-300 where e passes through the subnormal range (_hmm_ref).
  S, nk    N non-negative terms in any order: N u S, N u nk.
  theta    (S + p) / (nk + 2 p): numerator (N + 1) u, denominator (N + 1) u (2 p is exact), the quotient u: (2 N + 3) u theta.
  weights  nk' = nk + eps rounds (N + 1) u, the K additions K u, the quotient u: (2 N + K + 3) u w.
  logt, logw   from the DEVICE's own theta and weights (as _gmm_ref takes logc from the device's variances): 4 u |log|.
  logf     from the device's own S and nk: nk - S, + p, nk + 2 p and the quotient round once each, at most 4 u relative on the
           argument f = ((nk - S) + p) / (nk + 2 p) (nk - S >= -N u nk and p > 0 keep it positive; the first difference's
           rounding is relative to |nk - S| <= the numerator up to N u nk, which the same 4 u covers for p >= N u nk), which log
           passes on as 4 u absolute, and log's own 4 u |log f|:  u (4 + 4 |log f|).
  fits     n_iter, converged / why, labels and the path equal; every other quantity within GATE_FACTOR = 64 times its f64 / long
           double difference, the rule of tests/test_hmm_cpu.py.
scikit-learn (the fixture).  BernoulliNB takes log theta = log(S + a) - log(nk + 2 a), log(1 - theta) = log(1 - exp(log theta)),
log w = log nk - log N and lp = X (log theta - log(1 - theta))^T + sum_l log(1 - theta) + log w; numpy's log and exp are taken at
the same 4 u.  Against this restatement:
  d_t      |log theta|: ours u (the quotient, through log) + 4 u |log theta|; theirs 4 u (|log(S + a)| + |log(nk + 2 a)|) + u |log theta|.
  d_f      theirs: t = log theta is off by e_t = 4 u (|log(S + a)| + |log(nk + 2 a)|) + u |t|, so exp(t) by theta (e_t + 4 u) and
           1 - exp(t) by that + u (1 - theta): relative to 1 - theta, g = theta / (1 - theta) (e_t + 4 u) + u; log adds 4 u |log(1 -
           theta)|.  Ours u (4 + 4 |log f|) from exact counts.  d_f = g + 4 u + 8 u |log(1 - theta)|.
  d_w      theirs 4 u (|log nk| + |log N|) + u |log w|; ours nk' / sum nk' is off from nk / N by eps / nk + K eps / N + (K + 2) u
           relative, and log adds 4 u |log w|.
  lp       sum_l (x d_t + (1 - x) d_f) + d_w; our sum (L - 1) u T + u |lp|; theirs: 2 L + 2 roundings in any order on terms whose
           absolute values add to Q = sum_l x |log theta - log(1 - theta)| + sum_l |log(1 - theta)| + |log w|, and the difference
           log theta - log(1 - theta) rounds once: (2 L + 3) u Q.
  resp     both sides evaluate the softmax: resp (2 max_k b_lp + 2 u (K + 8 + W + 4 |log S| + |lognorm|) + 2 u |lp - lognorm|).
"""
import functools
import os

import numpy as np

import _gmm_ref as G
import _hmm_ref as H
from _projection_ref import TINY, U, rejects, within  # noqa: F401

LD = np.longdouble
NK_EPS = G.NK_EPS
BN_CHUNK = 4096                         # f64 values of the interleaved log tables per LDS chunk
ROUND = G.ROUND
SUBNORMAL = H.SUBNORMAL
GATE_FACTOR = H.GATE_FACTOR
HERE = os.path.dirname(os.path.abspath(__file__))


def ok(N, L, K):
    return 1 <= L <= 128 and 1 <= K <= 256 and K <= N <= 1 << 20 and N * K <= 1 << 26


def chunk_components(L):
    return BN_CHUNK // (2 * L)


def ws_bytes(N, L, K):
    return 8 * G.blocks_rows(N)[0] * K * (L + 1)


def as_bits(X):
    """X [N, L] of any values -> bool [N, L]: x > 0.5 (NaN: False)"""
    with np.errstate(invalid="ignore"):
        return np.asarray(X) > 0.5


def pack(X):
    """-> uint32 [N, 4]: bit l of a row in word l // 32 at position l % 32, zeros from L upward"""
    b = as_bits(X)
    N, L = b.shape
    full = np.zeros((N, 128), dtype=np.uint64)
    full[:, :L] = b
    w = (full.reshape(N, 4, 32) << np.arange(32, dtype=np.uint64)[None, None, :]).sum(axis=2)
    return w.astype(np.uint32)


def planted_chain(N, L, K, flip, stay, seed):
    """-> (X f32 [N, L] of 0 / 1, the states int64 [N], the prototypes bool [K, L]), drawn from RandomState(seed) in this
    order: proto = rand(K, L) < 0.5; s_0 = 0; s_t = s_(t-1) if rand() < stay else randint(K); X = proto[s] ^ (rand(N, L) < flip)"""
    r = np.random.RandomState(seed)
    proto = r.rand(K, L) < 0.5
    s = np.zeros(N, dtype=np.int64)
    for t in range(1, N):
        s[t] = s[t - 1] if r.rand() < stay else r.randint(K)
    X = proto[s] ^ (r.rand(N, L) < flip)
    return X.astype(np.float32), s, proto


# ---- emissions and the E-step ------------------------------------------------------------------------------------------------

def table_sums(X, logt, logf, dtype=np.float64):
    """-> (lb [N, K] = sum_l (bit ? logt_kl : logf_kl), l ascending from zero, every addition rounded in `dtype`;
    T [N, K] = the sum of the selected entries' absolute values, in long double)"""
    b = as_bits(X)
    logt, logf = np.asarray(logt).astype(dtype), np.asarray(logf).astype(dtype)
    lb = np.zeros((len(b), len(logt)), dtype=dtype)
    T = np.zeros((len(b), len(logt)), dtype=LD)
    for l in range(b.shape[1]):
        sel = np.where(b[:, l, None], logt[None, :, l], logf[None, :, l])
        lb = lb + sel
        T = T + np.abs(sel)
    return lb, T


def emit(X, logt, logf, dtype=np.float64):
    """-> (lb [N, K], m [N], e [N, K])"""
    lb, _ = table_sums(X, logt, logf, dtype)
    m = lb.max(axis=1)
    with np.errstate(under="ignore"):
        e = np.exp(lb - m[:, None])
    return lb, m, e


def _b_lb(X, logt, logf):
    L = np.asarray(X).shape[1]
    lb, T = table_sums(X, logt, logf, LD)
    return lb, ((L - 1) * U * T).astype(np.float64)


def emit_bounds(X, logt, logf):
    lb, b_lb = _b_lb(X, logt, logf)
    m = lb.max(axis=1)
    with np.errstate(under="ignore"):
        e = np.exp(lb - m[:, None])
    f = lambda v: v.astype(np.float64)  # noqa: E731
    b_e = f(e) * (b_lb + b_lb.max(axis=1)[:, None] + U * f(np.abs(lb - m[:, None])) + 4 * U) + SUBNORMAL
    return {"lb": f(lb), "m": f(m), "e": f(e), "b_lb": b_lb + ROUND(f(lb)), "b_m": b_lb.max(axis=1) + ROUND(f(m)),
            "b_e": b_e + ROUND(f(e))}


def estep(X, logt, logf, logw, dtype=np.float64):
    """-> (lp [N, K], lognorm [N], resp [N, K], label [N]): lp = lb + logw (added last), k ascending, ties to the lower k"""
    lb, _ = table_sums(X, logt, logf, dtype)
    lp = lb + np.asarray(logw).astype(dtype)[None, :]
    K = lp.shape[1]
    m = lp.max(axis=1)
    S = np.zeros(len(lp), dtype=dtype)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore", under="ignore"):
        for k in range(K):
            S = S + np.exp(lp[:, k] - m)
        lognorm = m + np.log(S)
        resp = np.exp(lp - lognorm[:, None])
    return lp, lognorm, resp, np.argmax(lp, axis=1).astype(np.int32)


def softmax_bounds(lp, b_lp):
    """lp [N, K] long double and its bound -> (lognorm, resp, W, S, b_ln, b_r) by _gmm_ref's derivation"""
    K = lp.shape[1]
    m = lp.max(axis=1)
    a = lp - m[:, None]
    with np.errstate(under="ignore"):
        e = np.exp(a)
    S = e.sum(axis=1)
    lognorm = m + np.log(S)
    with np.errstate(under="ignore"):
        resp = np.exp(lp - lognorm[:, None])
    W = (e * np.abs(a)).sum(axis=1) / S
    b_ln = b_lp.max(axis=1) + U * (K + 4 + W + 4 * np.abs(np.log(S)) + np.abs(lognorm)).astype(np.float64)
    b_r = (resp * (b_lp + b_ln[:, None] + U * np.abs(lp - lognorm[:, None]) + 4 * U)).astype(np.float64)
    return lognorm, resp, W, S, b_ln, b_r


def estep_bounds(X, logt, logf, logw):
    lb, b_lb = _b_lb(X, logt, logf)
    lp = lb + np.asarray(logw).astype(LD)[None, :]
    b_lp = b_lb + (U * np.abs(lp)).astype(np.float64)
    lognorm, resp, _, _, b_ln, b_r = softmax_bounds(lp, b_lp)
    K = lp.shape[1]
    if K > 1:
        order = np.argsort(-lp, axis=1, kind="stable")
        rows = np.arange(len(lp))
        top, second = order[:, 0], order[:, 1]
        decided = (lp[rows, top] - lp[rows, second]).astype(np.float64) > b_lp[rows, top] + b_lp[rows, second]
    else:
        decided = np.ones(len(lp), dtype=bool)
    f = lambda v: v.astype(np.float64)  # noqa: E731
    return {"lp": f(lp), "lognorm": f(lognorm), "resp": f(resp), "label": np.argmax(lp, axis=1).astype(np.int32),
            "decided": decided, "b_lp": b_lp + ROUND(f(lp)), "b_ln": b_ln + ROUND(f(lognorm)), "b_r": b_r + ROUND(f(resp)) + SUBNORMAL}


# ---- M-step ------------------------------------------------------------------------------------------------------------------

def block_partials(X, resp):
    """resp [N, K] f64 -> f64 [blocks, K, L + 1]: the workspace of rbvae_bern_mstep, every cell's rows added in ascending order
    from zero (a term is r_ki or not there: adding the exact 0 of r * 0 changes nothing)"""
    b = as_bits(X).astype(np.float64)
    resp = np.asarray(resp, dtype=np.float64)
    N, L = b.shape
    blocks, rows = G.blocks_rows(N)
    out = np.zeros((blocks, resp.shape[1], L + 1))
    for blk in range(blocks):
        part = np.zeros((resp.shape[1], L + 1))
        for r in range(blk * rows, min(N, (blk + 1) * rows)):
            part[:, :L] = part[:, :L] + resp[r][:, None] * b[r][None, :]
            part[:, L] = part[:, L] + resp[r]
        out[blk] = part
    return out


def block_totals(partials):
    """the partials in block order from zero -> (S [K, L], nk [K])"""
    tot = np.zeros(partials.shape[1:])
    for blk in range(partials.shape[0]):
        tot = tot + partials[blk]
    return tot[:, :-1], tot[:, -1]


def finish(S, nk, prior, dtype=np.float64):
    """-> (weights, logw, theta, logt, logf) from the sums"""
    S, nk, p = np.asarray(S).astype(dtype), np.asarray(nk).astype(dtype), dtype(prior)
    den = nk + dtype(2) * p
    theta = (S + p) / den[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        logt = np.log(theta)
        logf = np.log(((nk[:, None] - S) + p) / den[:, None])
        tot = dtype(0)
        for k in range(len(nk)):
            tot = tot + (nk[k] + dtype(NK_EPS))
        weights = (nk + dtype(NK_EPS)) / tot
        logw = np.log(weights)
    return weights, logw, theta, logt, logf


def mstep(X, resp, prior=1.0, dtype=np.float64):
    """resp [N, K] -> dict(weights, logw, theta, logt, logf, S, nk): the blocked order in f64, plain sums in long double"""
    if dtype == np.float64:
        S, nk = block_totals(block_partials(X, resp))
    else:
        b, R = as_bits(X).astype(LD), np.asarray(resp).astype(LD)
        S, nk = R.T @ b, R.sum(axis=0)
    w, logw, theta, logt, logf = finish(S, nk, prior, dtype)
    return {"weights": w, "logw": logw, "theta": theta, "logt": logt, "logf": logf, "S": S, "nk": nk}


def mstep_bounds(X, resp, prior, dev):
    """long double references (resp [N, K] f64 as given) and the bounds of the docstring; dev: the device's (or the f64
    restatement's) dict(S, nk, theta, weights), from which the three log tables follow"""
    N = len(np.asarray(X))
    K = np.asarray(resp).shape[1]
    ld = mstep(X, resp, prior, LD)
    dS, dnk, dth, dw = (np.asarray(dev[n]).astype(LD) for n in ("S", "nk", "theta", "weights"))
    p = LD(prior)
    logt, logw = np.log(dth), np.log(dw)
    logf = np.log(((dnk[:, None] - dS) + p) / (dnk[:, None] + 2 * p))
    f = lambda a: np.asarray(a).astype(np.float64)  # noqa: E731
    return {"S": f(ld["S"]), "nk": f(ld["nk"]), "theta": f(ld["theta"]), "weights": f(ld["weights"]), "logt": f(logt),
            "logf": f(logf), "logw": f(logw),
            "b_S": N * U * f(ld["S"]) + ROUND(f(ld["S"])), "b_nk": N * U * f(ld["nk"]) + ROUND(f(ld["nk"])),
            "b_theta": (2 * N + 3) * U * f(ld["theta"]) + ROUND(f(ld["theta"])),
            "b_weights": (2 * N + K + 3) * U * f(ld["weights"]) + ROUND(f(ld["weights"])),
            "b_logt": 4 * U * np.abs(f(logt)) + ROUND(f(logt)), "b_logw": 4 * U * np.abs(f(logw)) + ROUND(f(logw)),
            "b_logf": U * (4 + 4 * np.abs(f(logf))) + ROUND(f(logf))}


# ---- scikit-learn's forms (the fixture) -----------------------------------------------------------------------------------------

def sklearn_bounds(X, labels, K, alpha):
    """the bounds of the docstring's last block for the one-hot M-step of `labels` and its E-step on X -> dict(d_t, d_f, d_w,
    b_lp, b_r), from long double values"""
    b = as_bits(X).astype(LD)
    N, L = b.shape
    R = G.one_hot(labels, K).astype(LD)
    S, nk, a = R.T @ b, R.sum(axis=0), LD(alpha)
    num, den = S + a, nk + 2 * a
    theta = num / den[:, None]
    t, f1 = np.log(theta), np.log1p(-theta)
    w = np.log(nk / N)
    e_t = 4 * U * (np.abs(np.log(num)) + np.abs(np.log(den))[:, None]) + U * np.abs(t)
    d_t = U + 4 * U * np.abs(t) + e_t
    g = theta / (1 - theta) * (e_t + 4 * U) + U
    d_f = g + 4 * U + 8 * U * np.abs(f1)
    d_w = (4 * U * (np.abs(np.log(nk)) + np.log(LD(N))) + U * np.abs(w) + NK_EPS / nk + K * NK_EPS / N + (K + 2) * U
           + 4 * U * np.abs(w))
    lp = b @ t.T + (1 - b) @ f1.T + w[None, :]
    T = b @ np.abs(t).T + (1 - b) @ np.abs(f1).T
    Q = b @ np.abs(t - f1).T + np.abs(f1).sum(axis=1)[None, :] + np.abs(w)[None, :]
    b_lp = (b @ d_t.T + (1 - b) @ d_f.T + d_w[None, :] + (L - 1) * U * T + U * np.abs(lp) + (2 * L + 3) * U * Q).astype(np.float64)
    lognorm, resp, W, Ssum, _, _ = softmax_bounds(lp, b_lp)
    own = U * (K + 8 + W + 4 * np.abs(np.log(Ssum)) + np.abs(lognorm)).astype(np.float64)
    b_r = (resp * (2 * b_lp.max(axis=1)[:, None] + 2 * own[:, None] + 2 * U * np.abs(lp - lognorm[:, None]))).astype(np.float64)
    f = lambda v: np.asarray(v).astype(np.float64)  # noqa: E731
    return {"d_t": f(d_t) + TINY, "d_f": f(d_f) + TINY, "d_w": f(d_w) + TINY, "b_lp": b_lp + TINY, "b_r": b_r + SUBNORMAL}


# ---- the fits ----------------------------------------------------------------------------------------------------------------

def _mean(v, dtype):
    return G.lower_bound(v) if dtype == np.float64 else float(v.sum() / len(v))


def bmm_n_parameters(K, L):
    return K * L + K - 1


def bhmm_n_parameters(K, L):
    return (K - 1) + K * (K - 1) + K * L


def criteria(score, N, p):
    return -2.0 * score * N + p * np.log(N), -2.0 * score * N + 2.0 * p


def bmm_fit(X, labels, K, max_iter=100, tol=1e-3, prior=1.0, dtype=np.float64):
    """mixture.gmm's loop from the one-hot start -> dict(weights, probs, logt, logf, logw, n_iter, converged, lower_bound,
    lower_bounds, labels, resp (the final E-step's), score_samples, score, bic, aic, changes)"""
    X = np.asarray(X)
    N, L = X.shape
    M = mstep(X, G.one_hot(np.asarray(labels), K).astype(dtype), prior, dtype)
    prev, history, converged = -np.inf, [], False
    for it in range(1, max_iter + 1):
        _, lognorm, resp, _ = estep(X, M["logt"], M["logf"], M["logw"], dtype)
        M = mstep(X, resp, prior, dtype)
        lb = _mean(lognorm, dtype)
        history.append(lb)
        if abs(lb - prev) < tol:
            converged = True
            break
        prev = lb
    _, lognorm, resp, label = estep(X, M["logt"], M["logf"], M["logw"], dtype)
    score = _mean(lognorm, dtype)
    bic, aic = criteria(score, N, bmm_n_parameters(K, L))
    f = lambda v: np.asarray(v).astype(np.float64)  # noqa: E731
    hist = np.array(history, dtype=np.float64)
    return {"weights": f(M["weights"]), "probs": f(M["theta"]), "logt": f(M["logt"]), "logf": f(M["logf"]), "logw": f(M["logw"]),
            "n_iter": it, "converged": converged, "lower_bound": float(hist[-1]), "lower_bounds": hist, "labels": label,
            "resp": f(resp), "score_samples": f(lognorm), "score": score, "bic": bic, "aic": aic,
            "changes": np.abs(np.diff(np.concatenate([[-np.inf], hist])))}


def bhmm_estep(X, pi, A, logt, logf, dtype=np.float64, R=None):
    lb, m, e = emit(X, logt, logf, dtype)
    alpha, ll, sa = H.forward(e, m, pi, A, None, dtype, R)
    beta, sb = H.backward(e, A, None, dtype, R)
    gamma, Xi, A_new, pi_new, sp = H.posterior(alpha, beta, e, A, None, dtype)
    return {"lb": lb, "ll": ll, "gamma": gamma, "A_new": A_new, "pi_new": pi_new, "bad": sa[0] + sb[0] + sp[0]}


def bhmm_fit(X, labels, K, max_iter=100, tol=1e-3, prior=1.0, dtype=np.float64, R=None):
    """hmm.hmm's iteration with Bernoulli emissions, from a labelling -> dict(pi, A, probs, logt, logf, n_iter, converged, why,
    log_likelihood, log_likelihoods, gamma, path, path_score, score, bic, aic, changes).  R: the recursions' block_rows (None:
    the plain recursion)"""
    X = np.asarray(X)
    N, L = X.shape
    labels = np.asarray(labels)
    M = mstep(X, G.one_hot(labels, K).astype(dtype), prior, dtype)
    A = H.initial_transitions(labels, K).astype(dtype)
    pi = np.full(K, 1 / dtype(K), dtype=dtype)
    prev, history, why = -np.inf, [], "max_iter"
    for it in range(1, max_iter + 1):
        E = bhmm_estep(X, pi, A, M["logt"], M["logf"], dtype, R)
        A, pi = E["A_new"], E["pi_new"]
        M = mstep(X, E["gamma"], prior, dtype)
        now = _mean(E["ll"], dtype)
        history.append(now)
        if E["bad"]:
            why = "degenerate"
            break
        if abs(now - prev) < tol:
            why = "converged"
            break
        prev = now
    E = bhmm_estep(X, pi, A, M["logt"], M["logf"], dtype, R)
    f = lambda v: np.asarray(v).astype(np.float64)  # noqa: E731
    path, pscore, _ = H.viterbi(f(E["lb"]), H.log0(f(pi)), H.log0(f(A)))
    score = _mean(E["ll"], dtype)
    bic, aic = criteria(score, N, bhmm_n_parameters(K, L))
    hist = np.array(history, dtype=np.float64)
    return {"pi": f(pi), "A": f(A), "probs": f(M["theta"]), "logt": f(M["logt"]), "logf": f(M["logf"]), "n_iter": it,
            "converged": why == "converged", "why": why, "log_likelihood": float(hist[-1]), "log_likelihoods": hist,
            "gamma": f(E["gamma"]), "path": path, "path_score": pscore, "score": score, "bic": bic, "aic": aic,
            "changes": np.abs(np.diff(np.concatenate([[-np.inf], hist])))}


BMM_QUANTITIES = ("weights", "probs", "lower_bounds", "resp")
BHMM_QUANTITIES = ("pi", "A", "probs", "log_likelihoods", "gamma")


def differences(a, b, quantities, labels):
    """the largest absolute difference of every quantity of two fits (inf where the histories differ in length), and the
    share of rows on which `labels` ("labels" or "path") differ"""
    out = {}
    for q in quantities:
        x, y = np.atleast_1d(a[q]), np.atleast_1d(b[q])
        out[q] = float(np.abs(x - y).max()) if x.shape == y.shape else np.inf
    out["n_iter"] = abs(a["n_iter"] - b["n_iter"])
    out["converged"] = int(a["converged"] != b["converged"])
    out[labels] = float((np.asarray(a[labels]) != np.asarray(b[labels])).mean())
    return out


def outside(diff, gates, quantities, labels):
    """the quantities of `diff` outside the gates: GATE_FACTOR times the f64 / long double difference; n_iter, converged and
    every label equal"""
    bad = [q for q in quantities if not diff[q] <= GATE_FACTOR * gates[q]]
    return bad + [q for q in ("n_iter", "converged", labels) if diff[q] != 0]


# ---- cases -------------------------------------------------------------------------------------------------------------------

# (N, L, K, flip, stay, seed) and the seed of _kmeans_ref's start.  From scikit-learn's own KMeans(seed 42) labelling of
# nine_states (ARI 0.285) the restatement reaches a Viterbi ARI of 0.922 in 10 iterations, the closest stop decision 3.46e-4
# from tol; _kmeans_ref's seed 42 labelling is another one (ARI 0.273; integer distances tie) and leads to 0.809 in 15
# iterations with a decision 2.6e-5 from tol.  Seed 9 is a start from which the restatement alone meets the conditions of
# tests/test_bernoulli_cpu.py: 0.324 -> 0.929 in 10 iterations, 3.47e-4.  hundred_bits: 0.838 -> 0.988 in 4, 4.83e-4.
PLANTED = {"nine_states": (900, 25, 9, 0.3, 0.92, 2), "hundred_bits": (600, 100, 5, 0.35, 0.9, 3)}
START_SEED = {"nine_states": 9, "hundred_bits": 42, "fixture": 42}
FIXTURE = (600, 32, 5, 0.2, 0.9, 1)     # tools/make_bernoulli_golden.py


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(os.path.join(HERE, "golden", "bernoulli.npz")))


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (X f32, the states, the k-means start of _kmeans_ref, K): a planted chain, or "fixture": the codes of
    tests/golden/bernoulli.npz"""
    if name == "fixture":
        g = golden()
        X, s, K = g["X"].astype(np.float32), g["states"].astype(np.int64), FIXTURE[2]
    else:
        X, s, _ = planted_chain(*PLANTED[name])
        K = PLANTED[name][2]
    return X, s, H.kmeans_labels(X, K, START_SEED[name]), K


@functools.lru_cache(maxsize=None)
def fitted(name, model):
    """model "bmm" or "bhmm" -> (the f64 fit, the long double fit, the gates: their differences), computed once"""
    X, s, start, K = case(name)
    fit, q, lab = (bmm_fit, BMM_QUANTITIES, "labels") if model == "bmm" else (bhmm_fit, BHMM_QUANTITIES, "path")
    f64, ld = fit(X, start, K), fit(X, start, K, dtype=LD)
    return f64, ld, differences(f64, ld, q, lab)


def tables_case(N, L, K, seed=0):
    """codes with a few values at and just above 0.5, and log tables of probabilities in (0.02, 0.98): f64 noise, so every
    addition rounds -> (X f32 [N, L], logt, logf, logw)"""
    r = np.random.RandomState(1000 * N + 10 * L + K + seed)
    X = (r.rand(N, L) < 0.5).astype(np.float32)
    X[r.rand(N, L) < 0.05] = 0.5
    X[r.rand(N, L) < 0.05] = np.nextafter(np.float32(0.5), np.float32(1))
    theta = 0.02 + 0.96 * r.rand(K, L)
    w = 0.2 + r.rand(K)
    w /= w.sum()
    return X, np.log(theta), np.log1p(-theta), np.log(w)
