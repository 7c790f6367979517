"""Reference and bounds for the hidden Markov model over several stacked sequences (the rbvae_hmm_seq_ entries of
csrc/hmm.hip, hmm.py's lengths=).

The recursions and Viterbi are tests/_hmm_ref.py's forward / backward / viterbi applied to every sequence on its own (so the
blocks restart at every sequence and no sequence sees another); the posterior, Xi and pi are restated here on the stacked
rows in the orders include/rbvae_hip.h states: gamma for every row, Xi as the two-stage sum over blocks_rows(N) blocks of the
stacked rows with the terms that end a sequence skipped, pi_new_k = (sum_s gamma_k,first(s)) / S as one running sum with s
ascending.  Every function also runs in long double (dtype=LD) and takes a `defect` name: the restatement with one named
mistake, which tests/test_hmm_seq_cpu.py uses to show that the check meant to catch that mistake does.

Bounds are _hmm_ref's with n counted inside the sequence: rho(n) of alpha has n = t - first(s) + 1, of beta n = last(s) - t,
and the blocks a path passes in launch (ii) are its own sequence's.  gamma: as there.  Xi: a term is off by rho_a(t) +
rho_b(t + 1) + 3 u over the terms that exist, and at most N of them are added: Xi (2 max + (K^2 + N + 7) u), the bound stated
there.  pi_new: every gamma_k,first(s) is off by its rg, S additions and one division: pi_new (max_s rg + (S + 1) u).
sum_ij Xi_ij = N - S within (N - S) (K^2 + N + 3) u (N - S rows of K^2 quotients are added).
"""
import functools

import numpy as np

import _gmm_ref as G
import _hmm_ref as R

LD, U, NO_ROW, EPS, ROUND, SUBNORMAL = R.LD, R.U, R.NO_ROW, R.EPS, R.ROUND, R.SUBNORMAL
DEFECTS = ("no_reset_at_start", "beta_not_reset", "boundary_pair_counted", "pi_first_sequence_only", "pi_not_divided",
           "blocks_on_stacked_rows", "viterbi_crosses_boundary", "initial_A_counts_boundary")

# the length lists of tests/test_hmm_seq_gpu.py
LENGTHS = {"ones": (1, 1), "pair": (2,), "mixed": (1, 63, 64, 65, 1, 129), "even": (64, 64, 64), "tail": (65, 1, 1, 200),
           "long": (4097, 1), "many": tuple((1, 2, 3)[i % 3] for i in range(300)), "single": (129,)}


def spans(lengths):
    first = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return [(int(a), int(b)) for a, b in zip(first[:-1], first[1:])]


def ends(lengths):
    """bool [N]: row t is the last of its sequence"""
    out = np.zeros(int(np.sum(lengths)), dtype=bool)
    out[np.cumsum(lengths) - 1] = True
    return out


# ---- the plan ------------------------------------------------------------------------------------------------------------------

def max_blocks(N, S, Rr):
    return min(N, -(-N // min(Rr, N)) + S)


def plan_bytes(N, S, Rr):
    return 4 * (6 + 2 * S + N + max_blocks(N, S, Rr))


def ws_bytes(N, K, S, Rr):
    return 8 * max(max_blocks(N, S, Rr) * (K * K + 2 * K), N + G.blocks_rows(N)[0] * K * K)


def plan(lengths, Rr):
    """the device plan, int32: {S, N, block_rows, B}, row [S + 1], end [N], blk [S + 1], seq [maxb] (zeros behind B)"""
    S, N = len(lengths), int(np.sum(lengths))
    Rr = min(Rr, N)
    nb = [-(-n // Rr) for n in lengths]
    seq = np.zeros(max_blocks(N, S, Rr), dtype=np.int64)
    seq[:sum(nb)] = np.repeat(np.arange(S), nb)
    return np.concatenate([[S, N, Rr, sum(nb)], np.concatenate([[0], np.cumsum(lengths)]), ends(lengths).astype(np.int64),
                           np.concatenate([[0], np.cumsum(nb)]), seq]).astype(np.int32)


def ok(N, L, K, S):
    return R.ok(N, L, K) and 1 <= S <= N


# ---- the recurrence --------------------------------------------------------------------------------------------------------------

def _blocked(e, m, pi, A, fwd, cuts, dtype):
    """_hmm_ref's blocked recurrence in the three launches' order with the blocks [cuts[b], cuts[b + 1]) -> (out, ll); for the
    defect "blocks_on_stacked_rows" (with _hmm_ref's own cuts it equals _hmm_ref bit for bit: test_hmm_seq_cpu.py)"""
    e, A = np.asarray(e).astype(dtype), np.asarray(A).astype(dtype)
    N, K = e.shape
    out, ll = np.zeros((N, K), dtype=dtype), np.zeros(N, dtype=dtype)
    span = list(zip(cuts[:-1], cuts[1:]))
    order = list(range(len(span))) if fwd else list(range(len(span) - 1, -1, -1))
    own = order[0]

    def rows(b):
        lo, hi = span[b]
        if fwd:
            return [(t, t) for t in range(max(lo, 1) if b == own else lo, hi)]
        return [(t, t + 1) for t in range((N - 2) if b == own else hi - 1, lo - 1, -1)]

    def first():
        if not fwd:
            return np.full(K, 1 / dtype(K), dtype=dtype), None
        y = np.asarray(pi).astype(dtype) * e[0]
        return y, R.wsum(y)

    def step(v, r):
        y = R._step(v, e[r], A, fwd)
        return y, R.wsum(y)

    with np.errstate(all="ignore"):
        Us, Ss = {}, {}
        for b in order[:-1]:
            if b == own:
                y, z = first()
                V = ((y / z if z > 0 else np.zeros(K, dtype=dtype)) if fwd else y)[None, :]
                s = np.zeros(1, dtype=dtype)
            else:
                V, s = np.eye(K, dtype=dtype), np.zeros(K, dtype=dtype)
            for t, r in rows(b):
                Y, z = step(V, r)
                V = np.where(z[:, None] > 0, Y / z[:, None], 0)
                s = s + np.log(z)
            Us[b], Ss[b] = V, s
        vin = {}
        if len(order) > 1:
            v = Us[own][0]
            vin[order[1]] = v
            for n in range(1, len(order) - 1):
                b = order[n]
                s = Ss[b]
                w = np.where(np.isneginf(s), 0, v * np.exp(s - s.max()))
                y = R.dot(w, Us[b])
                z = R.wsum(y)
                v = y / z if z > 0 else np.zeros(K, dtype=dtype)
                vin[order[n + 1]] = v
        for b in order:
            if b == own:
                y, z = first()
                v = y / z if fwd else y
                out[0 if fwd else N - 1] = v
                if fwd:
                    ll[0] = np.log(z) + np.asarray(m).astype(dtype)[0]
            else:
                v = vin[b]
            for t, r in rows(b):
                y, z = step(v, r)
                v = y / z
                out[t] = v
                if fwd:
                    ll[t] = np.log(z) + np.asarray(m).astype(dtype)[t]
    return out, ll


def own_cuts(n, Rr):
    return list(range(0, n, Rr)) + [n]


def _stacked_cuts(lo, hi, Rr):
    """the cuts of [lo, hi) at the multiples of Rr counted from the stack's first row, relative to lo"""
    inner = [c - lo for c in range((lo // Rr + 1) * Rr, hi, Rr)]
    return [0] + inner + [hi - lo]


def _shift(status, lo):
    return [status[0], status[1] + lo if status[0] else NO_ROW]


def _merge(statuses):
    return [sum(s[0] for s in statuses), min(s[1] for s in statuses)]


def forward(e, m, pi, A, lengths, defect=None, dtype=np.float64, R_=None):
    """-> (alpha [N, K], ll [N], status): _hmm_ref.forward per sequence.  defects: "no_reset_at_start" (the stack taken as one
    sequence), "blocks_on_stacked_rows" """
    if defect == "no_reset_at_start":
        return R.forward(e, m, pi, A, dtype=dtype, R=R_)
    e, m = np.asarray(e), np.asarray(m)
    al, ll, st = np.zeros(e.shape, dtype=dtype), np.zeros(len(e), dtype=dtype), []
    for lo, hi in spans(lengths):
        if defect == "blocks_on_stacked_rows" and R_ is not None:
            a, l = _blocked(e[lo:hi], m[lo:hi], pi, A, True, _stacked_cuts(lo, hi, R_), dtype)
            s = [0, NO_ROW]
        else:
            a, l, s = R.forward(e[lo:hi], m[lo:hi], pi, A, dtype=dtype, R=R_)
        al[lo:hi], ll[lo:hi] = a, l
        st.append(_shift(s, lo))
    return al, ll, _merge(st)


def backward(e, A, lengths, defect=None, dtype=np.float64, R_=None):
    """-> (beta [N, K], status).  defects: "beta_not_reset", "blocks_on_stacked_rows" """
    if defect == "beta_not_reset":
        return R.backward(e, A, dtype=dtype, R=R_)
    e = np.asarray(e)
    be, st = np.zeros(e.shape, dtype=dtype), []
    for lo, hi in spans(lengths):
        if defect == "blocks_on_stacked_rows" and R_ is not None:
            b, s = _blocked(e[lo:hi], None, None, A, False, _stacked_cuts(lo, hi, R_), dtype)[0], [0, NO_ROW]
        else:
            b, s = R.backward(e[lo:hi], A, dtype=dtype, R=R_)
        be[lo:hi] = b
        st.append(_shift(s, lo))
    return be, _merge(st)


# ---- the posterior ---------------------------------------------------------------------------------------------------------------

def posterior(alpha, beta, e, A, lengths, defect=None, dtype=np.float64):
    """-> (gamma [N, K], Xi [K, K], A_new [K, K], pi_new [K], status) on the stacked rows.  defects: "boundary_pair_counted",
    "pi_first_sequence_only", "pi_not_divided" """
    alpha, beta, e, A = (np.asarray(a).astype(dtype) for a in (alpha, beta, e, A))
    N, K = alpha.shape
    S = len(lengths)
    pair = ~ends(lengths)[:N - 1] if defect != "boundary_pair_counted" else np.ones(N - 1, dtype=bool)
    with np.errstate(all="ignore"):
        g = np.zeros(N, dtype=dtype)
        for k in range(K):
            g = g + alpha[:, k] * beta[:, k]
        gamma = (alpha * beta) / g[:, None]
        w = e[1:] * beta[1:]
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
                    if pair[lo + r]:
                        part = part + terms[r]
            Xi = Xi + part
        rs = np.zeros(K, dtype=dtype)
        for j in range(K):
            rs = rs + Xi[:, j]
        A_new = (Xi + dtype(EPS) / K) / (rs[:, None] + dtype(EPS))
        if defect == "pi_first_sequence_only":
            pi_new = gamma[0].copy()
        else:
            pi_new = np.zeros(K, dtype=dtype)
            for lo, _ in spans(lengths):
                pi_new = pi_new + gamma[lo]
            if defect != "pi_not_divided":
                pi_new = pi_new / dtype(S)
    bad = [t for t in range(N) if R._bad(g[t])] + [t for t in range(N - 1) if pair[t] and R._bad(Z[t])]
    return gamma, Xi, A_new, pi_new, [len(bad), min(bad) if bad else NO_ROW]


# ---- Viterbi ---------------------------------------------------------------------------------------------------------------------

def viterbi(logb, lpi, lA, lengths, defect=None):
    """-> (path [N] int32, scores [S], back [N, K] uint8): _hmm_ref.viterbi per sequence.  defect "viterbi_crosses_boundary":
    one path through the stack, its score in scores[0]"""
    logb = np.asarray(logb, dtype=np.float64)
    if defect == "viterbi_crosses_boundary":
        path, score, back = R.viterbi(logb, lpi, lA)
        return path, np.array([score] + [0.0] * (len(lengths) - 1)), back
    path, back, scores = np.zeros(len(logb), dtype=np.int32), np.zeros(logb.shape, dtype=np.uint8), []
    for lo, hi in spans(lengths):
        p, s, b = R.viterbi(logb[lo:hi], lpi, lA)
        path[lo:hi], back[lo:hi] = p, b
        scores.append(s)
    return path, np.array(scores, dtype=np.float64), back


def sum_ascending(a):
    s = np.float64(0.0)
    for x in np.asarray(a, dtype=np.float64):
        s = s + x
    return float(s)


def sequence_scores(ll, lengths):
    """every sequence's sum of ll_t, t ascending"""
    return np.array([sum_ascending(ll[lo:hi]) for lo, hi in spans(lengths)])


def change_points(path, lengths):
    path = np.asarray(path)
    starts = {lo for lo, _ in spans(lengths)}
    return [t for t in range(1, len(path)) if path[t] != path[t - 1] and t not in starts]


# ---- all paths -------------------------------------------------------------------------------------------------------------------

def brute(logb, pi, A, lengths):
    """_hmm_ref.brute per sequence -> (the log-likelihood of all sequences: the likelihoods multiplied, gamma [N, K], Xi [K, K]
    added over the sequences, the best paths joined, the smallest margin)"""
    logb = np.asarray(logb)
    ll, gamma, Xi, path, margin = 0.0, [], 0.0, [], np.inf
    for lo, hi in spans(lengths):
        l, g, x, p, mg = R.brute(logb[lo:hi], pi, A)
        ll, Xi, margin = ll + l, Xi + x, min(margin, mg)
        gamma.append(g)
        path.append(p)
    return ll, np.concatenate(gamma), Xi, np.concatenate(path), margin


# ---- bounds ----------------------------------------------------------------------------------------------------------------------

def ld_passes(e, m, pi, A, lengths):
    """the long double recursions of every sequence, to be shared by several calls of recurrence_bounds"""
    e, m = np.asarray(e), np.asarray(m)
    return [R.ld_passes(e[lo:hi], m[lo:hi], pi, A) for lo, hi in spans(lengths)]


def recurrence_bounds(e, m, pi, A, lengths, R_=None, ld=None):
    """_hmm_ref.recurrence_bounds per sequence, stacked: the long double references and the bounds with rho counted from the
    sequence's own start (alpha) or end (beta)"""
    e, m = np.asarray(e), np.asarray(m)
    ld = ld_passes(e, m, pi, A, lengths) if ld is None else ld
    parts = [R.recurrence_bounds(e[lo:hi], m[lo:hi], pi, A, R_, ld=p) for (lo, hi), p in zip(spans(lengths), ld)]
    out = {k: np.concatenate([p[k] for p in parts]) for k in ("alpha", "beta", "ll", "b_alpha", "b_beta", "b_ll", "rho_a", "rho_b")}
    los = [lo for lo, _ in spans(lengths)]
    out["status_a"] = _merge([_shift(p["status_a"], lo) for p, lo in zip(parts, los)])
    out["status_b"] = _merge([_shift(p["status_b"], lo) for p, lo in zip(parts, los)])
    return out


def posterior_bounds(alpha, beta, e, A, rho_a, rho_b, lengths):
    """long double references of the stacked posterior from the long double alpha and beta, and the docstring's bounds"""
    N, K = np.asarray(alpha).shape
    S = len(lengths)
    with np.errstate(all="ignore"):
        gamma, Xi, A_new, pi_new, _ = posterior(alpha, beta, e, A, lengths, dtype=LD)
    f = lambda v: np.asarray(v).astype(np.float64)  # noqa: E731
    rg = 2 * (rho_a + rho_b) + (K + 3) * U
    pair = ~ends(lengths)[:N - 1]
    rx = 2 * float(((rho_a[:-1] + rho_b[1:])[pair]).max() if pair.any() else 0.0) + (K * K + N + 7) * U
    rp = float(max(rg[lo] for lo, _ in spans(lengths))) + (S + 1) * U
    return {"gamma": f(gamma), "xi": f(Xi), "A_new": f(A_new), "pi_new": f(pi_new),
            "b_gamma": f(gamma) * rg[:, None] + ROUND(f(gamma)) + SUBNORMAL, "b_xi": f(Xi) * rx + ROUND(f(Xi)) + SUBNORMAL,
            "b_A_new": f(A_new) * (2 * rx + (K + 3) * U) + ROUND(f(A_new)) + SUBNORMAL,
            "b_pi_new": f(pi_new) * rp + ROUND(f(pi_new)) + SUBNORMAL,
            "b_gamma_sum": 2 * K * U, "b_xi_sum": (N - S) * (K * K + N + 3) * U}


# ---- the fit ---------------------------------------------------------------------------------------------------------------------

def initial_transitions(labels, K, lengths, defect=None):
    """_hmm_ref.initial_transitions without the pairs across a boundary.  defect: "initial_A_counts_boundary" """
    labels = np.asarray(labels)
    keep = ~ends(lengths)[:-1] if defect != "initial_A_counts_boundary" else np.ones(len(labels) - 1, dtype=bool)
    n = np.zeros((K, K))
    np.add.at(n, (labels[:-1][keep], labels[1:][keep]), 1)
    return (n + 1) / (n.sum(axis=1, keepdims=True) + K)


def estep(X, pi, A, mu, s, lengths, defect=None, dtype=np.float64, R_=None):
    lb, m, e = R.emit(X, mu, s, dtype)
    alpha, ll, sa = forward(e, m, pi, A, lengths, defect, dtype, R_)
    beta, sb = backward(e, A, lengths, defect, dtype, R_)
    gamma, Xi, A_new, pi_new, sp = posterior(alpha, beta, e, A, lengths, defect, dtype)
    return {"lb": lb, "ll": ll, "gamma": gamma, "A_new": A_new, "pi_new": pi_new, "bad": sa[0] + sb[0] + sp[0]}


def fit(X, labels, K, lengths, max_iter=100, tol=1e-3, reg_covar=1e-6, defect=None, dtype=np.float64, R_=None):
    """_hmm_ref.fit over several sequences (the same start but initial_transitions, the same stopping rule on all N rows) ->
    its dict, with path_scores [S] and path_score their sum with s ascending.  defects: all of DEFECTS"""
    X = np.asarray(X)
    N, Ld = X.shape
    labels = np.asarray(labels)
    mu, var, s = R._mstep(X, G.one_hot(labels, K).astype(dtype), reg_covar, dtype)
    A = initial_transitions(labels, K, lengths, defect).astype(dtype)
    pi = np.full(K, 1 / dtype(K), dtype=dtype)
    prev, history, why = -np.inf, [], "max_iter"
    for it in range(1, max_iter + 1):
        E = estep(X, pi, A, mu, s, lengths, defect, dtype, R_)
        A, pi = E["A_new"], E["pi_new"]
        mu, var, s = R._mstep(X, E["gamma"], reg_covar, dtype)
        now = R._mean(E["ll"], dtype)
        history.append(now)
        if E["bad"]:
            why = "degenerate"
            break
        if abs(now - prev) < tol:
            why = "converged"
            break
        prev = now
    E = estep(X, pi, A, mu, s, lengths, defect, dtype, R_)
    f = lambda v: np.asarray(v).astype(np.float64)  # noqa: E731
    path, scores, _ = viterbi(f(E["lb"]), R.log0(f(pi)), R.log0(f(A)), lengths, defect)
    score = R._mean(E["ll"], dtype)
    bic, aic = R.criteria(score, N, K, Ld)
    hist = np.array(history, dtype=np.float64)
    return {"pi": f(pi), "A": f(A), "means": f(mu), "covars": f(var), "prec": f(s), "n_iter": it, "converged": why == "converged",
            "why": why, "log_likelihood": float(hist[-1]), "log_likelihoods": hist, "gamma": f(E["gamma"]), "path": path,
            "path_scores": scores, "path_score": sum_ascending(scores), "score": score, "bic": bic, "aic": aic,
            "ll": f(E["ll"]), "changes": np.abs(np.diff(np.concatenate([[-np.inf], hist])))}


# ---- cases -----------------------------------------------------------------------------------------------------------------------

def chain(name, K, seed=3, kind="dense"):
    """the recursion inputs of a length list of LENGTHS -> (lengths, e, m, pi, A)"""
    lengths = LENGTHS[name]
    return (lengths,) + R.random_chain(int(np.sum(lengths)), K, seed, kind)


def cut_chains(lengths, K=4, Ld=3, stay=0.95, sd=0.35, seed=3, spread=1.5):
    """independent planted sticky chains with the same state means, one per sequence, stacked -> (X f32 [N, L], the states)"""
    r = np.random.RandomState(seed)
    mu = spread * r.rand(K, Ld)
    z = np.zeros(int(np.sum(lengths)), dtype=np.int64)
    for lo, hi in spans(lengths):
        z[lo] = r.randint(K)
        for t in range(lo + 1, hi):
            z[t] = z[t - 1] if r.rand() < stay else (z[t - 1] + 1 + r.randint(K - 1)) % K
    return (mu[z] + sd * r.randn(len(z), Ld)).astype(np.float32), z


# the fits of the GPU test: planted chains of 600 rows cut into (300, 1, 299) and into 20 equal pieces
FITS = {"uneven": (300, 1, 299), "twenty": (30,) * 20}


@functools.lru_cache(maxsize=None)
def planted(name):
    """-> (X, states, lengths, the k-means start, the f64 fit, the long double fit, the gates: their differences)"""
    lengths = FITS[name]
    X, z = cut_chains(lengths)
    start = R.kmeans_labels(X, 4)
    f64, ld = fit(X, start, 4, lengths), fit(X, start, 4, lengths, dtype=LD)
    return X, z, lengths, start, f64, ld, R.differences(f64, ld)


# three videos of one task for the held-out labelling: separation chosen so that the restatement alone labels the third
VIDEOS = dict(lengths=(400, 350, 300), K=4, Ld=3, stay=0.95, sd=0.30, seed=11, spread=2.0)


@functools.lru_cache(maxsize=None)
def videos():
    """-> (X, states, lengths, the f64 fit on the first two videos from their k-means start, the restatement's Viterbi path of
    the third under that fit, its ARI against the third's states)"""
    v = dict(VIDEOS)
    lengths = v.pop("lengths")
    K = v.pop("K")
    X, z = cut_chains(lengths, K=K, **v)
    n = lengths[0] + lengths[1]
    start = R.kmeans_labels(X[:n], K)
    f = fit(X[:n], start, K, lengths[:2])
    lb = R.emit(X[n:], f["means"], f["prec"])[0]
    path = R.viterbi(lb, R.log0(f["pi"]), R.log0(f["A"]))[0]
    return X, z, lengths, f, path, R.ari(z[n:], path)


# ---- Bernoulli emissions (bernoulli.bhmm with lengths) -------------------------------------------------------------------------

def bhmm_fit(X, labels, K, lengths, max_iter=100, tol=1e-3, prior=1.0, dtype=np.float64, R_=None):
    """_bernoulli_ref.bhmm_fit over several sequences: its emissions and M-step, this module's recursions, posterior, start and
    Viterbi"""
    import _bernoulli_ref as Bn
    X = np.asarray(X)
    labels = np.asarray(labels)
    M = Bn.mstep(X, G.one_hot(labels, K).astype(dtype), prior, dtype)
    A = initial_transitions(labels, K, lengths).astype(dtype)
    pi = np.full(K, 1 / dtype(K), dtype=dtype)

    def E_(pi, A, M):
        lb, m, e = Bn.emit(X, M["logt"], M["logf"], dtype)
        alpha, ll, sa = forward(e, m, pi, A, lengths, None, dtype, R_)
        beta, sb = backward(e, A, lengths, None, dtype, R_)
        gamma, _, A_new, pi_new, sp = posterior(alpha, beta, e, A, lengths, None, dtype)
        return {"lb": lb, "ll": ll, "gamma": gamma, "A_new": A_new, "pi_new": pi_new, "bad": sa[0] + sb[0] + sp[0]}

    prev, history, why = -np.inf, [], "max_iter"
    for it in range(1, max_iter + 1):
        E = E_(pi, A, M)
        A, pi = E["A_new"], E["pi_new"]
        M = Bn.mstep(X, E["gamma"], prior, dtype)
        now = Bn._mean(E["ll"], dtype)
        history.append(now)
        if E["bad"]:
            why = "degenerate"
            break
        if abs(now - prev) < tol:
            why = "converged"
            break
        prev = now
    E = E_(pi, A, M)
    f = lambda v: np.asarray(v).astype(np.float64)  # noqa: E731
    path, scores, _ = viterbi(f(E["lb"]), R.log0(f(pi)), R.log0(f(A)), lengths)
    hist = np.array(history, dtype=np.float64)
    return {"pi": f(pi), "A": f(A), "probs": f(M["theta"]), "n_iter": it, "converged": why == "converged", "why": why,
            "log_likelihoods": hist, "gamma": f(E["gamma"]), "path": path, "path_scores": scores, "ll": f(E["ll"]),
            "score": Bn._mean(E["ll"], dtype), "changes": np.abs(np.diff(np.concatenate([[-np.inf], hist])))}


# planted codes of L bits (N, L, K, flip, stay, seed of _bernoulli_ref.planted_chain) cut into CODE_LENGTHS
CODES = {32: (300, 32, 4, 0.2, 0.9, 1), 50: (300, 50, 4, 0.25, 0.9, 2), 128: (300, 128, 4, 0.35, 0.9, 3)}
CODE_LENGTHS = (100, 1, 120, 79)


@functools.lru_cache(maxsize=None)
def planted_codes(Ld):
    """-> (X, states, the k-means start, the f64 fit, the long double fit, the gates) of the codes of Ld bits"""
    import _bernoulli_ref as Bn
    X, s, _ = Bn.planted_chain(*CODES[Ld])
    start = R.kmeans_labels(X, CODES[Ld][2])
    f64, ld = bhmm_fit(X, start, CODES[Ld][2], CODE_LENGTHS), bhmm_fit(X, start, CODES[Ld][2], CODE_LENGTHS, dtype=LD)
    return X, s, start, f64, ld, Bn.differences(f64, ld, Bn.BHMM_QUANTITIES, "path")
