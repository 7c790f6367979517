"""Reference and bounds for the segmentation tests (csrc/segment.hip, segments.py).

The definition of include/rbvae_hip.h restated in numpy, written independently of the package, once in f64 with the
device's operation order (the device must equal it bit for bit: every operation is a basic IEEE one) and once in long
double (what both are held to), and a brute-force enumeration of all segmentations for tiny N.
  prefix      r_i = sum_l x_il x_il (l ascending), then rows in blocks of SEG_SCAN = 256: off + np.cumsum(block, axis=0),
              off <- the block's last row
  candidates  d2 = sum_l (P[t]_l - P[s]_l)^2 (l ascending); cost = (Q[t] - Q[s]) - d2 / (t - s); cand = prev[s] + cost for
              0 <= s <= t - m with prev[s] finite
  layer       the smallest candidate in the order (value, s): np.argmin takes the first of equal values
  table, trace    D_1 = layer([0, inf, ...]), D_k = layer(D_{k - 1}); t <- arg[j][t] from t = N
Large cases are evaluated in blocks of ROWS ends.

Bounds.  u = 2^-53 is the f64 unit roundoff and u_ld long double's; every rounding is taken at its full half ulp with
the same sign.  Nothing was chosen by looking at device output.  A(t, l) = sum_{i < t} |x_il|.
  P       P[t]_l is reached from its terms through at most depth(t) = min(t, 256) + (t - 1) // 256 + 1 additions (up to
          255 inside the block, one per earlier block along the offsets, the last one), each off by at most u times a
          partial sum of absolute values: depth(t) u A(t, l).  The long double reference adds its terms one by one:
          t u_ld A(t, l) more (p_bound).
  Q       the same over r_i >= 0, each of which carries L - 1 roundings of its own (the products of two f32 values are
          exact): (depth(t) + L) u Q[t] + t u_ld Q[t] (q_bound).
  exact   where every x_il is an integer and sum x_il^2 < 2^53 (hard codes) every sum, difference and square is an exact
          integer in either format: P, Q and d2 carry no error at all.
  d2      per coordinate the difference df of two P values carries their bounds e = pb[t] + pb[s] and rounds once, the
          square and the addition round once each: sum_l (2 |df_l| e_l + e_l^2) + (L + 3) u d2; 0 on exact data.
  cost    qb[t] + qb[s], the subtraction's u |Q[t] - Q[s]| (0 on exact data), d2's bound over n = t - s, the division's
          u d2 / n and the last subtraction's u |cost|.
  cand    cost's bound and the addition's u |cand|; prev is given and carries nothing.
  The long double reference's own roundings after P and Q are 2^-11 of these term by term: every bound is multiplied by
  LD_SLOP = 1 + 2^-10.
  out     with s' the minimiser in one format and s* in the other, out is between min - b(s') and min + b(s*): the row's
          bound is the largest candidate bound over its candidates, and u |out| more for rounding the long double minimum
          to f64.
  arg     decided where the runner-up in long double is more than twice the row's bound above the minimum; on an
          undecided row the long double candidate at the device's arg is within twice the bound of the minimum.
Undecided rows may be at most UNDECIDED_CAP of a case: 1 % on soft data, 10 % on codes, where integer costs tie exactly.

Measured on the CPU (tests/test_segment_cpu.py prints them): the f64 restatement's candidates' minima are within 0.04 of
their bound on the soft cases and 0.77 on the codes; no soft row is undecided; the code cases have 5 of 128, 1 of 508 and
2 of 1023 rows undecided from D_2 (exact ties of integer costs) and none from the random prev.  On soft data the derived
bound sits about 25 times above the observed error (depth(t) roundings of one sign do not happen), so a subtly wrong
kernel would be caught by the GPU tests' bit-equality with the f64 restatement, not by the bounds; the bounds are the gate
that holds if an operation ever legitimately differs.
"""
import functools
import itertools

import numpy as np

from _projection_ref import TINY, U, within  # noqa: F401

LD = np.longdouble
ULD = float(np.finfo(LD).eps) / 2.0
LD_SLOP = 1.0 + 2.0 ** -10
SEG_SCAN = 256
ROWS = 256
UNDECIDED_CAP = {"soft": 0.01, "code": 0.10}

#             kind    N     L    S  m
LAYER_CASES = [("soft", 63, 1, 3, 1), ("soft", 64, 3, 3, 1), ("soft", 65, 50, 4, 1), ("soft", 130, 128, 5, 3),
               ("soft", 513, 32, 9, 1), ("soft", 1025, 2, 5, 1), ("code", 130, 50, 5, 1), ("code", 513, 50, 9, 2),
               ("code", 1025, 8, 5, 1)]
LARGE_CASE = ("soft", 4097, 2, 5, 1)                # f64 only: many tiles and runs of start tiles
PREFIX_SHAPES = [(2, 1), (255, 3), (256, 50), (257, 128), (1025, 2)]
BRUTE_CASES = [(9, 2, 4, 1), (10, 3, 3, 2), (8, 1, 8, 1)]              # N, L, K, m
PLANTED_CASES = [("soft", 65, 3, 4, 1), ("soft", 130, 50, 5, 1), ("soft", 257, 128, 6, 3), ("soft", 1000, 32, 17, 1),
                 ("code", 130, 50, 5, 1), ("code", 1000, 50, 17, 2)]


def data(kind, N, L, S, seed):
    r = np.random.RandomState(seed)
    cuts = np.sort(r.choice(np.arange(1, N), S - 1, replace=False))
    lab = np.searchsorted(cuts, np.arange(N), side="right")
    if kind == "soft":
        mu = r.rand(S, L); X = np.clip(mu[lab] + 0.05 * r.randn(N, L), 0, 1).astype(np.float32)     # noqa: E702
    else:
        mu = r.rand(S, L) < 0.5; flip = r.rand(N, L) < 0.03; X = (mu[lab] ^ flip).astype(np.float32)   # noqa: E702
    return X, cuts


@functools.lru_cache(maxsize=None)
def case(kind, N, L, S):
    X, cuts = data(kind, N, L, S, N + L)
    X.setflags(write=False)
    return X, cuts


# ---- the restatement ------------------------------------------------------------------------------------------------------

def prefix(X, dtype=np.float64):
    """-> (P [N + 1, L], Q [N + 1]) in `dtype`, in the device's order"""
    X = np.asarray(X).astype(dtype)
    N, L = X.shape
    r = np.zeros(N, dtype=dtype)
    for l in range(L):
        r += X[:, l] * X[:, l]
    P, Q = np.zeros((N + 1, L), dtype=dtype), np.zeros(N + 1, dtype=dtype)
    offP, offQ = np.zeros(L, dtype=dtype), dtype(0.0)
    for b in range(0, N, SEG_SCAN):
        cP = offP + np.cumsum(X[b:b + SEG_SCAN], axis=0)
        cQ = offQ + np.cumsum(r[b:b + SEG_SCAN])
        P[b + 1:b + 1 + len(cP)], Q[b + 1:b + 1 + len(cQ)] = cP, cQ
        offP, offQ = cP[-1], cQ[-1]
    return P, Q


def candidates(P, Q, prev, m, t, pb=None, qb=None, exact=False):
    """For the ends t (a vector) -> (cand [T, C] with +inf where there is no candidate, valid [T, C], and with pb and qb
    given the candidates' bounds [T, C], else None) over the starts s < C = max(t) - m + 1, beyond which no end of t has
    a candidate.  Everything in P's dtype."""
    dtype = P.dtype.type
    L = P.shape[1]
    N1 = max(int(t.max()) - m + 1, 1)
    s = np.arange(N1)
    prev = np.asarray(prev).astype(dtype)[:N1]
    valid = (s[None, :] <= t[:, None] - m) & np.isfinite(prev)[None, :]
    n = np.where(valid, t[:, None] - s[None, :], 1).astype(dtype)
    d2 = np.zeros((len(t), N1), dtype=dtype)
    e2 = np.zeros((len(t), N1)) if pb is not None and not exact else None
    for l in range(L):
        df = P[t, l][:, None] - P[None, :N1, l]
        d2 += df * df
        if e2 is not None:
            e = pb[t, l][:, None] + pb[None, :N1, l]
            e2 += 2.0 * np.abs(df).astype(np.float64) * e + e * e
    dq = Q[t][:, None] - Q[None, :N1]
    cost = dq - d2 / n
    cand = np.where(valid, np.where(np.isfinite(prev), prev, dtype(0.0))[None, :] + cost, dtype(np.inf))
    bound = None
    if pb is not None:
        f = lambda a: np.abs(a).astype(np.float64)         # noqa: E731
        if exact:
            bound = U * f(d2 / n) + U * f(cost)
        else:
            bound = (qb[t][:, None] + qb[None, :N1] + U * f(dq) + (e2 + (L + 3) * U * f(d2)) / f(n) + U * f(d2 / n)
                     + U * f(cost))
        bound = np.where(valid, (bound + U * f(np.where(valid, cand, 0.0))) * LD_SLOP + TINY, 0.0)
    return cand, valid, bound


def layer(P, Q, prev, m=1):
    """-> (out [N + 1], arg int32 [N + 1]) in P's dtype: the smallest candidate in the order (value, s), (+inf, -1) where
    there is none"""
    N1 = len(Q)
    out, arg = np.full(N1, np.inf, dtype=P.dtype), np.full(N1, -1, dtype=np.int32)
    for t0 in range(0, N1, ROWS):
        t = np.arange(t0, min(N1, t0 + ROWS))
        cand, valid, _ = candidates(P, Q, prev, m, t)
        a = np.argmin(cand, axis=1)                         # the first of equal values: the lower s
        some = valid.any(axis=1)
        out[t] = np.where(some, cand[np.arange(len(t)), a], np.inf)
        arg[t] = np.where(some, a, -1)
    return out, arg


def first_prev(N, dtype=np.float64):
    prev = np.full(N + 1, np.inf, dtype=dtype)
    prev[0] = 0.0
    return prev


def table(X, K, m=1, dtype=np.float64):
    """-> (cost [K, N + 1], arg int32 [K, N + 1], P, Q)"""
    P, Q = prefix(X, dtype)
    N = len(X)
    cost, arg = np.empty((K, N + 1), dtype=dtype), np.empty((K, N + 1), dtype=np.int32)
    prev = first_prev(N, dtype)
    for k in range(K):
        cost[k], arg[k] = layer(P, Q, prev, m)
        prev = cost[k]
    return cost, arg, P, Q


def trace(cost, arg):
    """-> cuts int32 [K, K]: row k - 1 = the k - 1 interior boundaries ascending, padded with -1"""
    K, N = cost.shape[0], cost.shape[1] - 1
    cuts = np.full((K, K), -1, dtype=np.int32)
    for k in range(1, K + 1):
        if not np.isfinite(cost[k - 1, N]):
            continue
        t = N
        for j in range(k, 1, -1):
            t = int(arg[j - 1, t])
            cuts[k - 1, j - 2] = t
    return cuts


def labels_of(cuts, N):
    return np.searchsorted(np.asarray(cuts), np.arange(N), side="right").astype(np.int32)


def brute(X, K, m=1):
    """All segmentations of the rows into k <= K segments of at least m rows, each segment's cost sum |x - mean|^2 taken
    directly in f64 -> (costs [K] with +inf where there is none, cuts: a list of K tuples or None)"""
    X = np.asarray(X).astype(np.float64)
    N = len(X)
    seg = {(s, t): float(((X[s:t] - X[s:t].mean(axis=0)) ** 2).sum()) for s in range(N) for t in range(s + m, N + 1)}
    costs, cuts = np.full(K, np.inf), [None] * K
    for k in range(1, K + 1):
        for c in itertools.combinations(range(1, N), k - 1):
            e = (0,) + c + (N,)
            if any(b - a < m for a, b in zip(e, e[1:])):
                continue
            v = sum(seg[(a, b)] for a, b in zip(e, e[1:]))
            if v < costs[k - 1]:
                costs[k - 1], cuts[k - 1] = v, c
    return costs, cuts


# ---- bounds ---------------------------------------------------------------------------------------------------------------

def is_exact(X):
    X = np.asarray(X).astype(np.float64)
    return bool(np.all(X == np.rint(X)) and (X * X).sum() < 2.0 ** 53)


def depth(N):
    t = np.arange(N + 1)
    return np.where(t > 0, np.minimum(t, SEG_SCAN) + (t - 1) // SEG_SCAN + 1, 0).astype(np.float64)


def p_bound(X):
    """[N + 1, L]: (depth(t) u + t u_ld) A(t, l); 0 on exact data"""
    X = np.asarray(X).astype(np.float64)
    N, L = X.shape
    if is_exact(X):
        return np.full((N + 1, L), TINY)
    A = np.vstack([np.zeros((1, L)), np.cumsum(np.abs(X), axis=0)])
    return ((depth(N) * U + np.arange(N + 1) * ULD)[:, None] * A) * LD_SLOP + TINY


def q_bound(X):
    """[N + 1]: ((depth(t) + L) u + t u_ld) Q[t]; 0 on exact data"""
    X = np.asarray(X).astype(np.float64)
    N, L = X.shape
    if is_exact(X):
        return np.full(N + 1, TINY)
    Qa = np.concatenate([[0.0], np.cumsum((X * X).sum(axis=1))])
    return ((depth(N) + L) * U + np.arange(N + 1) * ULD) * Qa * LD_SLOP + TINY


def table_bound(X, K):
    """What K layers can put between D_k[N] and the exact optimum: each layer adds at most the largest candidate bound
    (taken over all pairs with prev = 0) and u Q[N] for the candidate's own magnitude, which prev = 0 leaves out"""
    Pl, Ql = prefix(X, LD)
    pb, qb, exact, N = p_bound(X), q_bound(X), is_exact(X), len(X)
    b = 0.0
    for t0 in range(1, N + 1, ROWS):
        t = np.arange(t0, min(N + 1, t0 + ROWS))
        b = max(b, float(candidates(Pl, Ql, np.zeros(N + 1), 1, t, pb, qb, exact)[2].max()))
    return K * (b + U * float(Ql[-1]) * LD_SLOP)


def layer_ld(X, prev, m=1):
    """The layer in long double with everything the checks need -> dict(out [N + 1] f64-rounded minimum, arg, bound [N + 1]
    the row's bound, gap [N + 1] the runner-up minus the minimum (+inf with fewer than two candidates), n_cand [N + 1],
    at: a function (t, s) -> the long double candidates at those pairs as f64-rounded differences to the minimum)"""
    Pl, Ql = prefix(X, LD)
    pb, qb, exact = p_bound(X), q_bound(X), is_exact(X)
    N1 = len(Ql)
    out, arg = np.full(N1, np.inf, dtype=LD), np.full(N1, -1, dtype=np.int32)
    bound, gap, n_cand = np.zeros(N1), np.full(N1, np.inf), np.zeros(N1, dtype=np.int64)
    for t0 in range(0, N1, ROWS):
        t = np.arange(t0, min(N1, t0 + ROWS))
        cand, valid, b = candidates(Pl, Ql, prev, m, t, pb, qb, exact)
        a = np.argmin(cand, axis=1)
        some = valid.any(axis=1)
        out[t] = np.where(some, cand[np.arange(len(t)), a], np.inf)
        arg[t] = np.where(some, a, -1)
        bound[t] = b.max(axis=1)
        n_cand[t] = valid.sum(axis=1)
        two = np.partition(cand, 1, axis=1)[:, :2] if cand.shape[1] > 1 else None
        with np.errstate(invalid="ignore"):
            g = (two[:, 1] - two[:, 0]).astype(np.float64)
        gap[t] = np.where(n_cand[t] >= 2, g, np.inf)

    def at(t, s):
        t, s = np.asarray(t), np.asarray(s)
        res = np.empty(len(t), dtype=LD)
        for i in range(len(t)):
            c, _, _ = candidates(Pl, Ql, prev, m, t[i:i + 1])
            res[i] = c[0, s[i]]
        return res

    return {"out": out, "arg": arg, "bound": bound, "gap": gap, "n_cand": n_cand, "at": at, "P": Pl, "Q": Ql}


def check_layer(kind, got_out, got_arg, ref, what):
    """The layer checks of the GPU tests, for any (out, arg) against layer_ld's dict -> (worst |err| / bound, undecided rows)"""
    got_out, got_arg = np.asarray(got_out), np.asarray(got_arg)
    none = ref["n_cand"] == 0
    assert np.all(np.isposinf(got_out[none])) and np.all(got_arg[none] == -1), f"{what}: rows without a candidate"
    some = ~none
    assert np.all(np.isfinite(got_out[some])), f"{what}: a row with candidates is not finite"
    worst = within(got_out[some], ref["out"][some].astype(np.float64), ref["bound"][some] + U * np.abs(got_out[some]), what)
    decided = some & (ref["gap"] > 2.0 * ref["bound"])
    assert np.array_equal(got_arg[decided], ref["arg"][decided]), f"{what}: arg differs on a decided row"
    und = np.nonzero(some & ~decided)[0]
    if und.size:
        off = (ref["at"](und, got_arg[und]) - ref["out"][und]).astype(np.float64)
        assert np.all(off <= 2.0 * ref["bound"][und]), f"{what}: arg on an undecided row is no near-minimum"
    cap = UNDECIDED_CAP[kind]
    assert und.size <= cap * some.sum(), f"{what}: {und.size} of {some.sum()} rows undecided (cap {cap})"
    return worst, int(und.size)


def random_prev(N, scale):
    """random finite values in [0, scale) with 30 % of the entries +inf"""
    r = np.random.RandomState(N)
    prev = r.rand(N + 1) * scale
    prev[r.rand(N + 1) < 0.3] = np.inf
    return prev


@functools.lru_cache(maxsize=None)
def layer_case(kind, N, L, S, m, which):
    """-> (X, P, Q, prev, out, arg) of the f64 restatement, which = "D2" (prev = the restatement's D_2) or "random"
    (random_prev scaled by Q[N])"""
    X, _ = case(kind, N, L, S)
    if which == "D2":
        cost, _, P, Q = table(X, 2, m)
        prev = cost[1].copy()
    else:
        P, Q = prefix(X)
        prev = random_prev(N, float(Q[-1]))
    out, arg = layer(P, Q, prev, m)
    for a in (P, Q, prev, out, arg):
        a.setflags(write=False)
    return X, P, Q, prev, out, arg


@functools.lru_cache(maxsize=None)
def layer_case_ld(kind, N, L, S, m, which):
    X, _, _, prev, _, _ = layer_case(kind, N, L, S, m, which)
    return layer_ld(X, prev, m)
