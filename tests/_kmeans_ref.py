"""Reference and bounds for the k-means and symbol tests (csrc/kmeans.hip, symbols.py).

An f64 numpy restatement of scikit-learn 1.7.2's KMeans(n_init=1, algorithm="lloyd") with k-means++ seeding, of the six
agreement scores of sklearn.metrics computed from the integer contingency table, and of the Davies-Bouldin and
Calinski-Harabasz indices, written independently of the package; tests/golden/kmeans.npz (tools/make_kmeans_golden.py) pins
it to scikit-learn.  Functions take a `defect` name: the restatement with one named mistake, which
tests/test_kmeans_cpu.py uses to show that the check meant to catch that mistake does.

Distances are direct differences, d2_ik = sum_l (x_il - c_kl)^2 with l ascending, and a tie goes to the lower centre;
scikit-learn takes |x|^2 - 2 x.c + |c|^2 on centred data.  Labels, init indices and n_iter are integers and must be equal:
the fixture's smallest gap between a row's nearest and second-nearest centre is 3.2e-4, far above either form's rounding.
An empty cluster keeps its centre (scikit-learn moves it to a far row); no fixture case has one.

Bounds.  u = 2^-53 is the f64 unit roundoff; every count is first order, each rounding taken at its full half ulp with the
same sign.  Nothing was chosen by looking at device output.
  d2      per coordinate the difference x - c rounds once (c is any f64 value), the square once and the addition once; all
          terms are non-negative: |got - ref| <= (L + 3) u d2 against a long double reference (d2_bound).
  labels  equal wherever the runner-up's d2 exceeds the winner's by more than twice that bound (decided).
  centre  sum_{i in k} x_il in any order is off by at most n_k u sum |x_il|; divided by n_k that is u sum_{i in k} |x_il|,
          and the division rounds once: one more u |c_kl| (centre_bound).
  within  n_k non-negative terms added in any order: n_k u within_k (n_k - 1 rounded up).  Where the d2 are the device's
          own and not given, each carries d2's bound: (L + 3) u within_k more.
  spread  the same n_k u spread_k: with d2 given, the reference takes the same f64 square roots and an IEEE root on the
          device adds nothing.  With the device's own d2, sqrt halves their relative error and the root of a different
          argument rounds on its own: ((L + 3) / 2 + 1) u spread_k more (sum_bounds).
  potential   min(closest, d2) keeps d2's bound; N terms in a tree: (N + L + 3) u pot (generous: a tree's depth is log2 N).
Agreement scores come from integers and equal scikit-learn's to 1e-15; centres, inertia (relative) and the two indices are
held to 1e-12 as the silhouette is (scikit-learn centres X and expands the square, the device does neither).
"""
import numpy as np

from _projection_ref import TINY, U, rejects, within  # noqa: F401

LD = np.longdouble
KM_CHUNK = 4096                         # f64 values of centres per LDS chunk of rbvae_kmeans_assign
WHY = {1: "strict", 2: "tol", 3: "max_iter"}


def chunk_centres(L):
    return KM_CHUNK // ((L + 7) // 8 * 8)


def soft_rows(N, Ld, seed):
    r = np.random.RandomState(seed)
    return (1.0 / (1.0 + np.exp(-2.0 * r.randn(N, Ld)))).astype(np.float32)


# ---- distances and assignment --------------------------------------------------------------------------------------------

def d2_to(X, C, dtype=np.float64):
    """[N, K]: sum_l (x_il - c_kl)^2, l ascending, every operation rounded in `dtype`"""
    X, C = np.asarray(X).astype(dtype), np.asarray(C).astype(dtype)
    D = np.zeros((len(X), len(C)), dtype=dtype)
    for l in range(X.shape[1]):
        df = X[:, None, l] - C[None, :, l]
        D += df * df
    return D


def d2_bound(L, d2):
    return (L + 3) * U * np.asarray(d2, dtype=np.float64) + TINY


def assign(X, C, defect=None, D=None):
    """-> (label [N] int32, d2 [N] f64): the smallest (d2, k).  defect "tie_high": ties go to the higher centre"""
    D = d2_to(X, C) if D is None else D
    K = D.shape[1]
    lab = (K - 1 - np.argmin(D[:, ::-1], axis=1)) if defect == "tie_high" else np.argmin(D, axis=1)
    return lab.astype(np.int32), D[np.arange(len(D)), lab]


def decided(D, L):
    """[N] bool from long double distances: the runner-up is more than twice d2's bound above the winner"""
    D = np.asarray(D, dtype=np.float64)
    if D.shape[1] == 1:
        return np.ones(len(D), dtype=bool)
    s = np.sort(D, axis=1)
    return s[:, 1] - s[:, 0] > 2.0 * d2_bound(L, s[:, 0])


def update(X, lab, C_old, d2=None, defect=None):
    """-> (centres [K, L], count [K], shift2 [K], within [K], spread [K]) with sums in long double.  An empty cluster keeps
    its centre; defect "empty_centre_zeroed": it becomes 0."""
    X64 = np.asarray(X).astype(np.float64)
    K = len(C_old)
    C = np.array(C_old, dtype=np.float64)
    count = np.bincount(lab[(lab >= 0) & (lab < K)], minlength=K).astype(np.int32)
    wi, sp = np.zeros(K), np.zeros(K)
    for k in range(K):
        rows = lab == k
        if count[k]:
            C[k] = (X64[rows].astype(LD).sum(0) / count[k]).astype(np.float64)
            if d2 is not None:
                wi[k] = float(d2[rows].astype(LD).sum())
                sp[k] = float(np.sqrt(d2[rows]).astype(LD).sum())
        elif defect == "empty_centre_zeroed":
            C[k] = 0.0
    return C, count, ((C - C_old) ** 2).sum(1), wi, sp


def centre_bound(X, lab, C):
    """[K, L]: u sum_{i in k} |x_il| (the sum's n_k roundings, divided by n_k) + u |c_kl| (the division)"""
    A = np.abs(np.asarray(X).astype(np.float64))
    S = np.stack([A[lab == k].sum(0) for k in range(len(C))])
    return U * S + U * np.abs(C) + TINY


def tolerance(X, tol):
    return float(np.mean(np.var(np.asarray(X).astype(np.float64), axis=0)) * tol)


def lloyd(X, C0, max_iter=300, tol=1e-4, defect=None):
    """-> dict(labels, centers, inertia, n_iter, converged, counts): scikit-learn's _kmeans_single_lloyd.
    defects: "tie_high", "empty_centre_zeroed", "shift_not_squared" (the tol rule sums |shift|), "no_final_assign_after_tol"
    (the labels of the last iteration are kept), "n_iter_off_by_one"."""
    X64 = np.asarray(X).astype(np.float64)
    C = np.array(C0, dtype=np.float64)
    tol_abs = tolerance(X, tol)
    old = np.full(len(X64), -1, dtype=np.int32)
    why = 3
    for it in range(max_iter):
        lab, _ = assign(X64, C, defect)
        C, _, shift2, _, _ = update(X64, lab, C, defect=defect)
        if np.array_equal(lab, old):
            why = 1
            break
        tot = np.sqrt(shift2).sum() if defect == "shift_not_squared" else shift2.sum()
        if tot <= tol_abs:
            why = 2
            break
        old = lab
    if why != 1 and defect != "no_final_assign_after_tol":
        lab, _ = assign(X64, C, defect)
    d2 = d2_to(X64, C)[np.arange(len(X64)), lab]
    inertia = float(np.stack([d2[lab == k].sum() for k in range(len(C))]).sum())
    return {"labels": lab, "centers": C, "inertia": inertia, "n_iter": it + (0 if defect == "n_iter_off_by_one" else 1),
            "converged": WHY[why], "counts": np.bincount(lab, minlength=len(C))}


def kmeans_pp(X, K, seed, defect=None):
    """scikit-learn's _kmeans_plusplus with unit weights -> indices [K].  defects: "pp_first_trial_wins" (the first
    candidate is taken, not the one with the lowest potential), "pp_unclipped_index" (searchsorted's N is kept and wraps
    to row 0)."""
    X64 = np.asarray(X).astype(np.float64)
    N = len(X64)
    rs = np.random.RandomState(seed)
    T = 2 + int(np.log(K))
    idx = np.full(K, -1, dtype=np.int64)
    idx[0] = rs.choice(N, p=np.ones(N) / np.ones(N).sum())
    closest = d2_to(X64, X64[idx[:1]])[:, 0]
    pot = closest.sum()
    for c in range(1, K):
        vals = rs.uniform(size=T) * pot
        cand = pp_candidates(closest, vals, defect)
        trial = np.minimum(closest[None, :], d2_to(X64, X64[cand]).T)
        pots = trial.sum(1)
        best = 0 if defect == "pp_first_trial_wins" else int(np.argmin(pots))
        pot, closest, idx[c] = pots[best], trial[best], cand[best]
    return idx


# ---- agreement of two labellings -------------------------------------------------------------------------------------------

def contingency(a, b, A=None, B=None):
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    A, B = int(a.max()) + 1 if A is None else A, int(b.max()) + 1 if B is None else B
    T = np.zeros((A, B), dtype=np.int64)
    np.add.at(T, (a, b), 1)
    return T


def _entropy(n):
    n = n[n > 0].astype(np.float64)
    if n.size == 1:
        return 0.0
    tot = np.sum(n)
    return float(-np.sum((n / tot) * (np.log(n) - np.log(tot))))


def _mutual_information(T):
    T = T[T.sum(1) > 0][:, T.sum(0) > 0]
    pi, pj = T.sum(1), T.sum(0)
    if pi.size == 1 or pj.size == 1:
        return 0.0
    x, y = np.nonzero(T)
    v = T[x, y].astype(np.float64)
    tot = float(T.sum())
    outer = pi[x].astype(np.int64) * pj[y].astype(np.int64)
    log_outer = -np.log(outer) + np.log(float(pi.sum())) + np.log(float(pj.sum()))
    mi = v / tot * (np.log(v) - np.log(tot)) + v / tot * log_outer
    mi = np.where(np.abs(mi) < np.finfo(np.float64).eps, 0.0, mi)
    return float(np.clip(mi.sum(), 0.0, None))


def agreement(T, defect=None):
    """the six scores of sklearn.metrics from the contingency table T [A, B] (rows: the true labels).  defects:
    "ari_unadjusted" (the plain Rand index), "nmi_geometric" (sqrt(H_a H_b) as the normaliser)"""
    T = np.asarray(T, dtype=np.int64)
    n = int(T.sum())
    ra, rb = [int(v) for v in T.sum(1)], [int(v) for v in T.sum(0)]
    sq = sum(int(v) ** 2 for v in T.reshape(-1))
    tp, fp, fn = sq - n, sum(v * v for v in rb) - sq, sum(v * v for v in ra) - sq
    tn = n * n - fp - fn - sq
    if defect == "ari_unadjusted":
        ari = (tp + tn) / (tp + tn + fp + fn)
    else:
        ari = 1.0 if fn == 0 and fp == 0 else 2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))
    ha, hb = _entropy(T.sum(1)), _entropy(T.sum(0))
    mi = _mutual_information(T)
    hom = mi / ha if ha else 1.0
    com = mi / hb if hb else 1.0
    v = 0.0 if hom + com == 0.0 else 2.0 * hom * com / (hom + com)
    na, nb = int((T.sum(1) > 0).sum()), int((T.sum(0) > 0).sum())
    if na == nb == 1 or na == nb == 0:
        nmi = 1.0
    elif mi == 0:
        nmi = 0.0
    else:
        nmi = float(mi / (np.sqrt(ha * hb) if defect == "nmi_geometric" else np.mean([ha, hb])))
    pk, qk = sum(v_ * v_ for v_ in rb) - n, sum(v_ * v_ for v_ in ra) - n
    fmi = float(np.sqrt(tp / pk) * np.sqrt(tp / qk)) if tp != 0 else 0.0
    return {"ari": float(ari), "nmi": nmi, "homogeneity": float(hom), "completeness": float(com), "v_measure": float(v),
            "fowlkes_mallows": fmi}


SCORES = ("ari", "nmi", "homogeneity", "completeness", "v_measure", "fowlkes_mallows")


# ---- cluster indices -------------------------------------------------------------------------------------------------------

def _dense_labels(lab):
    return np.unique(np.asarray(lab), return_inverse=True)[1].reshape(-1)


def cluster_sums(X, lab):
    """-> (centroids, counts, within, spread) of the non-empty labels in ascending order, distances to the own centroid"""
    X64 = np.asarray(X).astype(np.float64)
    lab = _dense_labels(lab)
    K = int(lab.max()) + 1
    C, n, _, _, _ = update(X64, lab, np.zeros((K, X64.shape[1])))
    d2 = d2_to(X64, C)[np.arange(len(X64)), lab]
    _, _, _, wi, sp = update(X64, lab, C, d2)
    return C, n, wi, sp


def davies_bouldin(X, lab, defect=None):
    """defect "db_squared_spread": a cluster's spread is its mean squared distance"""
    C, n, wi, sp = cluster_sums(X, lab)
    intra = (wi if defect == "db_squared_spread" else sp) / n
    cd = np.sqrt(d2_to(C, C))
    if np.allclose(intra, 0) or np.allclose(cd, 0):
        return 0.0
    cd[cd == 0] = np.inf
    return float(np.mean(np.max((intra[:, None] + intra[None, :]) / cd, axis=1)))


def calinski_harabasz(X, lab, defect=None):
    """defect "ch_dof_swapped": (K - 1) and (N - K) change places"""
    X64 = np.asarray(X).astype(np.float64)
    C, n, wi, _ = cluster_sums(X, lab)
    N, K = len(X64), len(C)
    extra = float((n * ((C - X64.mean(0)) ** 2).sum(1)).sum())
    intra = float(wi.sum())
    if intra == 0.0:
        return 1.0
    if defect == "ch_dof_swapped":
        return extra * (K - 1.0) / (intra * (N - K))
    return extra * (N - K) / (intra * (K - 1.0))


# ---- the synthetic cases of the kernel tests ---------------------------------------------------------------------------------

ASSIGN_CASES = [(1, 1, 1), (65, 3, 4), (257, 50, 17), (300, 128, 33), (300, 128, 256), (16385, 2, 3)]


def assign_case(N, Ld, K):
    """X f32 [N, L] and centres f64 [K, L] that are no f32 values (rows of X moved by f64 noise): x - c rounds"""
    r = np.random.RandomState(1000 * N + 10 * Ld + K)
    X = soft_rows(N, Ld, N + Ld + K)
    C = X[r.randint(0, N, K)].astype(np.float64) + 0.05 * r.randn(K, Ld)
    return X, C


def tie_case():
    """small-integer coordinates and duplicated centres: exact ties, all of which go to the lower centre"""
    r = np.random.RandomState(7)
    X = r.randint(0, 3, (300, 5)).astype(np.float32)
    C = r.randint(0, 3, (6, 5)).astype(np.float64)
    return X, np.concatenate([C, C[::-1], C[:2] + 0.5])


def update_labels(N, K, kind, seed=0):
    """"random"; "empty": every third cluster (and the last) holds no row; "one": cluster K // 2 holds every row;
    "striped": row i belongs to cluster i mod K, so every cluster is split across all row blocks"""
    r = np.random.RandomState(seed + N + K)
    if kind == "one":
        return np.full(N, K // 2, dtype=np.int32)
    if kind == "striped":
        return (np.arange(N) % K).astype(np.int32)
    lab = r.randint(0, K, N).astype(np.int32)
    if kind == "empty":
        keep = [k for k in range(K) if k % 3 != 1 and k != K - 1] or [0]
        lab = np.asarray(keep, dtype=np.int32)[r.randint(0, len(keep), N)]
    return lab


def sum_bounds(count, within_, spread_, Ld=None):
    """(bound of within, bound of spread): n_k u times the value.  Ld: the d2 are the device's own and carry d2_bound, the
    reference's are long double: (L + 3) u more for within, (L + 3) / 2 u + u (the root of another argument rounds) for
    spread"""
    n = np.asarray(count, dtype=np.float64)
    extra_w, extra_s = (0.0, 0.0) if Ld is None else (Ld + 3.0, (Ld + 3.0) / 2.0 + 1.0)
    return (n + extra_w) * U * within_ + TINY, (n + extra_s) * U * spread_ + TINY


def pp_candidates(closest, vals, defect=None):
    """searchsorted(cumsum(closest), vals) clipped to N - 1; defect "pp_unclipped_index": N wraps to row 0"""
    N = len(closest)
    cand = np.searchsorted(np.cumsum(closest), vals)
    return cand % N if defect == "pp_unclipped_index" else np.minimum(cand, N - 1)
