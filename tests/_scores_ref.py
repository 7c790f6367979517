"""Reference and bounds for the latent-score tests (csrc/scores.hip, scores.py).

An f64 numpy restatement of the neighbour ranks behind trustworthiness / continuity, the per-state distance sums, the
silhouette and the kNN label agreement, written independently of the package; tests/golden/latent_scores.npz
(tools/make_scores_golden.py) pins it to scikit-learn 1.7.2.  Functions take a `defect` name: the restatement with one
named mistake, which tests/test_scores_cpu.py uses to show that the check meant to catch that mistake does.

Ranks are integers: they must be equal wherever they are decided.  d2 = sum_l (x_il - x_jl)^2 is computed as the kernel
computes it (_projection_ref.sqdist: l ascending, each difference exact, each square rounded once), so exact ties are
ties on both sides and the (d2, index) rule settles them; an entry is undecided only where another distance of its row
lies within 1e-12 relative of the neighbour's without being equal to it (decided).

Bound of the Euclidean sums.  u = 2^-53 is the f64 unit roundoff; every count is first order, each rounding taken at its
full half ulp with the same sign.  Nothing was chosen by looking at device output.
  d2      the L squares round once each and L additions of positive terms follow: |got - ref| <= (L + 1) u ref, as in
          _projection_ref.  (The device and this restatement add in the same order, so in fact they agree bit for bit; the
          bound does not rely on it.)
  sqrt    sqrt(d (1 + e)) = sqrt(d) (1 + e / 2): the root halves the relative error, (L + 1) / 2 u, and rounds once:
          (L + 1) / 2 u + u = (L + 3) / 2 u per term.
  sum     n_s non-negative terms added in any order: at most (n_s - 1) u times their sum more.
          |got - ref| <= ((L + 3) / 2 + n_s) u sums[i][s] + tiny          (sum_bound; n_s - 1 rounded up to n_s)
  The reference sum is taken in long double, whose own error (n_s 2^-64) is a thousandth of that.
Hamming sums are integers and exact.  The silhouette is finished on the host in both implementations: (b - a) / max(a, b)
moves by a few u of its operands, and scikit-learn's own samples sit 8e-16 from this restatement on the fixture (Euclidean
through its expanded-form distances, Hamming through mean(x != y) = count / L); the tests hold both to 1e-12.
"""
import numpy as np

from _projection_ref import TINY, U, hard_codes, knn, rejects, sqdist, within  # noqa: F401

LD = np.longdouble
BAD = (0x7FFFFFFF, -1)                  # entries of nbr that are no row: rbvae_knn's unfilled slot, a negative index


# ---- neighbour ranks -----------------------------------------------------------------------------------------------------

def random_neighbours(N, k, seed):
    """[N, k] int32: k random other rows per row (with repeats): ranks from 1 to N - 1 all occur"""
    r = np.random.RandomState(seed)
    nb = r.randint(0, N - 1, (N, k))
    return (nb + (nb >= np.arange(N)[:, None])).astype(np.int32)


def soft_rows(N, Ld, seed):
    r = np.random.RandomState(seed)
    return (1.0 / (1.0 + np.exp(-2.0 * r.randn(N, Ld)))).astype(np.float32)


def ranks(X, nbr, defect=None, D=None):
    """-> (rank [N, k] int32, excess [N] int64, decided [N, k] bool).  rank = 1 + the number of rows m != i that come
    before j = nbr[i, r] in the order (d2(i, .), index); -1 where j is no other row.
    defects: "rank_counts_self" (m = i is counted: d2 = 0 comes before everything), "tie_high" (equal distances go to the
    higher index)."""
    D = sqdist(X) if D is None else D
    N, k = nbr.shape
    rank = np.full((N, k), -1, dtype=np.int32)
    decided = np.ones((N, k), dtype=bool)
    m = np.arange(N)
    for i in range(N):
        d = D[i][None, :]
        j = nbr[i].astype(np.int64)
        ok = (j >= 0) & (j < N) & (j != i)
        j = np.where(ok, j, 0)[:, None]
        dj = D[i][j]                                        # [k, 1]
        tie = (m[None, :] > j) if defect == "tie_high" else (m[None, :] < j)
        before = (d < dj) | ((d == dj) & tie)               # [k, N]
        near = (np.abs(d - dj) < 1e-12 * dj) & (d != dj)
        near[:, i] = False
        if defect != "rank_counts_self":
            before[:, i] = False
        rank[i] = np.where(ok, 1 + before.sum(1), -1)
        decided[i] = ~near.any(1) | ~ok
    excess = np.where(rank > k, rank - k, 0).astype(np.int64).sum(1)
    return rank, excess, decided


def trust_from_excess(excess, N, k):
    """sklearn.manifold.trustworthiness' last line, from the exact integer sum of the excesses"""
    t = int(np.asarray(excess, dtype=np.int64).sum())
    return 1.0 - t * (2.0 / (N * k * (2.0 * N - 3.0 * k - 1.0)))


def trustworthiness(X, Y, k, defect=None):
    """the ranks in X of the k nearest neighbours in Y (by (d2, index), self excluded)"""
    idx, _, _ = knn(Y, k)
    _, excess, _ = ranks(X, idx, defect)
    return trust_from_excess(excess, len(X), k)


# ---- per-state sums ------------------------------------------------------------------------------------------------------

def group(lab, S):
    """(order [N] int32: rows grouped by state, ascending within a state; seg [S + 1] int32: the states' offsets)"""
    lab = np.asarray(lab, dtype=np.int64)
    order = np.concatenate([np.nonzero(lab == s)[0] for s in range(S)]).astype(np.int32)
    seg = np.zeros(S + 1, dtype=np.int32)
    for s in range(S):
        seg[s + 1] = seg[s] + int((lab == s).sum())
    return order, seg


def dist_sums(X, lab, S, D=None):
    """sums [N, S] f64 (added in long double): sums[i, s] = sum over the rows j of state s of sqrt(d2(i, j))"""
    root = np.sqrt(sqdist(X) if D is None else D).astype(LD)
    lab = np.asarray(lab)
    return np.stack([root[:, lab == s].sum(1) for s in range(S)], axis=1).astype(np.float64)


def sum_bound(Ld, lab, S, sums):
    n = np.bincount(np.asarray(lab, dtype=np.int64), minlength=S).astype(np.float64)
    return ((Ld + 3) / 2.0 + n[None, :]) * U * sums + TINY


def hamming_sums(C, lab, S):
    """sums [N, S] int64: the number of differing bits of the codes C > 0.5, summed over the rows of state s"""
    B = np.asarray(C) > 0.5
    ham = (B[:, None, :] != B[None, :, :]).sum(-1)
    lab = np.asarray(lab)
    return np.stack([ham[:, lab == s].sum(1) for s in range(S)], axis=1).astype(np.int64)


def silhouette(sums, lab, S, defect=None):
    """silhouette samples [N] f64 from sums [N, S], row by row.
    defects: "a_over_n" (the own-state mean divided by n instead of n - 1), "b_includes_own" (the row's own state takes
    part in the minimum), "empty_state_is_zero" (an empty state's mean is 0 and wins the minimum), "singleton_not_zero" (a
    row alone in its state keeps a = 0 and scores (b - 0) / b)."""
    sums = np.asarray(sums, dtype=np.float64)
    lab = np.asarray(lab, dtype=np.int64)
    n = np.bincount(lab, minlength=S)
    out = np.zeros(len(lab))
    for i, own in enumerate(lab):
        if n[own] == 1 and defect != "singleton_not_zero":
            continue
        a = 0.0 if n[own] == 1 else sums[i, own] / (n[own] if defect == "a_over_n" else n[own] - 1)
        means = []
        for s in range(S):
            if s == own and defect != "b_includes_own":
                continue
            if n[s] == 0:
                if defect == "empty_state_is_zero":
                    means.append(0.0)
                continue
            means.append(sums[i, s] / n[s])
        b = min(means)
        out[i] = 0.0 if max(a, b) == 0.0 else (b - a) / max(a, b)
    return out


# ---- kNN label agreement ---------------------------------------------------------------------------------------------------

def agreement(idx, lab, S, defect=None):
    """-> (purity, predictions [N], accuracy, tied rows) from neighbour indices [N, k].  defect "vote_tie_high": a tied
    vote goes to the largest label."""
    lab = np.asarray(lab, dtype=np.int64)
    nl = lab[np.asarray(idx, dtype=np.int64)]
    purity = float((nl == lab[:, None]).sum()) / nl.size
    pred, tied = np.zeros(len(lab), dtype=np.int64), 0
    for i, row in enumerate(nl):
        votes = np.bincount(row, minlength=S)
        best = np.nonzero(votes == votes.max())[0]
        tied += len(best) > 1
        pred[i] = best[-1] if defect == "vote_tie_high" else best[0]
    return purity, pred, float((pred == lab).sum()) / len(lab), tied


def edge_states(N, S, seed):
    """labels in [0, S) with state 1 empty and state S - 1 a singleton (row N // 2)"""
    lab = np.random.RandomState(seed).randint(0, S - 1, N)
    lab[lab == 1] = 0
    lab[N // 2] = S - 1
    return lab
