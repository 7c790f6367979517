"""CPU: tests/_scores_ref.py (the f64 restatement the GPU tests compare the score kernels with) against the scikit-learn
fixture tests/golden/latent_scores.npz (tools/make_scores_golden.py), each check of the GPU tests against the named defect
it has to reject, and the host side of scores.py.  Nothing here reads the reference or scikit-learn.

Measured here: trustworthiness and continuity of the restatement differ from scikit-learn's by 0.0 at k = 5, 24 and 91
(the gate is 1e-15); its silhouette samples by at most 8.4e-16 (Euclidean) and 7.4e-16 (Hamming) on either label vector
(the gate is 1e-12: scikit-learn's Euclidean distances come from the expanded form |x|^2 - 2 x.y + |y|^2)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _scores_ref as R
import sfv_amd as sfv

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "latent_scores.npz")
K_TRUST, K_VOTE = (5, 24, 91), (5, 24)
# (N, L, k) of the GPU rank cases small enough for the host
RANK_CASES = [(2, 1, 1), (65, 3, 31), (257, 50, 24), (700, 128, 5)]


@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(GOLD))
    g["DX"], g["DY"] = R.sqdist(g["X"]), R.sqdist(g["Y"])
    return g


def _labels(gold, which):
    lab = gold["lab" + which].astype(np.int64)
    return lab, int(lab.max()) + 1


def test_fixture(gold):
    """every rank the fixture asks for is decided far above f64 rounding, in both directions; the labels are what the
    generator says: sorted, 8 states, and the edge vector has a gap (3 and 8 are empty) and a singleton (10)"""
    assert os.path.getsize(GOLD) <= 1 << 20
    for k in K_TRUST:
        for A, B in (("X", "Y"), ("Y", "X")):
            idx, _, dec = R.knn(gold[B], k, D=gold["D" + B])
            assert dec.all()
            assert R.ranks(gold[A], idx, D=gold["D" + A])[2].all(), (k, A)
    D = gold["DX"].copy()
    np.fill_diagonal(D, np.inf)
    srt = np.sort(D, axis=1)[:, :-1]
    gap = np.diff(srt, axis=1) / srt[:, 1:]
    print(f"smallest relative gap between two distances of a row: {gap[gap > 0].min():.3g}")
    assert gap.min() > 1e-10
    lab, lab_edge = gold["lab"], gold["lab_edge"]
    assert np.all(np.diff(lab) >= 0) and set(lab) == set(range(8))
    freq = np.bincount(lab_edge, minlength=11)
    assert freq[3] == 0 and freq[8] == 0 and freq[10] == 1 and lab_edge[0] == 10 and freq[9] == (lab == 3).sum() - (lab[0] == 3)


@pytest.mark.parametrize("k", K_TRUST)
def test_trustworthiness_equals_sklearn(gold, k):
    t, c = R.trustworthiness(gold["X"], gold["Y"], k), R.trustworthiness(gold["Y"], gold["X"], k)
    print(f"k = {k}: trustworthiness {t:.6f} (differs by {abs(t - gold[f'trust_{k}']):.3g}), continuity {c:.6f} (differs "
          f"by {abs(c - gold[f'cont_{k}']):.3g})")
    assert abs(t - float(gold[f"trust_{k}"])) <= 1e-15
    assert abs(c - float(gold[f"cont_{k}"])) <= 1e-15
    assert 0.5 < t < 0.9 and 0.5 < c < 0.9                  # nothing saturates on this fixture


@pytest.mark.parametrize("which", ["", "_edge"])
def test_silhouette_against_sklearn(gold, which):
    lab, S = _labels(gold, which)
    se = R.silhouette(R.dist_sums(gold["X"], lab, S, D=gold["DX"]), lab, S)
    sh = R.silhouette(R.hamming_sums(gold["X"], lab, S), lab, S)
    de, dh = np.abs(se - gold["sil_euclid" + which]).max(), np.abs(sh - gold["sil_hamming" + which]).max()
    print(f"silhouette{which}: mean {se.mean():.4f} / Hamming {sh.mean():.4f}; max |restatement - sklearn| {de:.3g} / {dh:.3g}")
    assert de <= 1e-12 and dh <= 1e-12
    if which:
        assert se[0] == 0.0 and sh[0] == 0.0                # the singleton


@pytest.mark.parametrize("k", K_VOTE)
def test_agreement_equals_sklearn(gold, k):
    idx, _, dec = R.knn(gold["X"], k, D=gold["DX"])
    assert dec.all() and np.array_equal(idx, gold[f"nn_{k}"])
    purity, pred, acc, tied = R.agreement(idx, gold["lab"], 8)
    print(f"k = {k}: purity {purity:.4f}, accuracy {acc:.4f}, {tied} tied votes")
    assert purity == float(gold[f"purity_{k}"]) and acc == float(gold[f"acc_{k}"])
    assert np.array_equal(pred, gold[f"pred_{k}"])
    assert tied == {5: 40, 24: 11}[k]


@pytest.mark.parametrize("N,Ld,k", RANK_CASES)
def test_rank_cases_are_decided(N, Ld, k):
    """the synthetic inputs of the GPU rank test: at least 99 % of their entries are decided"""
    X, nbr = R.soft_rows(N, Ld, N + Ld), R.random_neighbours(N, k, N + k)
    rank, excess, dec = R.ranks(X, nbr)
    assert dec.mean() >= 0.99
    assert rank.min() >= 1 and rank.max() <= N - 1 and not np.any(nbr == np.arange(N)[:, None])
    assert np.array_equal(excess, np.maximum(rank.astype(np.int64) - k, 0).sum(1))


# ---- the checks reject the named defects -----------------------------------------------------------------------------------

def test_rank_counts_self_rejected(gold):
    idx = R.knn(gold["Y"], 24, D=gold["DY"])[0]
    good, ex, _ = R.ranks(gold["X"], idx, D=gold["DX"])
    bad, exb, _ = R.ranks(gold["X"], idx, "rank_counts_self", D=gold["DX"])
    assert np.array_equal(bad, good + 1)
    assert abs(R.trust_from_excess(exb, 320, 24) - float(gold["trust_24"])) > 1e-3
    assert abs(R.trust_from_excess(ex, 320, 24) - float(gold["trust_24"])) <= 1e-15
    # a row's own nearest neighbours stand at ranks 1..k
    own = R.knn(gold["X"], 24, D=gold["DX"])[0]
    assert np.array_equal(R.ranks(gold["X"], own, D=gold["DX"])[0], np.broadcast_to(np.arange(1, 25), (320, 24)))
    assert not np.array_equal(R.ranks(gold["X"], own, "rank_counts_self", D=gold["DX"])[0][:, 0], np.ones(320))


def test_rank_tie_rule_rejected():
    """hard codes with many duplicates: integer distances, zero distances, exact ties, all decided by the index"""
    X = R.hard_codes()
    D = R.sqdist(X)
    idx, d2, _ = R.knn(X, 64, D=D)
    assert np.any(d2 == 0.0) and np.any(np.diff(d2, axis=1) == 0)
    rank, _, dec = R.ranks(X, idx, D=D)
    assert dec.all() and np.array_equal(rank, np.broadcast_to(np.arange(1, 65), rank.shape))
    bad = R.ranks(X, idx, "tie_high", D=D)[0]
    assert not np.array_equal(bad, rank)
    nbr = R.random_neighbours(len(X), 7, 1)
    assert not np.array_equal(R.ranks(X, nbr, "tie_high", D=D)[0], R.ranks(X, nbr, D=D)[0])


@pytest.mark.parametrize("defect,which", [("a_over_n", ""), ("b_includes_own", ""), ("empty_state_is_zero", "_edge"),
                                          ("singleton_not_zero", "_edge")])
@pytest.mark.parametrize("metric", ["euclid", "hamming"])
def test_silhouette_defects_rejected(gold, defect, which, metric):
    lab, S = _labels(gold, which)
    sums = R.dist_sums(gold["X"], lab, S, D=gold["DX"]) if metric == "euclid" else R.hamming_sums(gold["X"], lab, S)
    ref = gold[f"sil_{metric}{which}"]
    assert np.abs(R.silhouette(sums, lab, S) - ref).max() <= 1e-12
    bad = R.silhouette(sums, lab, S, defect)
    assert np.abs(bad - ref).max() > 1e-3, f"{defect} passes the silhouette gate"
    if defect == "singleton_not_zero":
        assert bad[0] == 1.0 and np.abs(bad[1:] - ref[1:]).max() <= 1e-12


def test_sum_bound_rejects_a_dropped_row(gold):
    """the Euclidean bound is tight enough to mean something: one row missing from a state, or a relative error of 1e-12,
    is outside; a plain f64 sum in another order is inside"""
    lab, S = _labels(gold, "_edge")
    sums = R.dist_sums(gold["X"], lab, S, D=gold["DX"])
    bnd = R.sum_bound(50, lab, S, sums)
    assert bnd.max() <= 1e-13 * sums.max()
    root = np.sqrt(gold["DX"])
    plain = np.stack([root[:, lab == s][:, ::-1].sum(1) if (lab == s).any() else np.zeros(320) for s in range(S)], axis=1)
    R.within(plain, sums, bnd, "f64 sums in reverse order")
    short = lab.copy()
    short[5] = 7                                            # row 5 leaves state 0
    assert R.rejects(R.dist_sums(gold["X"], short, S, D=gold["DX"])[:, 0], sums[:, 0], bnd[:, 0])
    assert R.rejects(sums * (1 + 1e-12), sums, bnd)
    assert np.all(sums[:, [3, 8]] == 0.0)                   # the empty states


@pytest.mark.parametrize("k", K_VOTE)
def test_vote_tie_rule_rejected(gold, k):
    _, pred, acc, tied = R.agreement(gold[f"nn_{k}"], gold["lab"], 8, "vote_tie_high")
    assert tied > 0 and not np.array_equal(pred, gold[f"pred_{k}"])


# ---- the host side of the package ------------------------------------------------------------------------------------------

NEW = ("rbvae_nbr_ranks_ok", "rbvae_nbr_ranks", "rbvae_label_sums_ok", "rbvae_label_dist_sums", "rbvae_label_hamming_sums")


def test_header_and_library():
    protos = sfv._lib.parse_header()
    raw = ctypes.CDLL(sfv._lib.LIB_PATH)
    for name in NEW:
        assert name in protos and hasattr(raw, name), name
    assert [len(protos[n][1]) for n in NEW] == [3, 8, 3, 8, 8]
    q = sfv._lib.query
    assert q("rbvae_nbr_ranks_ok", 12298, 50, 24) == 1 and q("rbvae_nbr_ranks_ok", 16384, 128, 128) == 1
    assert q("rbvae_nbr_ranks_ok", 2, 1, 1) == 1 and q("rbvae_nbr_ranks_ok", 16385, 2, 3) == 0
    assert q("rbvae_nbr_ranks_ok", 10, 4, 10) == 0 and q("rbvae_nbr_ranks_ok", 100, 129, 5) == 0
    assert q("rbvae_nbr_ranks_ok", 1, 4, 1) == 0 and q("rbvae_nbr_ranks_ok", 300, 4, 129) == 0
    assert q("rbvae_label_sums_ok", 12298, 50, 17) == 1 and q("rbvae_label_sums_ok", 16384, 128, 256) == 1
    assert q("rbvae_label_sums_ok", 16385, 50, 17) == 0 and q("rbvae_label_sums_ok", 100, 129, 3) == 0
    assert q("rbvae_label_sums_ok", 100, 8, 257) == 0 and q("rbvae_label_sums_ok", 100, 8, 0) == 0
    for N, Ld, k in RANK_CASES + [(320, 50, 5), (320, 50, 24), (4100, 2, 24), (16384, 2, 3)]:
        assert q("rbvae_nbr_ranks_ok", N, Ld, k) == q("rbvae_knn_ok", N, Ld, k) == 1


def test_cpu_inputs_raise():
    X, Y = torch.zeros((8, 4)), torch.zeros((8, 2))
    lab = np.array([0, 0, 0, 0, 1, 1, 1, 1])
    with pytest.raises(ValueError, match="GPU"):
        sfv.neighbour_ranks(X, torch.zeros((8, 3), dtype=torch.int32))
    with pytest.raises(ValueError, match="GPU"):
        sfv.trustworthiness(X, Y, 3)
    with pytest.raises(ValueError, match="GPU"):
        sfv.continuity(X, Y, 3)
    with pytest.raises(ValueError, match="GPU"):
        sfv.label_distance_sums(X, lab, 2)
    with pytest.raises(ValueError, match="GPU"):
        sfv.silhouette_samples(X, lab)
    with pytest.raises(ValueError, match="GPU"):
        sfv.silhouette_score(X, lab, metric="hamming")
    with pytest.raises(ValueError, match="GPU"):
        sfv.knn_label_agreement(X, lab, 3)
    with pytest.raises(ValueError, match="GPU"):
        sfv.latent_scores(None, torch.zeros((2, 3, 8, 8)), [0, 1], [1])
    with pytest.raises(ValueError, match="tensor"):
        sfv.trustworthiness(np.zeros((8, 4), dtype=np.float32), Y, 3)
    assert sfv.scores.trustworthiness is sfv.trustworthiness and sfv.scores.MAX_STATES == 256
