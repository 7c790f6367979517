"""CPU: tests/_dtw_ref.py (the f64 restatement the GPU tests compare csrc/dtw.hip with) against the brute-force enumeration of
all warping paths on every shape up to 5 x 5, against two tables worked by hand, and for the properties of its paths; the
named defects of the restatement on the GPU test's own inputs; alignment.warp_map and transfer_labels on hand-made paths; and
the limits of rbvae_dtw_ok and the two size queries, which need the library but no GPU.
"""
import itertools

import numpy as np
import pytest

import _dtw_ref as R
import sfv_amd as sfv

q = sfv._lib.query
TI, TJ = q("rbvae_dtw_tile_rows"), q("rbvae_dtw_tile_cols")
TILE = (TI, TJ)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---- the restatement against all paths ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,M", list(itertools.product(range(1, 6), range(1, 6))))
def test_cost_is_the_minimum_over_all_paths(N, M):
    for kind, L in (("soft", 3), ("repeat", 2), ("code", 32)):
        X, Y = R.make(kind, N, M, L, seed=1)
        for metric in R.metrics_of(kind):
            d = R.cost_matrix(X, Y, metric)
            # a tile of 2 x 3 puts tile edges inside even these tables
            for sub, window in ((False, None), (True, None), (False, abs(N - M)), (False, abs(N - M) + 1)):
                got = R.dtw_from_cost(d, window, sub, tile=(2, 3))
                assert got["cost"] == R.brute(d, window, sub), (kind, metric, sub, window)
                same = R.dtw_from_cost(d, window, sub, tile=TILE)
                assert np.array_equal(_bits(got["D"]), _bits(same["D"])) and np.array_equal(got["dirs"], same["dirs"])


def test_hand_worked_euclidean_table():
    X = np.array([[0.0], [3.0], [4.0]], dtype=np.float32)
    Y = np.array([[0.0], [1.0], [4.0], [4.0]], dtype=np.float32)
    # d = |x - y|:   0 1 4 4      D:  0 1 5 9     dirs: 3 2 2 2
    #                3 2 1 1          3 2 2 3           1 0 0 2   (1, 3): diagonal 5, up 9, left 2: left
    #                4 3 0 0          7 5 2 2           1 1 0 0   (2, 1): diagonal 3, up 2, left 7: up; (2, 2): diagonal 2, up 2:
    #                                                             the diagonal wins the tie, and at (2, 3) against left 2
    got = R.dtw(X, Y, "euclidean")
    assert np.array_equal(got["D"], [[0, 1, 5, 9], [3, 2, 2, 3], [7, 5, 2, 2]])
    assert np.array_equal(got["dirs"], [[3, 2, 2, 2], [1, 0, 0, 2], [1, 1, 0, 0]])
    assert got["path"].tolist() == [[0, 0], [0, 1], [1, 2], [2, 3]] and got["cost"] == 2.0
    assert (got["start"], got["end"]) == (0, 3)
    sq = R.dtw(X, Y, "sqeuclidean")
    assert np.array_equal(sq["D"], [[0, 1, 17, 33], [9, 4, 2, 3], [25, 13, 2, 2]])
    assert np.array_equal(got["packed"], [[3 | 2 << 2 | 2 << 4 | 2 << 6], [1 | 2 << 6], [1 | 1 << 2]])
    assert np.array_equal(R.unpack_dirs(got["packed"], 4), got["dirs"])


def test_hand_worked_hamming_table_with_ties():
    X = np.zeros((3, 40), dtype=np.float32)
    Y = np.zeros((3, 40), dtype=np.float32)
    X[1, 35] = X[2, 35] = X[2, 3] = 1.0                     # rows 0, {35}, {3, 35}: bits in both words
    Y[0, 35] = Y[2, 3] = 1.0                                # rows {35}, 0, {3}
    # d:  1 0 1     D:  1 1 2     dirs: 3 2 2
    #     0 1 2         1 2 3           1 0 0     (1, 1): diagonal 1, up 1, left 1: diagonal
    #     1 2 1         2 3 3           1 0 0     (2, 1): diagonal 1, up 2, left 2; (2, 2): diagonal 2, up 3, left 3
    got = R.dtw(X, Y, "hamming")
    assert np.array_equal(got["D"], [[1, 1, 2], [1, 2, 3], [2, 3, 3]])
    assert np.array_equal(got["dirs"], [[3, 2, 2], [1, 0, 0], [1, 0, 0]])
    assert got["path"].tolist() == [[0, 0], [1, 1], [2, 2]] and got["cost"] == 3.0
    up = R.dtw(X, Y, "hamming", defect="tie_up_first")
    assert np.array_equal(up["D"], got["D"]) and up["dirs"][1, 1] == 1 and up["path"].tolist() != got["path"].tolist()
    # subsequence: row 0 is d itself, the end the lowest j among the smallest of the last row
    sub = R.dtw(X, Y, "hamming", subsequence=True)
    assert np.array_equal(sub["D"], [[1, 0, 1], [1, 1, 2], [2, 3, 2]]) and np.array_equal(sub["dirs"][0], [3, 3, 3])
    assert (sub["start"], sub["end"], sub["cost"]) == (0, 0, 2.0) and sub["path"].tolist() == [[0, 0], [1, 0], [2, 0]]
    assert R.dtw(X, Y, "hamming", subsequence=True, defect="end_last_min")["end"] == 2
    # a band of 0 on a square table is the diagonal
    band = R.dtw(X, Y, "hamming", window=0)
    assert band["path"].tolist() == [[0, 0], [1, 1], [2, 2]] and np.isinf(band["D"][0, 1]) and band["dirs"][0, 1] == 3


@pytest.mark.parametrize("kind,L,N,M", [c for c in R.global_cases(TI, TJ) if c[2] * c[3] <= 4 * TI * TJ][::3])
def test_path_properties(kind, L, N, M):
    X, Y = R.make(kind, N, M, L)
    for metric in R.metrics_of(kind):
        d = R.cost_matrix(X, Y, metric)
        for sub in (False, True):
            got = R.dtw_from_cost(d, None, sub, TILE)
            p = got["path"]
            assert p[0, 0] == 0 and p[-1, 0] == N - 1 and p[-1, 1] == got["end"] and p[0, 1] == got["start"]
            assert sub or (got["start"], got["end"]) == (0, M - 1)
            steps = {tuple(s) for s in np.diff(p, axis=0).tolist()}
            assert steps <= {(1, 1), (1, 0), (0, 1)} and len(p) <= N + M - 1
            assert not sub or (p[:, 0] == 0).sum() == 1     # an open begin never walks along row 0
            along = d[p[:, 0], p[:, 1]]
            if metric == "hamming":
                assert along.sum() == got["cost"]           # integers: exact in any order
            else:
                s = 0.0
                for v in along.tolist():
                    s = v + s
                assert s == got["cost"]                     # the table's own additions, in path order


# ---- the defects have teeth on the GPU test's inputs --------------------------------------------------------------------------------------

def _differs(a, b):
    return (not np.array_equal(_bits(a["D"]), _bits(b["D"])) or not np.array_equal(a["dirs"], b["dirs"])
            or a["path"].tolist() != b["path"].tolist() or a["end"] != b["end"])


def _gpu_inputs(defect):
    """the GPU test's cases on which the defect can show, smallest first: (X, Y, metric, window, subsequence)"""
    if defect in ("subseq_row0_accumulates", "end_last_min"):
        for _, metric, X, Y in R.subsequence_cases(TI, TJ):
            yield X, Y, metric, None, True
    elif defect == "band_off_by_one":
        for kind, L, metric, N, M, w in R.band_cases(TI, TJ):
            if w >= abs(N - M):
                yield (*R.make(kind, N, M, L), metric, w, False)
    else:
        for kind, L, N, M in sorted(R.global_cases(TI, TJ), key=lambda c: c[2] * c[3]):
            for metric in R.metrics_of(kind):
                yield (*R.make(kind, N, M, L), metric, None, False)


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_every_defect_shows_on_the_gpu_inputs(defect):
    shown = 0
    for X, Y, metric, w, sub in _gpu_inputs(defect):
        d = R.cost_matrix(X, Y, metric)
        if _differs(R.dtw_from_cost(d, w, sub, TILE), R.dtw_from_cost(d, w, sub, TILE, defect)):
            shown += 1
            if shown == 2:
                break
    assert shown >= 1, f"{defect} changes nothing on the GPU test's inputs"
    print(f"{defect}: shown")


def test_stale_corner_needs_a_tile_edge():
    """inside one tile the defect is silent, so shapes beyond a tile are what catches it"""
    X, Y = R.make("soft", TI, TJ, 50)
    d = R.cost_matrix(X, Y, "sqeuclidean")
    assert not _differs(R.dtw_from_cost(d, tile=TILE), R.dtw_from_cost(d, tile=TILE, defect="stale_corner"))
    X, Y = R.make("soft", TI + 1, TJ + 1, 50)
    d = R.cost_matrix(X, Y, "sqeuclidean")
    a, b = R.dtw_from_cost(d, tile=TILE), R.dtw_from_cost(d, tile=TILE, defect="stale_corner")
    assert a["D"][TI, TJ] != b["D"][TI, TJ] or a["dirs"][TI, TJ] != b["dirs"][TI, TJ]


def test_subsequence_cases_are_what_they_say():
    for kind, L, metric in (("code", 50, "hamming"), ("soft", 50, "sqeuclidean")):
        X, Y, pos = R.subsequence_case(kind, L, TI, TJ, 0)
        got = R.dtw(X, Y, metric, subsequence=True, tile=TILE)
        assert got["cost"] == 0.0 and (got["start"], got["end"]) == (pos, pos + len(X) - 1)
        assert pos < TJ <= got["end"] and len(Y) == 3 * TJ + 1 and len(X) == TI + 3
    X, Y, (a, b) = R.twice_case(50, TI, TJ)
    got = R.dtw(X, Y, "hamming", subsequence=True, tile=TILE)
    assert got["cost"] == 0.0 and got["end"] == a + len(X) - 1 and got["last_row"][b + len(X) - 1] == 0.0


# ---- the library's queries ----------------------------------------------------------------------------------------------------------------

def test_limits_without_a_gpu():
    assert q("rbvae_version") >= 109 and TI >= 2 and TJ >= 4 and TJ % 4 == 0
    ok = lambda *a: q("rbvae_dtw_ok", *a)                   # noqa: E731  (N, M, L, metric, window, subsequence)
    for a in ((1, 1, 1, 0, -1, 0), (16384, 16384, 128, 2, -1, 1), (100, 90, 50, 1, 10, 0), (100, 90, 50, 0, 1 << 30, 0),
              (7, 300, 3, 0, -1, 1), (300, 7, 3, 2, 293, 0)):
        assert ok(*a) == 1, a
    for a in ((0, 5, 3, 0, -1, 0), (5, 0, 3, 0, -1, 0), (16385, 5, 3, 0, -1, 0), (5, 16385, 3, 0, -1, 0), (5, 5, 0, 0, -1, 0),
              (5, 5, 129, 0, -1, 0), (5, 5, 3, 3, -1, 0), (5, 5, 3, -1, -1, 0), (100, 90, 50, 0, 9, 0), (90, 100, 50, 0, 9, 0),
              (5, 5, 3, 0, -2, 0), (5, 5, 3, 0, 0, 1), (5, 9, 3, 0, 100, 1), (5, 5, 3, 0, -1, 2)):
        assert ok(*a) == 0, a
    for N, M in ((1, 1), (5, 7), (TI, TJ), (TI + 1, TJ + 1), (16384, 16384), (12298, 9000)):
        tiles = -(-N // TI) * -(-M // TJ)
        assert q("rbvae_dtw_ws_bytes", N, M) == 8 * (N + M + tiles)
        assert q("rbvae_dtw_dirs_bytes", N, M) == N * ((M + 3) // 4)
    for N, M in ((0, 5), (5, 0), (16385, 1), (1, 16385), (-1, 4)):
        assert q("rbvae_dtw_ws_bytes", N, M) == 0 and q("rbvae_dtw_dirs_bytes", N, M) == 0
    assert q("rbvae_dtw_ws_bytes", 16384, 16384) < 1 << 20  # the product path stores no N x M doubles


# ---- the host helpers ---------------------------------------------------------------------------------------------------------------------

def test_warp_map_and_transfer_labels():
    path = [[0, 0], [1, 0], [2, 1], [2, 2], [3, 3], [4, 3], [5, 3]]
    w = sfv.warp_map(path, 6, 4)
    assert w["first_i"].tolist() == [0, 2, 2, 3] and w["last_i"].tolist() == [1, 2, 2, 5]
    assert w["first_j"].tolist() == [0, 0, 1, 3, 3, 3] and w["last_j"].tolist() == [0, 0, 2, 3, 3, 3]
    assert all(v.dtype == np.int64 for v in w.values())
    # j = 0 sees labels {2, 0}: a tie, the smallest; j = 3 sees {1, 1, 0}: the majority
    assert sfv.transfer_labels(path, [2, 0, 5, 1, 1, 0], 4).tolist() == [0, 5, 5, 1]
    assert sfv.transfer_labels(path, np.array([3, 3, 3, 0, 0, 1]), 4).tolist() == [3, 3, 3, 0]
    assert sfv.transfer_labels(path, [1, 1, 0, 2, 0, 1], 4).tolist() == [1, 0, 0, 0]       # {2, 0, 1}: a three-way tie
    # subsequence: the path covers rows 2 .. 3 of Y only
    sub = [[0, 2], [1, 2], [2, 3]]
    assert sfv.transfer_labels(sub, [4, 4, 1], 6).tolist() == [-1, -1, 4, 1, -1, -1]
    ws = sfv.warp_map(sub, 3, 6)
    assert ws["first_i"].tolist() == [-1, -1, 0, 2, -1, -1] and ws["last_i"].tolist() == [-1, -1, 1, 2, -1, -1]
    assert ws["first_j"].tolist() == [2, 2, 3]
    for call, match in ((lambda: sfv.warp_map([[0, 0], [1, 1]], 1, 2), "leaves"), (lambda: sfv.warp_map([[1, 1], [0, 0]], 2, 2), "ascending"),
                        (lambda: sfv.warp_map([0, 1], 2, 2), "len, 2"), (lambda: sfv.transfer_labels(path, [0, 1], 4), "leaves"),
                        (lambda: sfv.transfer_labels(path, [0, -1, 0, 0, 0, 0], 4), "non-negative")):
        with pytest.raises(ValueError, match=match):
            call()
    # on a restated path: every row of Y is covered, and a label that A holds throughout reaches every row of B
    X, Y = R.make("code", 9, 13, 32)
    got = R.dtw(X, Y, "hamming")
    assert sfv.transfer_labels(got["path"], np.full(9, 2), 13).tolist() == [2] * 13
    wm = sfv.warp_map(got["path"], 9, 13)
    assert wm["first_i"].min() >= 0 and np.all(np.diff(wm["first_i"]) >= 0) and np.all(wm["first_i"] <= wm["last_i"])
