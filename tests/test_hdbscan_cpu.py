"""CPU: tests/_hdbscan_ref.py, the f64 restatement of csrc/hdbscan.hip, against scikit-learn 1.7.2's HDBSCAN and scipy's minimum
spanning tree as recorded in tests/golden/hdbscan.npz (tools/make_hdbscan_golden.py) and, where both are installed, run live;
and the library's host half (rbvae_hdbscan_tree / rbvae_hdbscan_cut, which make no GPU call) against the restatement bit for bit.

What scikit-learn is held to be the reference for: the sorted weights of the tree (exactly), every recorded cut (as a
partition), the number of clusters on every case, and labels (as a partition) and probabilities (bit for bit) on the cases the
fixture marks `agrees` -- all four with min_samples = 1 and four of the seven with min_samples >= 2.  On the others its answer
depends on the order of the rows: the fixture's permutation_note records that its own labels did not survive a row permutation
of case m3_a, while the restatement's do (test_restatement_is_order_free).

The named defects, each of which the gates reject (test_named_defects, test_eom_tie):
  binary            merging the edges of one level one at a time makes a nested chain of nodes at one lambda, whose shape follows
                    the edges' order; on the fixture it changes labels or probabilities, so library == restatement catches it
  eom_ge            `>=` in the excess-of-mass test drops a cluster whose children only EQUAL it; the hand-made tree of
                    test_eom_tie has such a cluster
  lmax_descendants  lambda_max taken over a cluster's descendants makes the probabilities of a selected cluster with children too
                    small; it disagrees with scikit-learn's probabilities on an `agrees` case
  core_off_by_one   min_samples counted without the row itself moves every core distance; the tree's weights then differ from
                    scipy's
"""
import ctypes
import functools

import numpy as np
import pytest

import _hdbscan_ref as R

CASES = R.golden_cases()
IDS = [c["name"] for c in CASES]
I32, F64 = np.int32, np.float64


@functools.lru_cache(maxsize=None)
def ref_fit(name, method="eom", defect=None):
    c = next(c for c in CASES if c["name"] == name)
    return R.hdbscan(c["X"], c["mcs"], c["m"], method, defect)


def lib_tree(edges, d, N, mcs, method="eom"):
    import sfv_amd as sfv
    labels, prob, table = sfv.density._host_tree(edges, d, N, mcs, method)
    return {"labels": labels, "prob": prob, "table": table, "n_clusters": int(table["selected"].sum())}


def lib_cut(edges, d, N, cut_distance, mcs):
    import sfv_amd as sfv
    labels, n = np.empty(N, dtype=I32), np.zeros(1, dtype=I32)
    sfv.density._host_call("rbvae_hdbscan_cut", np.ascontiguousarray(edges, dtype=I32), np.ascontiguousarray(d, dtype=F64), N,
                           float(cut_distance), mcs, labels, n)
    return labels, int(n[0])


# ---- the restatement against scikit-learn and scipy --------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_against_fixture(case):
    N = len(case["X"])
    got = ref_fit(case["name"])
    assert np.array_equal(got["d"], case["mst_w"]), "the tree's sorted weights are scipy's"
    assert (got["edges"][:, 0] < got["edges"][:, 1]).all() and len(got["edges"]) == N - 1
    for cut_distance, want in case["cuts"]:
        labels, n = R.cut(got["edges"], got["d"], N, cut_distance, case["mcs"])
        assert R.same_partition(labels, want) and n == int(want.max()) + 1, f"cut at {cut_distance}"
    assert got["n_clusters"] == case["n_clusters"]
    if case["agrees"]:
        assert R.same_partition(got["labels"], case["labels"])
        assert np.array_equal(got["prob"].view(np.int64), case["prob"].view(np.int64))


def test_fixture_conditions():
    g = R.golden()
    assert str(g["sklearn"]) == "1.7.2"
    assert all(c["agrees"] for c in CASES if c["m"] == 1) and sum(c["m"] == 1 for c in CASES) >= 4
    assert sum(c["agrees"] and c["m"] >= 2 for c in CASES) >= 3
    marked = [c["name"] for c in CASES if not c["agrees"]]
    assert marked, "the cases that do not agree are kept and marked"
    note = str(g["permutation_note"])
    assert marked[0] in note and "ANOTHER partition" in note, note
    for c in CASES:
        N = len(c["X"])
        assert c["X"].dtype == np.float32 and 100 <= N <= 600 and 2 <= c["mcs"] <= N and c["labels"].dtype == I32
        assert (c["mst_w"] > 0).all(), "no duplicate rows: scipy reads a zero as no edge"
        for cut_distance, _ in c["cuts"]:
            assert np.abs(c["mst_w"] / cut_distance - 1.0).min() > 1e-9


@pytest.mark.parametrize("name", ["m1_c", "m5_b", "m3_a"])
def test_restatement_against_live_sklearn(name):
    sk = pytest.importorskip("sklearn.cluster")
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    import _dbscan_ref as D
    case = next(c for c in CASES if c["name"] == name)
    N, got = len(case["X"]), ref_fit(name)
    D2 = D.d2_matrix(case["X"])
    dist = np.sqrt(D2)
    c = np.sqrt(R.core2(D2, case["m"]))
    mr = np.maximum(np.maximum(c[:, None], c[None, :]), dist)
    np.fill_diagonal(mr, 0.0)
    assert np.array_equal(np.sort(csgraph.minimum_spanning_tree(mr).data), got["d"])
    fit = sk.HDBSCAN(min_cluster_size=case["mcs"], min_samples=case["m"], metric="precomputed", copy=True).fit(dist)
    assert int(fit.labels_.max()) + 1 == got["n_clusters"]
    for cut_distance, _ in case["cuts"]:
        assert R.same_partition(fit.dbscan_clustering(cut_distance, min_cluster_size=case["mcs"]),
                                R.cut(got["edges"], got["d"], N, cut_distance, case["mcs"])[0])
    if case["agrees"]:
        assert R.same_partition(fit.labels_, got["labels"])
        assert np.array_equal(fit.probabilities_.view(np.int64), got["prob"].view(np.int64))


def test_restatement_is_order_free():
    case = next(c for c in CASES if not c["agrees"])
    got = ref_fit(case["name"])
    perm = np.random.RandomState(5).permutation(len(case["X"]))
    again = R.hdbscan(case["X"][perm], case["mcs"], case["m"])
    assert R.same_partition(again["labels"], got["labels"][perm])
    assert np.array_equal(again["prob"].view(np.int64), got["prob"][perm].view(np.int64))
    assert np.array_equal(again["d"], got["d"])
    for k in ("birth", "lambda_max", "stability", "size"):     # bit for bit: one product and one add per level, n whole
        assert np.array_equal(np.sort(again["table"][k]).view(np.uint8), np.sort(got["table"][k]).view(np.uint8)), k


# ---- the library's host half against the restatement -------------------------------------------------------------------------

@pytest.mark.parametrize("method", ["eom", "leaf"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_library_equals_restatement(case, method):
    N, want = len(case["X"]), ref_fit(case["name"], method)
    got = lib_tree(want["edges"], want["d"], N, case["mcs"], method)
    assert R.same_fit(got, want) and got["n_clusters"] == want["n_clusters"]
    if method == "leaf":
        t = want["table"]
        assert np.array_equal(t["selected"][1:] == 1, ~np.isin(np.arange(1, len(t["parent"])), t["parent"]))
        return
    for cut_distance, sk in case["cuts"]:
        labels, n = lib_cut(want["edges"], want["d"], N, cut_distance, case["mcs"])
        ref_labels, ref_n = R.cut(want["edges"], want["d"], N, cut_distance, case["mcs"])
        assert np.array_equal(labels, ref_labels) and n == ref_n and R.same_partition(labels, sk)


def test_chain_dendrogram_is_n_deep():
    N = 16384
    edges, d = R.chain_tree(N)
    for mcs in (2, 100, N):
        want = R.tree(edges, d, N, mcs)
        got = lib_tree(edges, d, N, mcs)
        assert R.same_fit(got, want)
        assert len(want["table"]["parent"]) == 1 and (got["labels"] == -1).all() and (got["prob"] == 0).all()   # nothing splits
    labels, n = lib_cut(edges, d, N, 8000.0, 2)
    assert n == 1 and (labels[:8001] == 0).all() and (labels[8001:] == -1).all()
    # the chain at both ends of two blobs: depth and a split at once
    e2 = np.concatenate([edges[:N // 2 - 1], edges[N // 2:], edges[N // 2 - 1:N // 2]])
    d2 = np.concatenate([d[:N // 2 - 1], d[:N // 2 - 1] + 0.5, [float(N)]])
    order = np.lexsort((e2[:, 1], e2[:, 0], d2))
    want = R.tree(e2[order], d2[order], N, 50)
    got = lib_tree(e2[order], d2[order], N, 50)
    assert R.same_fit(got, want) and got["n_clusters"] == 2 and set(got["labels"][:N // 2]) == {0} and set(got["labels"][N // 2:]) == {1}


def test_duplicates_nothing_splits_and_whole_size():
    r = np.random.RandomState(3)
    X = R.blobs(150, 4, 3, 11)
    X[10:20] = X[0]                                         # eleven copies of one row: d = 0, lambda = inf
    X[140:] = X[139]
    for m, mcs in ((1, 5), (3, 5), (12, 5)):
        want = R.hdbscan(X, mcs, m)
        assert (want["d"] == 0).sum() >= (20 if m == 1 else 0)
        got = lib_tree(want["edges"], want["d"], len(X), mcs)
        assert R.same_fit(got, want)
        if m == 1:
            assert np.isinf(want["table"]["lambda_max"]).any() and (want["prob"][10:20] == 1.0).all()
    one = (0.1 * r.randn(90, 3)).astype(np.float32)         # one blob
    want = R.hdbscan(one, 40, 5)
    assert len(want["table"]["parent"]) == 1 and (want["labels"] == -1).all()
    assert R.same_fit(lib_tree(want["edges"], want["d"], 90, 40), want)
    full = R.hdbscan(X, len(X), 5)                          # min_cluster_size = N: only the root is that big
    assert len(full["table"]["parent"]) == 1 and R.same_fit(lib_tree(full["edges"], full["d"], len(X), len(X)), full)
    labels, n = lib_cut(full["edges"], full["d"], len(X), float(full["d"][-1]), len(X))
    assert n == 1 and (labels == 0).all()


EOM_TIE = (np.array([[0, 1], [2, 3], [8, 9], [1, 2], [3, 4], [4, 5], [5, 6], [6, 7], [7, 8]], dtype=I32),
           np.array([.25, .25, .25, .5, .5, .5, .5, .5, 1.0]))


def test_eom_tie():
    """rows 0 .. 7 are cluster A, born at 1, which at lambda 2 splits into {0, 1} and {2, 3} while 4 .. 7 leave: stability
    (2 - 1) * 8 = 8; the two children die at 4: (4 - 2) * 2 = 4 each.  8 > 8 is false: A is selected."""
    edges, d = EOM_TIE
    want = R.tree(edges, d, 10, 2)
    assert want["labels"].tolist() == [0] * 8 + [1, 1] and want["table"]["stability"].tolist() == [10.0, 8.0, 6.0, 4.0, 4.0]
    assert want["table"]["selected"].tolist() == [0, 1, 1, 0, 0] and want["table"]["parent"].tolist() == [-1, 0, 0, 1, 1]
    assert want["prob"].tolist() == [1.0] * 10
    assert R.same_fit(lib_tree(edges, d, 10, 2), want)
    bad = R.tree(edges, d, 10, 2, defect="eom_ge")
    assert bad["labels"].tolist() == [0, 0, 1, 1, -1, -1, -1, -1, 2, 2]
    leaf = lib_tree(edges, d, 10, 2, "leaf")
    assert leaf["labels"].tolist() == [0, 0, 1, 1, -1, -1, -1, -1, 2, 2] and R.same_fit(leaf, R.tree(edges, d, 10, 2, "leaf"))


def test_named_defects():
    differs = {k: [c["name"] for c in CASES if not R.same_fit(ref_fit(c["name"], "eom", k), ref_fit(c["name"]))]
               for k in ("binary", "lmax_descendants", "core_off_by_one")}
    assert all(differs.values()), differs                   # library == restatement on the fixture would catch each
    agree = [c for c in CASES if c["agrees"]]
    bad = [c["name"] for c in agree
           if not np.array_equal(ref_fit(c["name"], "eom", "lmax_descendants")["prob"].view(np.int64), c["prob"].view(np.int64))]
    assert bad, "lambda_max over the descendants passes scikit-learn's probabilities"
    for c in CASES:                                         # (m = 1 -> 2 changes nothing: d >= both rows' nearest distance)
        assert c["m"] == 1 or not np.array_equal(ref_fit(c["name"], "eom", "core_off_by_one")["d"], c["mst_w"]), c["name"]


def _raw_tree(edges, d, N, mcs, method=0):
    """the entry itself on sentinel-filled outputs -> (rc, every output untouched)"""
    import sfv_amd as sfv
    lib = sfv._lib.lib()
    outs = [np.full(N, -77, dtype=I32), np.full(N, -7.5), np.full(N, -77, dtype=I32), np.full(N, -7.5), np.full(N, -7.5),
            np.full(N, -7.5), np.full(N, -77, dtype=I32), np.full(N, -77, dtype=I32), np.full(N, -77, dtype=I32),
            np.full(1, -77, dtype=I32)]
    e, w = np.ascontiguousarray(edges, dtype=I32), np.ascontiguousarray(d, dtype=F64)
    rc = lib.rbvae_hdbscan_tree(e.ctypes.data, w.ctypes.data, N, mcs, method, *[o.ctypes.data for o in outs])
    cut = [np.full(N, -77, dtype=I32), np.full(1, -77, dtype=I32)]
    rc2 = lib.rbvae_hdbscan_cut(e.ctypes.data, w.ctypes.data, N, ctypes.c_double(1.0), mcs, *[o.ctypes.data for o in cut])
    clean = [all((o == (-77 if o.dtype == I32 else -7.5)).all() for o in group) for group in (outs, cut)]
    return rc, rc2, clean[0] and (clean[1] or rc2 == 0)


def test_refused_inputs_write_nothing():
    import sfv_amd as sfv
    E = sfv._lib
    edges, d = EOM_TIE
    assert _raw_tree(edges, d, 10, 2)[:2] == (0, 0)
    cycle = edges.copy()
    cycle[8] = [0, 3]                                       # 0-1-2-3-0, and rows 8, 9 cut off: a forest with a cycle
    twice = edges.copy()
    twice[1] = [1, 0]                                       # one edge twice
    outside = edges.copy()
    outside[4] = [3, 10]
    nan, neg, inf, desc = d.copy(), d.copy(), d.copy(), d.copy()
    nan[3], neg[0], inf[8], desc[2] = np.nan, -0.25, np.inf, 0.125
    for what, (e, w, N, mcs, method) in {"cycle": (cycle, d, 10, 2, 0), "twice": (twice, d, 10, 2, 0),
                                         "outside": (outside, d, 10, 2, 0), "NaN": (edges, nan, 10, 2, 0),
                                         "negative": (edges, neg, 10, 2, 0), "inf": (edges, inf, 10, 2, 0),
                                         "descending": (edges, desc, 10, 2, 0), "mcs 1": (edges, d, 10, 1, 0),
                                         "mcs N + 1": (edges, d, 10, 11, 0), "method": (edges, d, 10, 2, 2)}.items():
        rc, rc2, clean = _raw_tree(e, w, N, mcs, method)
        assert rc == E.E_INVALID and clean, what
        assert rc2 == (0 if what == "method" else E.E_INVALID), what
    lib = E.lib()
    one = np.full(4, -77, dtype=I32)
    assert lib.rbvae_hdbscan_cut(edges.ctypes.data, d.ctypes.data, 1, ctypes.c_double(1.0), 2, one.ctypes.data, one.ctypes.data) \
        == E.E_UNSUPPORTED and (one == -77).all()
    assert lib.rbvae_hdbscan_cut(edges.ctypes.data, d.ctypes.data, 10, ctypes.c_double(-1.0), 2, one.ctypes.data, one.ctypes.data) \
        == E.E_INVALID and (one == -77).all()
    assert lib.rbvae_hdbscan_cut(None, d.ctypes.data, 10, ctypes.c_double(1.0), 2, one.ctypes.data, one.ctypes.data) == E.E_INVALID
    with pytest.raises(ValueError, match="cycle"):
        lib_tree(cycle, d, 10, 2)


def test_library_queries():
    import sfv_amd as sfv
    q = sfv._lib.query
    assert q("rbvae_version") >= 108
    for N, L, ok in ((2, 1, 1), (16384, 128, 1), (1, 3, 0), (16385, 3, 0), (8, 0, 0), (8, 129, 0)):
        assert q("rbvae_mst_ok", N, L) == ok, (N, L)
    assert q("rbvae_mst_ws_bytes", 2) == 256 and q("rbvae_mst_ws_bytes", 16384) == 128 * 16384 and q("rbvae_mst_ws_bytes", 1) == 0
    assert sfv.density.MAX_MST_ROWS == 16384 and sfv.density.SELECTION_METHODS == ("eom", "leaf")
    for f in (lambda X: sfv.hdbscan(X), lambda X: sfv.core_distances(X, 3), lambda X: sfv.mutual_reachability_mst(X, 3),
              lambda X: sfv.hdbscan_sweep(X, [5], 3)):
        with pytest.raises(ValueError, match="GPU"):
            f(np.zeros((8, 2), dtype=np.float32))
        import torch
        with pytest.raises(ValueError, match="GPU"):
            f(torch.zeros(8, 2))
    with pytest.raises(ValueError, match="min_samples"):
        sfv.hdbscan_sweep(None, [5], None)
