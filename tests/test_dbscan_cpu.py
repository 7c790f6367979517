"""CPU: tests/_dbscan_ref.py, the numpy restatement of csrc/dbscan.hip, against scikit-learn 1.7.2's DBSCAN as recorded in
tests/golden/dbscan.npz (tools/make_dbscan_golden.py) -- labels_ and core_sample_indices_ on every row of every case -- the
conditions that make that comparison meaningful, and the round rule's fixed point.  Everything is exact equality."""
import numpy as np
import pytest

import _dbscan_ref as R

CASES = R.golden_cases()
CONTESTED = np.array([0, .1, .2, .3, .4, 2, 2.1, 2.2, 2.3, 2.4, 1.2, 10.0])


def _properties(X, metric, eps, labels, core_idx):
    A = R.case_adjacency(X, metric, eps)
    core = np.zeros(len(X), dtype=bool)
    core[core_idx] = True
    border = ~core & (labels >= 0)
    contested = [i for i in np.flatnonzero(border) if len(set(labels[np.flatnonzero(A[i] & core)])) > 1]
    return int(border.sum()), contested, int((labels < 0).sum()), int(core.sum())


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_restatement_equals_sklearn(case):
    name, X, metric, eps, m, labels, core_idx = case
    A = R.case_adjacency(X, metric, eps)
    assert A.diagonal().all() and np.array_equal(A, A.T)
    for by_rounds in (False, True):
        got = R.dbscan(A, m, by_rounds=by_rounds)
        assert np.array_equal(got["labels"], labels), f"{name}: labels"
        assert np.array_equal(got["core_sample_indices"], core_idx), f"{name}: core rows"
        assert got["n_clusters"] == int(labels.max()) + 1
    assert got["labels"].dtype == np.int32 and X.dtype == np.float32 and 12 <= len(X) <= 400


def test_fixture_conditions():
    g = R.golden()
    assert str(g["sklearn"]) == "1.7.2"
    strings = [k for k in g.files if g[k].dtype.kind in "US"]
    assert sorted(strings) == ["names", "sklearn"]          # inputs, labels_, core_sample_indices_ and two strings, nothing else
    assert all(k in strings or k.split("/")[1] in ("X", "eps", "bits", "min_samples", "labels", "core_sample_indices") for k in g.files)
    seen = {}
    for name, X, metric, eps, m, labels, core_idx in CASES:
        border, contested, noise, core = _properties(X, metric, eps, labels, core_idx)
        seen[name] = (metric, m, border, contested, noise, core)
        if metric == "euclidean":                           # no pair near eps^2: sklearn's distances cannot disagree with row_d2
            margin = np.abs(R.d2_matrix(X) / (eps * eps) - 1.0).min()
            assert margin > 1e-9, (name, margin)
        else:
            assert set(np.unique(X)) <= {0.0, 1.0} and X.shape[1] == 32
    for metric in ("euclidean", "hamming"):
        assert any(v[0] == metric and v[2] for v in seen.values()), metric + ": no case with border rows"
    assert any(v[3] for v in seen.values()), "no contested border row"
    assert any(v[4] for v in seen.values()), "no noise"
    assert any(v[5] == 0 for v in seen.values()), "no case without a core row"
    assert any(v[1] == 1 for v in seen.values()), "no case with min_samples = 1"
    # the contested case is the construction, permuted
    name, X, metric, eps, m, labels, core_idx = next(c for c in CASES if c[0] == "contested")
    assert np.array_equal(np.sort(X[:, 0]), np.sort(CONTESTED.astype(np.float32))) and (eps, m) == (0.85, 5)
    row = seen["contested"][3]
    assert len(row) == 1 and X[row[0], 0] == np.float32(1.2) and labels[row[0]] == 0


def test_contested_row_takes_the_lower_id_under_every_permutation():
    r = np.random.RandomState(0)
    perms = [np.arange(12), np.arange(12)[::-1]] + [r.permutation(12) for _ in range(200)]
    for perm in perms:
        X = CONTESTED[perm].astype(np.float32)[:, None]
        got = R.dbscan(R.adjacency(X, 0.85 * 0.85), 5, by_rounds=True)
        at = int(np.flatnonzero(perm == 10)[0])
        assert not got["core"][at] and got["labels"][at] == 0 and got["n_clusters"] == 2
        assert got["labels"][int(np.flatnonzero(perm == 11)[0])] == -1
        first = min(int(np.flatnonzero(perm == k)[0]) for k in range(10))       # the first core row decides which blob is 0
        assert got["labels"][first] == 0


@pytest.mark.parametrize("name", sorted(R.GRAPHS))
def test_rounds_reach_the_smallest_core_index(name):
    A, m = R.GRAPHS[name]()
    cnt, core = R.core_rows(A, m)
    fs, n = R.run_rounds(A, core, limit=64)
    want = R.components(A, core)
    assert np.array_equal(fs[-1], want) and n == len(fs)
    befores = [R.start(core)] + fs[:-1]                     # only the last round changes nothing
    assert [np.array_equal(a, b) for a, b in zip(befores, fs)] == [False] * (n - 1) + [True]
    for a, b in zip([R.start(core)] + fs, fs):
        assert (b <= a).all()                               # an entry only ever decreases
    N = len(core)
    assert (want[~core] == N).all() and (want[core] <= np.flatnonzero(core)).all()
    print(f"{name}: {n} rounds, {len(set(want[core]))} components of {int(core.sum())} core rows")
    if name == "no_core":
        assert not core.any() and n == 1
    if name == "isolated":
        assert n == 1 and np.array_equal(want, np.arange(N))
    if name == "interleaved":
        assert set(want) == {0, 1}
    if name in ("path", "path_permuted", "one_cluster"):
        assert (want == 0).all()


def test_packing_and_noise_runs():
    r = np.random.RandomState(2)
    for N in (2, 63, 64, 65, 129):
        A = r.rand(N, N) < 0.3
        P = R.pack_adj(A)
        assert P.shape == (N, R.words(N)) and P.dtype == np.uint64
        back, pad = R.unpack_adj(P, N)
        assert np.array_equal(back, A) and not pad.any()
        for i, j in ((0, 0), (N - 1, N - 1), (1, N - 1)):
            assert bool((int(P[i, j // 64]) >> (j % 64)) & 1) == bool(A[i, j])
    assert R.noise_runs(np.array([-1, -1, 0, 1, -1, 2, -1])) == [(0, 2), (4, 5), (6, 7)]
    assert R.noise_runs(np.array([0, 0])) == [] and R.noise_runs(np.array([-1])) == [(0, 1)]
    X = (r.rand(50, 40) < 0.5).astype(np.float32)
    assert np.array_equal(R.hamming_matrix(X), (X[:, None, :] != X[None, :, :]).sum(-1))
    assert np.array_equal(R.hamming_adjacency(X, 17), R.adjacency(X, 17.0))     # on 0 / 1 the squared distance is the count


def test_library_queries():
    import sfv_amd as sfv
    q = sfv._lib.query
    assert q("rbvae_version") >= 107
    for N, L, ok in ((2, 1, 1), (65536, 128, 1), (1, 3, 0), (65537, 3, 0), (8, 0, 0), (8, 129, 0)):
        assert q("rbvae_dbscan_ok", N, L) == ok, (N, L)
    for N in (1, 2, 63, 64, 65, 4200, 65536):
        assert q("rbvae_dbscan_words", N) == R.words(N)
    assert q("rbvae_dbscan_words", 0) == q("rbvae_dbscan_words", 65537) == 0
    assert q("rbvae_dbscan_ws_bytes", 65) == 32 and q("rbvae_dbscan_ws_bytes", 65536) == 16384 and q("rbvae_dbscan_ws_bytes", 1) == 0
    assert sfv.density.MAX_ROWS == 65536 and sfv.noise_runs(np.array([-1, 0, -1, -1])) == [(0, 1), (2, 4)]
    assert sfv.density.knee(np.array([0.0, 0.0, 0.0, 1.0])) == 2 and sfv.density.knee(np.ones(5)) == 0
    with pytest.raises(ValueError, match="GPU"):
        sfv.dbscan(np.zeros((4, 2), dtype=np.float32), 0.5)
