"""GPU: csrc/dbscan.hip and density.py against tests/_dbscan_ref.py and scikit-learn 1.7.2's DBSCAN (tests/golden/dbscan.npz).
Every output sits inside sentinel guard bands (tests/_bounds.py's GuardedFlat) and every comparison is exact equality: the
distance is rbvae_knn's f64 sum, compared once with eps^2, and everything behind the comparison is integer.

  graph, Euclidean    adj and cnt bit for bit for N in {2, 63, 64, 65, 129, 257, 1000} x L in {1, 3, 32, 33, 100, 128}; eps^2 is one
                      of the matrix's own d2 values, so ties d2 == eps^2 are present and inside; padding bits zero, diagonal set,
                      symmetric, cnt = popcounts; the 6 x 6 lattice's ties
  graph, Hamming      L in {1, 31, 32, 33, 64, 65, 127, 128} x max_bits in {0, 1, L}: the restatement's words and the Euclidean
                      kernel's on the same 0 / 1 matrix at eps^2 = max_bits
  kNN                 cnt[i] >= m  <=>  rbvae_knn's d2[i][m - 2] <= eps^2 on every row
  components          f after every round and the number of rounds on _dbscan_ref.GRAPHS; behind done nothing is written
  labels              the restatement's and the fixture's on every row, through the entries and through density.py; N = 4200
                      (66 words a row) and N = 65536 (all 1024 words of the scan)
  refusals, repeatability, scoring

On the planted chain of test_planted_chain (400 rows, 4 states, 48 transition rows on bent bridges) the noise rows of the Euclidean
fit at eps 0.5 are exactly the 48 transition rows (share within tolerance 0 of a planted transition: 1.0), as the restatement
gives on the CPU; the permuted 1000-row path takes 12 rounds, the time-ordered one 11.
"""
import functools

import numpy as np
import pytest
import torch

import _bounds as B
import _bernoulli_ref as Bn
import _dbscan_ref as R
import sfv_amd as sfv

pytestmark = pytest.mark.gpu

GUARD = 4096
B.SENTINEL.setdefault(torch.int32, (torch.int32, -0x21524111))
B.SENTINEL.setdefault(torch.int64, (torch.int64, 0x6B5FCA6B5FCA6B5F))
call, query = sfv._lib.call, sfv._lib.query
I32, I64 = torch.int32, torch.int64
CASES = R.golden_cases()


def G(dtype, *shape):
    g = B.GuardedFlat(int(np.prod(shape)), dtype, guard=GUARD)
    g.t = g.view.view(*shape)
    return g


def out(g, what):
    B.assert_guards(g, what)
    return g.t.cpu().numpy()


def untouched(g, what):
    B.assert_guards_where(g, torch.zeros(g.rows, dtype=torch.bool), what)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def _state(*v):
    return torch.tensor(list(v) or [0, 0, 0, 0], dtype=I32, device="cuda")


def _adj_dev(A):
    """a neighbourhood matrix as the device's words and counts"""
    return _dev(R.pack_adj(A).view(np.int64)), _dev(A.sum(axis=1).astype(np.int32))


def _graph(X, eps2=None, bits=None, packed=None):
    """-> (adj uint64 [N, W], cnt) of one of the two graph entries, guards checked"""
    N, L = X.shape
    W = query("rbvae_dbscan_words", N)
    assert W == R.words(N)
    adj, cnt = G(I64, N, W), G(I32, N)
    if eps2 is not None:
        call("rbvae_dbscan_adj", _dev(X), N, L, float(eps2), adj.t, cnt.t)
    else:
        call("rbvae_dbscan_adj_bits", _dev((Bn.pack(X) if packed is None else packed).view(np.int32)), N, L, int(bits), adj.t, cnt.t)
    what = f"({N}, {L})"
    return out(adj, "adj " + what).view(np.uint64), out(cnt, "cnt " + what)


def _check_graph(adj, cnt, A, what):
    N = len(A)
    assert np.array_equal(adj, R.pack_adj(A)), what + ": the words"
    got, pad = R.unpack_adj(adj, N)
    assert not pad.any(), what + ": padding bits"
    assert got.diagonal().all() and np.array_equal(got, got.T), what + ": diagonal and symmetry"
    assert np.array_equal(cnt, got.sum(axis=1)) and cnt.dtype == np.int32, what + ": cnt"


# ---- the graph ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", [1, 3, 32, 33, 100, 128])
def test_graph_euclidean(L):
    for N in (2, 63, 64, 65, 129, 257, 1000):
        r = np.random.RandomState(1000 * L + N)
        X = r.randn(N, L).astype(np.float32)
        if N >= 63:
            X[N // 3] = X[N // 2]                           # a pair at distance zero
        D = R.d2_matrix(X)
        off = D[~np.eye(N, dtype=bool)]
        eps2 = float(np.sort(off)[len(off) // 3])           # one of the matrix's own values: a tie, and it is inside
        A = D <= eps2
        assert (D == eps2).sum() >= 2
        adj, cnt = _graph(X, eps2=eps2)
        _check_graph(adj, cnt, A, f"({N}, {L})")
        if N == 257:
            again = _graph(X, eps2=eps2)
            assert np.array_equal(adj, again[0]) and np.array_equal(cnt, again[1]), "two runs differ"
            only_self = _graph(X, eps2=0.0)                 # eps = 0: the row and its exact copies
            _check_graph(*only_self, D <= 0.0, f"({N}, {L}) at 0")
            assert only_self[1].sum() == N + 2
            _check_graph(*_graph(X, eps2=float("inf")), np.ones((N, N), dtype=bool), f"({N}, {L}) at inf")


def test_graph_lattice_ties():
    X = np.array([[i, j] for i in range(6) for j in range(6)], dtype=np.float32)
    for eps2, m, n_core in ((1.0, 5, 16), (1.0, 4, 32), (2.0, 9, 16)):
        adj, cnt = _graph(X, eps2=eps2)
        _check_graph(adj, cnt, R.adjacency(X, eps2), f"lattice at {eps2}")
        mask, f = G(I64, 1), G(I32, 36)
        call("rbvae_dbscan_core", _dev(cnt), 36, m, mask.t, f.t)
        core = R.unpack_adj(out(mask, "core_mask").reshape(1, 1), 36)[0][0]
        assert int(core.sum()) == n_core and np.array_equal(core, cnt >= m)
        assert np.array_equal(out(f, "f"), np.where(core, np.arange(36), 36))
        fit = sfv.dbscan(_dev(X), np.sqrt(eps2), m)         # sqrt(2)^2 rounds to just above 2: the ties stay inside
        ref = R.dbscan(R.adjacency(X, eps2), m)
        assert int(fit.core.sum()) == n_core and fit.n_clusters == 1 and np.array_equal(fit.labels.cpu().numpy(), ref["labels"])
        assert fit.n_noise == (4 if (eps2, m) == (1.0, 5) else 0)      # the corners' neighbours are edge rows, core only at 4


@pytest.mark.parametrize("L", [1, 31, 32, 33, 64, 65, 127, 128])
def test_graph_hamming(L):
    for N in (2, 65, 257):
        r = np.random.RandomState(100 * L + N)
        proto = r.rand(3, L) < 0.5
        X = (proto[r.randint(3, size=N)] ^ (r.rand(N, L) < 1.0 / (L + 1))).astype(np.float32)
        X[N - 1] = X[0]                                     # a pair at distance zero
        packed = Bn.pack(X)
        assert torch.equal(sfv.pack_codes(_dev(X)).cpu(), torch.from_numpy(packed.view(np.int32)))
        H = R.hamming_matrix(X)
        for bits in (0, 1, L):
            adj, cnt = _graph(X, bits=bits, packed=packed)
            _check_graph(adj, cnt, H <= bits, f"({N}, {L}) at {bits} bits")
            e_adj, e_cnt = _graph(X, eps2=float(bits))
            assert np.array_equal(adj, e_adj) and np.array_equal(cnt, e_cnt), "the Euclidean kernel's words on 0 / 1"
        assert (H <= 0).sum() >= N + 2 and (H <= L).all()


def test_counts_agree_with_the_knn_kernel():
    X = np.random.RandomState(4).randn(300, 8).astype(np.float32)
    Xd = _dev(X)
    K1 = 10
    _, d2 = sfv.knn_graph(Xd, K1)
    d2 = d2.cpu().numpy()
    for eps2 in (float(d2[17, 3]), float(np.median(d2[:, 5])), 4.0):     # the first two are distances of the matrix itself
        adj, cnt = _graph(X, eps2=eps2)
        for m in range(2, K1 + 2):
            assert np.array_equal(cnt >= m, d2[:, m - 2] <= eps2), (eps2, m)


# ---- components --------------------------------------------------------------------------------------------------------------

def _core(cnt, N, m):
    W = R.words(N)
    mask, f = G(I64, W), G(I32, N)
    call("rbvae_dbscan_core", _dev(cnt), N, m, mask.t, f.t)
    return out(mask, "core_mask").view(np.uint64), out(f, "f")


def _rounds(adj_d, mask_d, f0, N, limit):
    """-> (f after every round, the states after every round): rounds until done, each into a fresh guarded buffer"""
    state = _state()
    f_in = _dev(f0)
    fs, states = [], []
    while not states or not states[-1][0]:
        assert len(fs) < limit, "the rounds do not settle"
        g = G(I32, N)
        call("rbvae_dbscan_round", adj_d, mask_d, N, f_in, g.t, state)
        fs.append(out(g, f"f_out of round {len(fs) + 1}"))
        states.append(state.cpu().tolist())
        f_in = g.t.clone()
    g = G(I32, N)                                           # behind done: nothing is written
    before = state.clone()
    call("rbvae_dbscan_round", adj_d, mask_d, N, f_in, g.t, state)
    untouched(g, "f_out behind done")
    assert torch.equal(state, before)
    return fs, states


@pytest.mark.parametrize("name", sorted(R.GRAPHS))
def test_components(name):
    A, m = R.GRAPHS[name]()
    N = len(A)
    cnt, core = R.core_rows(A, m)
    adj_d, cnt_d = _adj_dev(A)
    mask, f0 = _core(cnt, N, m)
    assert np.array_equal(mask, R.pack_adj(core[None, :])[0]) and np.array_equal(f0, R.start(core))
    want, n = R.run_rounds(A, core, limit=64)
    fs, states = _rounds(adj_d, _dev(mask.view(np.int64)), f0, N, limit=64)
    print(f"{name}: {len(fs)} rounds on the device, {n} in the restatement")
    assert len(fs) == n
    for r, (a, b) in enumerate(zip(fs, want)):
        assert np.array_equal(a, b), f"{name}: f after round {r + 1}"
    assert states == [[0, r + 1, 1, 0] for r in range(n - 1)] + [[1, n, 0, 0]]
    assert np.array_equal(fs[-1], R.components(A, core))
    labels, nc, ws = G(I32, N), G(I32, 1), torch.empty(query("rbvae_dbscan_ws_bytes", N) // 8, dtype=I64, device="cuda")
    call("rbvae_dbscan_labels", adj_d, _dev(mask.view(np.int64)), _dev(fs[-1]), N, labels.t, nc.t, ws)
    ref = R.dbscan(A, m)
    assert np.array_equal(out(labels, "labels"), ref["labels"]) and int(out(nc, "n_clusters")[0]) == ref["n_clusters"]
    fit = sfv.dbscan(None, 0.0, m, graph=(adj_d, cnt_d))
    assert fit.n_rounds == n and fit.n_clusters == ref["n_clusters"] and np.array_equal(fit.labels.cpu().numpy(), ref["labels"])
    if name == "no_core":
        assert ref["n_clusters"] == 0 and (ref["labels"] == -1).all() and fit.n_noise == N
    if name == "path_permuted":
        assert n == 12                                      # the restatement's count; plain propagation needs 541


# ---- labels ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _reference(name):
    _, X, metric, eps, m, _, _ = next(c for c in CASES if c[0] == name)
    return R.dbscan(R.case_adjacency(X, metric, eps), m, by_rounds=True)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_labels(case):
    name, X, metric, eps, m, sk_labels, sk_core = case
    N, L = X.shape
    ref = _reference(name)
    A = R.case_adjacency(X, metric, eps)
    adj, cnt = _graph(X, eps2=eps * eps) if metric == "euclidean" else _graph(X, bits=eps)
    _check_graph(adj, cnt, A, name)
    mask, f0 = _core(cnt, N, m)
    adj_d, mask_d = _dev(adj.view(np.int64)), _dev(mask.view(np.int64))
    fs, states = _rounds(adj_d, mask_d, f0, N, limit=64)
    assert len(fs) == ref["n_rounds"] and np.array_equal(fs[-1], ref["f"])
    labels, nc, ws = G(I32, N), G(I32, 1), G(I64, 2 * R.words(N))
    call("rbvae_dbscan_labels", adj_d, mask_d, _dev(fs[-1]), N, labels.t, nc.t, ws.t)
    W = R.words(N)                                          # ws: the root mask u64 [W], then int32 [W]; the rest stays untouched
    B.assert_guards_where(ws, torch.arange(2 * W) < W + (W + 1) // 2, "ws " + name)
    lab = out(labels, "labels " + name)
    assert np.array_equal(lab, ref["labels"]) and np.array_equal(lab, sk_labels), name
    assert int(out(nc, "n_clusters")[0]) == ref["n_clusters"] == int(sk_labels.max()) + 1
    # through density.py
    Xd = _dev(X)
    fit = sfv.dbscan(Xd, eps, m, metric=metric)
    assert fit.labels.dtype == I32 and fit.core.dtype == torch.bool and fit.counts.dtype == I32
    assert np.array_equal(fit.labels.cpu().numpy(), sk_labels)
    assert np.array_equal(np.flatnonzero(fit.core.cpu().numpy()), sk_core)
    assert np.array_equal(fit.counts.cpu().numpy(), ref["counts"])
    assert (fit.n_clusters, fit.n_noise, fit.n_rounds) == (ref["n_clusters"], int((sk_labels < 0).sum()), ref["n_rounds"])
    assert (fit.eps, fit.min_samples, fit.metric) == (eps, m, metric)
    assert np.array_equal(fit.graph[0].cpu().numpy().view(np.uint64), adj) and np.array_equal(fit.graph[1].cpu().numpy(), cnt)
    again = sfv.dbscan(Xd, eps, m, metric=metric, graph=fit.graph)
    assert torch.equal(again.labels, fit.labels) and again.n_rounds == fit.n_rounds
    if metric == "hamming":                                 # a packed input equals an unpacked one
        packed = sfv.dbscan(sfv.pack_codes(Xd), eps, m, metric="hamming")
        assert torch.equal(packed.labels, fit.labels) and torch.equal(packed.counts, fit.counts) and torch.equal(packed.core, fit.core)
        assert torch.equal(packed.graph[0], fit.graph[0])
    if name == "contested":
        at = int(np.flatnonzero(X[:, 0] == np.float32(1.2))[0])
        near = np.flatnonzero(A[at] & ref["core"])
        assert not ref["core"][at] and set(lab[near]) == {0, 1} and lab[at] == 0


def test_sweep_equals_separate_fits():
    for name, ms in (("blobs", (1, 3, 5, 9, 400)), ("codes", (1, 2, 5, 30))):
        _, X, metric, eps, _, _, _ = next(c for c in CASES if c[0] == name)
        Xd = _dev(X)
        A = R.case_adjacency(X, metric, eps)
        fits = sfv.dbscan_sweep(Xd, eps, ms, metric=metric)
        assert len(fits) == len(ms) and all(f.graph[0] is fits[0].graph[0] for f in fits)
        for m, fit in zip(ms, fits):
            one, ref = sfv.dbscan(Xd, eps, m, metric=metric), R.dbscan(A, m, by_rounds=True)
            assert torch.equal(fit.labels, one.labels) and torch.equal(fit.core, one.core) and fit.min_samples == m
            assert (fit.n_clusters, fit.n_noise, fit.n_rounds) == (one.n_clusters, one.n_noise, one.n_rounds)
            assert np.array_equal(fit.labels.cpu().numpy(), ref["labels"]) and fit.n_rounds == ref["n_rounds"]


def test_more_than_64_words_a_row():
    """N = 4200: 66 words a row, so a lane of the count, round and label kernels walks more than one word, and 17 row chunks"""
    N, L = 4200, 24
    r = np.random.RandomState(8)
    proto = r.rand(6, L) < 0.5
    X = (proto[r.randint(6, size=N)] ^ (r.rand(N, L) < 0.08)).astype(np.float32)
    X[r.permutation(N)[:200]] = (r.rand(200, L) < 0.5).astype(np.float32)
    assert R.words(N) == 66
    H = R.hamming_matrix(X)
    for bits, m in ((1, 40), (2, 3)):
        A = H <= bits
        adj, cnt = _graph(X, bits=bits)
        _check_graph(adj, cnt, A, f"({N}, {L}) at {bits} bits")
        e_adj, e_cnt = _graph(X, eps2=float(bits))
        assert np.array_equal(adj, e_adj) and np.array_equal(cnt, e_cnt)
        ref = R.dbscan(A, m, by_rounds=True)
        fit = sfv.dbscan(_dev(X), bits, m, metric="hamming")
        print(f"({N}, {L}) at {bits} bits, min_samples {m}: {fit.n_clusters} clusters, {fit.n_noise} noise rows, "
              f"{int(fit.core.sum())} core rows, {fit.n_rounds} rounds")
        assert np.array_equal(fit.labels.cpu().numpy(), ref["labels"]) and np.array_equal(fit.core.cpu().numpy(), ref["core"])
        assert (fit.n_clusters, fit.n_rounds) == (ref["n_clusters"], ref["n_rounds"])
        assert 0 < fit.n_noise < N and 0 < int(fit.core.sum()) < N - fit.n_noise       # border rows exist


def test_largest_shape():
    """N = 65536: all 1024 words of the scan, 256 row chunks, a graph of 512 MB.  The codes are 37 prototypes without flips, so at
    0 bits a row's neighbours are its prototype's rows: the counts, the labels (the prototypes in order of first appearance) and
    sampled rows of the graph follow from the assignment alone."""
    N, L, K = 65536, 16, 37
    r = np.random.RandomState(9)
    proto = np.unique(r.rand(4 * K, L) < 0.5, axis=0)[:K]
    which = r.randint(K, size=N)
    X = proto[which].astype(np.float32)
    assert len(proto) == K and query("rbvae_dbscan_ok", N, L) == 1 and query("rbvae_dbscan_words", N) == 1024
    size = np.bincount(which, minlength=K)
    first = np.array([np.flatnonzero(which == k)[0] for k in range(K)])
    rank = np.empty(K, dtype=np.int64)
    rank[np.argsort(first)] = np.arange(K)
    Xd = _dev(X)
    fit = sfv.dbscan(Xd, 0, 5, metric="hamming")
    assert size.min() >= 5 and fit.n_clusters == K and fit.n_noise == 0 and fit.n_rounds == 2 and bool(fit.core.all())
    assert np.array_equal(fit.counts.cpu().numpy(), size[which]) and np.array_equal(fit.labels.cpu().numpy(), rank[which])
    adj = fit.graph[0]
    for i in (0, 1, 4095, 4096, 32767, N - 1):
        row = R.unpack_adj(adj[i:i + 1].cpu().numpy(), N)[0][0]
        assert np.array_equal(row, which == which[i]), i
    e_adj, e_cnt = sfv.radius_graph(Xd, 0.0)                # the Euclidean kernel at eps 0 on the same 0 / 1 matrix
    assert torch.equal(e_adj, adj) and torch.equal(e_cnt, fit.counts)
    sparse = sfv.dbscan(None, 0, int(size.max()) + 1, graph=fit.graph)
    assert sparse.n_clusters == 0 and sparse.n_noise == N and sparse.n_rounds == 1


# ---- refused arguments -------------------------------------------------------------------------------------------------------

def test_refused_arguments_write_nothing():
    adj, cnt, mask, f, labels, nc, ws = G(I64, 4096), G(I32, 4096), G(I64, 4096), G(I32, 4096), G(I32, 4096), G(I32, 1), G(I64, 4096)
    X = torch.zeros((300, 129), dtype=torch.float32, device="cuda")
    words = torch.zeros((300, 4), dtype=I32, device="cuda")
    a_in, m_in = torch.zeros(4096, dtype=I64, device="cuda"), torch.zeros(4096, dtype=I64, device="cuda")
    c_in, f_in, state = torch.zeros(4096, dtype=I32, device="cuda"), torch.zeros(4096, dtype=I32, device="cuda"), _state()
    for N, L, match in ((1, 3, "N=1"), (65537, 3, "N=65537"), (8, 129, "L=129"), (8, 0, "L=0")):
        assert query("rbvae_dbscan_ok", N, L) == 0
        with pytest.raises(RuntimeError, match=match):
            call("rbvae_dbscan_adj", X, N, L, 1.0, adj.t, cnt.t)
        with pytest.raises(RuntimeError, match=match):
            call("rbvae_dbscan_adj_bits", words, N, L, 0, adj.t, cnt.t)
        if L == 3:
            assert query("rbvae_dbscan_ws_bytes", N) == 0
            with pytest.raises(RuntimeError, match=match):
                call("rbvae_dbscan_core", c_in, N, 2, mask.t, f.t)
            with pytest.raises(RuntimeError, match=match):
                call("rbvae_dbscan_round", a_in, m_in, N, f_in, f.t, state)
            with pytest.raises(RuntimeError, match=match):
                call("rbvae_dbscan_labels", a_in, m_in, f_in, N, labels.t, nc.t, ws.t)
    assert query("rbvae_dbscan_ok", 2, 1) == query("rbvae_dbscan_ok", 65536, 128) == 1
    assert query("rbvae_dbscan_words", 64) == 1 and query("rbvae_dbscan_words", 65) == 2 and query("rbvae_dbscan_words", 65536) == 1024
    assert query("rbvae_dbscan_ws_bytes", 65) == 32
    for eps2 in (-1.0, float("nan"), -0.5):
        with pytest.raises(ValueError, match="eps2"):
            call("rbvae_dbscan_adj", X, 8, 3, eps2, adj.t, cnt.t)
    for bits in (-1, 4):
        with pytest.raises(ValueError, match="max_bits"):
            call("rbvae_dbscan_adj_bits", words, 8, 3, bits, adj.t, cnt.t)
    for m in (0, -3):
        with pytest.raises(ValueError, match="min_samples"):
            call("rbvae_dbscan_core", c_in, 8, m, mask.t, f.t)
    with pytest.raises(ValueError, match="same buffer"):
        call("rbvae_dbscan_round", a_in, m_in, 8, f.t, f.t, state)
    for args in ((None, 8, 3, 1.0, adj.t, cnt.t), (X, 8, 3, 1.0, None, cnt.t), (X, 8, 3, 1.0, adj.t, None)):
        with pytest.raises(ValueError, match="null"):
            call("rbvae_dbscan_adj", *args)
    for args in ((None, 8, 3, 1, adj.t, cnt.t), (words, 8, 3, 1, None, cnt.t), (words, 8, 3, 1, adj.t, None)):
        with pytest.raises(ValueError, match="null"):
            call("rbvae_dbscan_adj_bits", *args)
    for args in ((None, 8, 2, mask.t, f.t), (c_in, 8, 2, None, f.t), (c_in, 8, 2, mask.t, None)):
        with pytest.raises(ValueError, match="null"):
            call("rbvae_dbscan_core", *args)
    for args in ((None, m_in, 8, f_in, f.t, state), (a_in, None, 8, f_in, f.t, state), (a_in, m_in, 8, None, f.t, state),
                 (a_in, m_in, 8, f_in, None, state), (a_in, m_in, 8, f_in, f.t, None)):
        with pytest.raises(ValueError, match="null"):
            call("rbvae_dbscan_round", *args)
    for args in ((None, m_in, f_in, 8, labels.t, nc.t, ws.t), (a_in, m_in, f_in, 8, None, nc.t, ws.t), (a_in, m_in, f_in, 8, labels.t, None, ws.t),
                 (a_in, m_in, f_in, 8, labels.t, nc.t, None)):
        with pytest.raises(ValueError, match="null"):
            call("rbvae_dbscan_labels", *args)
    for g, n in ((adj, "adj"), (cnt, "cnt"), (mask, "core_mask"), (f, "f"), (labels, "labels"), (nc, "n_clusters"), (ws, "ws")):
        untouched(g, n)
    assert state.cpu().tolist() == [0, 0, 0, 0]
    ok = torch.rand(8, 3, generator=torch.Generator().manual_seed(0)).cuda()
    bad, inf = ok.clone(), ok.clone()
    bad[2, 1], inf[0, 0] = float("nan"), float("inf")
    graph = sfv.radius_graph(ok, 0.5)
    for fn, match in ((lambda: sfv.dbscan(ok.cpu(), 0.5), "GPU"), (lambda: sfv.radius_graph(ok.cpu(), 0.5), "GPU"),
                      (lambda: sfv.dbscan(bad, 0.5), "NaN"), (lambda: sfv.dbscan(inf, 0.5, metric="hamming"), "NaN or infinite"),
                      (lambda: sfv.dbscan(ok.double(), 0.5), "float32"), (lambda: sfv.dbscan(ok, -0.5), "eps"),
                      (lambda: sfv.dbscan(ok, float("nan")), "eps"), (lambda: sfv.dbscan(ok, 0.5, min_samples=0), "min_samples"),
                      (lambda: sfv.dbscan(ok, 0.5, min_samples=2.5), "min_samples"), (lambda: sfv.dbscan(ok, 0.5, metric="cosine"), "metric"),
                      (lambda: sfv.dbscan(ok, 1.5, metric="hamming"), "whole number"), (lambda: sfv.dbscan(ok, 4, metric="hamming"), r"\[0, L = 3\]"),
                      (lambda: sfv.dbscan(ok[:1].contiguous(), 0.5), "N=1"), (lambda: sfv.dbscan(ok[:4].contiguous(), 0.5, graph=graph), "rows"),
                      (lambda: sfv.dbscan(ok, 0.5, graph=(graph[0].cpu(), graph[1])), "graph"),
                      (lambda: sfv.dbscan_sweep(ok, 0.5, [2, 0]), "min_samples"), (lambda: sfv.k_distances(ok, 0), "k"),
                      (lambda: sfv.k_distances(ok, 9), "k=9"), (lambda: sfv.k_distances(ok.cpu(), 2), "GPU"), (lambda: sfv.suggest_eps(bad, 2), "NaN"),
                      (lambda: sfv.latent_density(None, torch.zeros((2, 3, 8, 8), device="cuda"), [0], [1]), "frame indices")):
        with pytest.raises(ValueError, match=match):
            fn()


# ---- repeatability and scoring ----------------------------------------------------------------------------------------------

CHAIN = dict(N=400, L=8, K=4, seed=7)


def test_planted_chain():
    """Two whole fits agree bit for bit; the noise rows of the fit at eps 0.5, min_samples 5 are the planted transition rows:
    measured (and given by the restatement on the CPU) 48 of 48 noise rows are transition rows and none of the 352 others is
    noise, in 4 clusters after 2 rounds.  The numbers are printed, the equality with the restatement is what is asserted."""
    X, s, tr = R.planted_chain(**CHAIN)
    N = len(X)
    Xd = _dev(X)
    ref = R.dbscan(R.adjacency(X, 0.25), 5, by_rounds=True)
    a, b = sfv.dbscan(Xd, 0.5), sfv.dbscan(Xd, 0.5)
    assert torch.equal(a.labels, b.labels) and torch.equal(a.counts, b.counts) and torch.equal(a.core, b.core)
    assert torch.equal(a.graph[0], b.graph[0]) and (a.n_rounds, a.n_clusters, a.n_noise) == (b.n_rounds, b.n_clusters, b.n_noise)
    lab = a.labels.cpu().numpy()
    assert np.array_equal(lab, ref["labels"]) and a.n_rounds == ref["n_rounds"] and a.n_clusters == ref["n_clusters"]
    noise = lab < 0
    print(f"planted chain: {a.n_clusters} clusters, {a.n_rounds} rounds, {int(noise.sum())} noise rows, {int((noise & tr).sum())} of them among "
          f"the {int(tr.sum())} transition rows, {int((noise & ~tr).sum())} elsewhere")
    runs = sfv.noise_runs(a.labels)
    assert runs == R.noise_runs(lab) == sfv.noise_runs(lab) and sum(e - b for b, e in runs) == a.n_noise
    assert all(lab[b:e].tolist() == [-1] * (e - b) and (b == 0 or lab[b - 1] >= 0) and (e == N or lab[e] >= 0) for b, e in runs)
    assert sfv.noise_runs(np.array([0, 1])) == [] and sfv.noise_runs(np.array([-1, 0, -1, -1])) == [(0, 1), (2, 4)]
    # the k-distance curve is the sorted (k - 1)-th column of the kNN graph
    for k in (2, 5):
        want = torch.sort(torch.sqrt(sfv.knn_graph(Xd, k - 1)[1][:, k - 2])).values
        got = sfv.k_distances(Xd, k)
        assert got.dtype == torch.float64 and torch.equal(got, want) and bool((got[1:] >= got[:-1]).all())
    assert torch.equal(sfv.k_distances(Xd, 1), torch.zeros(N, dtype=torch.float64, device="cuda"))
    curve = sfv.k_distances(Xd, 5).cpu().numpy()
    eps = sfv.suggest_eps(Xd, 5)
    at = sfv.density.knee(curve)
    assert eps == curve[at] and 0 < at < N - 1 and curve[0] < eps < curve[-1]
    assert sfv.density.knee(np.array([0.0, 0.0, 0.0, 1.0])) == 2 and sfv.density.knee(np.ones(5)) == 0
    print(f"suggest_eps(k = 5) = {eps:.4f} at position {at} of {N}")


def test_latent_density_agrees_with_its_parts():
    X, s, tr = R.planted_chain(**CHAIN)
    F_, RES, LD = len(X), 64, 16
    torch.manual_seed(0)
    model = sfv.Seq2SeqBinaryVAE(3, 3, LD, LD, variant="contrastive", input_hw=(RES, RES), compute_dtype="f32").cuda().eval()
    x = torch.rand(F_, 3, RES, RES, generator=torch.Generator().manual_seed(1)).cuda()
    u = torch.rand(F_, LD, generator=torch.Generator().manual_seed(2))
    cps = [t for t in range(1, F_) if s[t] != s[t - 1]]
    flags = cps                                             # frame f carries index f: the state changes at the flags
    res = sfv.latent_density(model, x, range(F_), flags, eps=0.5, projections={"latents": _dev(X)}, u=u)
    assert set(res) == {"latents", "codes", "labels", "eps", "code_bits", "soft", "hard"} and not model.training
    assert res["eps"] == 0.5 and res["code_bits"] == 1 and torch.equal(res["latents"], _dev(X))
    states = res["labels"]
    assert [t for t in range(1, F_) if states[t] != states[t - 1]] == cps
    S = len(flags) + 1
    for key, fit in (("soft", sfv.dbscan(_dev(X), 0.5)), ("hard", sfv.dbscan(res["codes"], 1, metric="hamming"))):
        part = res[key]
        assert set(part) == {"fit", "agreement", "noise_fraction", "noise_near_change", "noise_runs", "boundaries"}
        assert torch.equal(part["fit"].labels, fit.labels) and part["fit"].n_rounds == fit.n_rounds
        lab = fit.labels.cpu().numpy()
        keep = lab >= 0
        assert part["noise_fraction"] == (~keep).sum() / F_ and part["noise_runs"] == sfv.noise_runs(lab)
        if keep.any():
            ref = sfv.clustering_agreement(states[keep], lab[keep].astype(np.int64), S, max(fit.n_clusters, 1))
            assert all(part["agreement"][n] == ref[n] for n in ("ari", "nmi", "v_measure", "fowlkes_mallows"))
        else:
            assert part["agreement"] is None
        noise = np.flatnonzero(~keep)
        if len(noise):
            near = sum(1 for t in noise if min(abs(t - c) for c in cps) <= 2)
            assert part["noise_near_change"] == near / len(noise)
        mids = [(b + e) // 2 for b, e in sfv.noise_runs(lab)]
        want = sfv.boundary_agreement(mids, cps, 2)         # mean_abs_offset is NaN when nothing matches
        assert set(part["boundaries"]) == set(want)
        assert all(np.array_equal(part["boundaries"][n], want[n], equal_nan=True) for n in want)
    soft = res["soft"]
    print(f"latent_density on the planted chain: noise fraction {soft['noise_fraction']:.3f}, share of noise within 2 of a change "
          f"{soft['noise_near_change']:.3f}, boundaries of the noise runs' midpoints {soft['boundaries']}")
    auto = sfv.latent_density(model, x, range(F_), flags, projections={"latents": _dev(X)}, u=u, code_bits=2, min_samples=4)
    assert auto["eps"] == sfv.suggest_eps(_dev(X), 4) and auto["code_bits"] == 2 and auto["soft"]["fit"].min_samples == 4
