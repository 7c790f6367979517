"""GPU: csrc/hdbscan.hip and density.py's HDBSCAN* against tests/_hdbscan_ref.py and, through tests/golden/hdbscan.npz, against
scikit-learn 1.7.2 wherever its answer is well defined.  Every device output sits inside sentinel guard bands (tests/_bounds.py's
GuardedFlat), a refused call leaves them untouched, and every comparison is exact equality: the distance is rbvae_knn's f64 sum,
the key (w2, lo, hi) is a strict total order, and everything behind the comparisons is integer.

  tree                the edge set, the weights and the order against the restatement's Kruskal under the same key, for
                      N in {2, 3, 63, 64, 65, 257, 1000} x L in {1, 3, 50, 128} x m in {1, 2, 5, 129 where N allows}; an integer
                      lattice in L = 2 (every distance ties: the order decides everything), duplicated rows, the planted chain
  many rounds         N = 1024 on a line whose gaps make the components pair up; n_rounds <= ceil(log2 N) + 1
  largest shape       N = 16384 on a line with strictly increasing gaps: the consecutive pairs, in closed form; one round, whose
                      hooks form one chain N deep
  core distances      k_distances' unsorted column bit for bit
  DBSCAN              the core rows are core_d <= eps and the tree's edges with d <= eps part them as dbscan(X, eps, m) does
  whole fits          labels, probabilities and the cluster table of every fixture case equal the restatement bit for bit, and so
                      scikit-learn on the cases marked `agrees`; a row permutation; sweep, cut, latent_hdbscan, two runs, refusals
"""
import functools

import numpy as np
import pytest
import torch

import _bounds as B
import _dbscan_ref as D
import _hdbscan_ref as R
import sfv_amd as sfv

pytestmark = pytest.mark.gpu

GUARD = 4096
B.SENTINEL.setdefault(torch.int32, (torch.int32, -0x21524111))
B.SENTINEL.setdefault(torch.int64, (torch.int64, 0x6B5FCA6B5FCA6B5F))
B.SENTINEL.setdefault(torch.float64, (torch.int64, 0x7FF8DEADDEADBEEF))
call, query = sfv._lib.call, sfv._lib.query
I32, I64, F64 = torch.int32, torch.int64, torch.float64
CASES = R.golden_cases()
IDS = [c["name"] for c in CASES]


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


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def rounds_bound(N):
    return (N - 1).bit_length() + 1


def device_mst(X, c2):
    """the entries themselves on guarded buffers -> (edges, w2 sorted by the key on the host, n_rounds)"""
    N, L = X.shape
    comp, edges, w2, state = G(I32, N), G(I32, N - 1, 2), G(F64, N - 1), G(I32, 4)
    ws = G(I64, query("rbvae_mst_ws_bytes", N) // 8)
    Xd, cd = _dev(X), _dev(c2)
    call("rbvae_mst_start", N, comp.t, state.t, ws.t)
    assert out(state, "state")[:3].tolist() == [0, 0, N] and np.array_equal(out(comp, "comp"), np.arange(N))
    call("rbvae_mst_search", Xd, cd, N, L, comp.t, edges.t, w2.t, state.t, ws.t)      # the search alone writes only into ws
    untouched(edges, "edges after the search alone")
    untouched(w2, "w2 after the search alone")
    assert out(state, "state")[:3].tolist() == [0, 0, N] and np.array_equal(out(comp, "comp"), np.arange(N))
    for it in range(rounds_bound(N) + 1):
        call("rbvae_mst_round", Xd, cd, N, L, comp.t, edges.t, w2.t, state.t, ws.t)
    what = f"({N}, {L})"
    done, n_rounds, n_comp, n_edges = out(state, "state " + what).tolist()
    assert (done, n_comp, n_edges) == (1, 1, N - 1) and n_rounds <= rounds_bound(N), (what, done, n_rounds, n_comp, n_edges)
    assert (out(comp, "comp " + what) == 0).all()
    B.assert_guards_where(ws, (ws.view != B.SENTINEL[I64][1]).cpu(), "ws " + what)      # nothing around the workspace
    e, w = out(edges, "edges " + what), out(w2, "w2 " + what)
    order = np.lexsort((e[:, 1], e[:, 0], w))
    return e[order], w[order], n_rounds


def check_tree(X, m, what, D2=None, api=False):
    N = len(X)
    D2 = D.d2_matrix(X) if D2 is None else D2
    c2 = R.core2(D2, m)
    want_e, want_w = R.mst(R.mutual_reachability2(D2, c2))
    e, w, n_rounds = device_mst(X, c2)
    assert (e[:, 0] < e[:, 1]).all(), what
    assert np.array_equal(e, want_e) and np.array_equal(bits(w), bits(want_w)), what
    if api:
        fit = sfv.mutual_reachability_mst(_dev(X), m)
        edges, d = fit
        assert np.array_equal(edges.cpu().numpy(), want_e) and np.array_equal(bits(fit.w2.cpu().numpy()), bits(want_w)), what
        assert np.array_equal(bits(d.cpu().numpy()), bits(np.sqrt(want_w))) and fit.n_rounds == n_rounds, what
        assert np.array_equal(bits(fit.core_distances.cpu().numpy()), bits(np.sqrt(c2))), what
    return n_rounds


# ---- the tree ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", [1, 3, 50, 128])
def test_tree_against_kruskal(L):
    for N in (2, 3, 63, 64, 65, 257, 1000):
        X = np.random.RandomState(1000 * L + N).randn(N, L).astype(np.float32)
        D2 = D.d2_matrix(X)
        for m in (1, 2, 5, 129):
            if m <= N:
                check_tree(X, m, f"({N}, {L}, m={m})", D2, api=N in (3, 257))


def test_tree_lattice_duplicates_and_chain():
    lattice = np.array([[i, j] for i in range(12) for j in range(12)], dtype=np.float32)
    for m in (1, 2, 5, 9):
        check_tree(lattice, m, f"lattice, m={m}", api=m == 5)
    perm = np.random.RandomState(4).permutation(144)
    check_tree(lattice[perm], 1, "lattice, permuted")
    r = np.random.RandomState(9)
    dup = r.randn(200, 3).astype(np.float32)
    dup[50:120] = dup[r.randint(0, 50, size=70)]            # seventy copies among fifty rows
    for m in (1, 3, 8):
        check_tree(dup, m, f"duplicates, m={m}", api=m == 3)
    same = np.ones((70, 5), dtype=np.float32)               # every row the same: every weight zero
    check_tree(same, 4, "one point", api=True)
    chain, _, _ = D.planted_chain(N=400, L=8, K=4, seed=7)
    for m in (1, 5):
        check_tree(chain, m, f"planted chain, m={m}", api=True)


def test_many_rounds():
    N = 1024
    X = R.pairing_gaps(N)
    n_rounds = check_tree(X, 1, "pairing gaps", api=True)
    assert 2 <= n_rounds <= rounds_bound(N)
    print(f"pairing gaps, N = {N}: {n_rounds} rounds")


def test_largest_shape():
    N = 16384
    X, want_e, want_w = R.increasing_gaps(N)
    e, w, n_rounds = device_mst(X, np.zeros(N))
    assert np.array_equal(e, want_e) and np.array_equal(bits(w), bits(want_w)) and n_rounds <= rounds_bound(N)
    fit = sfv.mutual_reachability_mst(_dev(X), 1)
    assert np.array_equal(fit.edges.cpu().numpy(), want_e) and np.array_equal(bits(fit.w2.cpu().numpy()), bits(want_w))
    assert fit.n_rounds == n_rounds
    print(f"increasing gaps, N = {N}: {n_rounds} rounds")


def test_core_distances_are_k_distances_unsorted():
    X = _dev(R.blobs(300, 8, 4, 2))
    D2 = D.d2_matrix(X.cpu().numpy())
    for m in (1, 2, 5, 129):
        c = sfv.core_distances(X, m)
        assert c.dtype == F64 and np.array_equal(bits(c.cpu().numpy()), bits(np.sqrt(R.core2(D2, m))))
        assert torch.equal(torch.sort(c).values, sfv.k_distances(X, m))
        if m > 1:
            assert torch.equal(c, torch.sqrt(sfv.knn_graph(X, m - 1)[1][:, m - 2]))


def test_against_dbscan():
    """DBSCAN* at eps is DBSCAN's core rows and their partition (its border rows are what the star drops)"""
    X = R.blobs(300, 8, 4, 5)
    Xd = _dev(X)
    for m in (1, 3, 5):
        mst = sfv.mutual_reachability_mst(Xd, m)
        e, d = mst.edges.cpu().numpy(), mst.d.cpu().numpy()
        core_d = mst.core_distances.cpu().numpy()
        levels = np.unique(d)
        for q in (0.3, 0.6, 0.9):
            k = int(q * (len(levels) - 1))
            eps = 0.5 * (levels[k] + levels[k + 1])
            assert np.abs(np.sqrt(D.d2_matrix(X)) / eps - 1.0).min() > 1e-12      # no pair within rounding of the radius
            fit = sfv.dbscan(Xd, eps, m)
            core = fit.core.cpu().numpy()
            assert np.array_equal(core, core_d <= eps), (m, eps)
            f = list(range(len(X)))
            for (a, b), w in zip(e, d):
                if w <= eps:
                    f[R._find(f, int(a))] = R._find(f, int(b))
            mine = np.array([R._find(f, i) for i in range(len(X))])
            assert R.same_partition(mine[core], fit.labels.cpu().numpy()[core]), (m, eps)
            labels, n = sfv.hdbscan_cut(mst, eps, 2)
            keep = core & (labels.cpu().numpy() >= 0)
            assert R.same_partition(labels.cpu().numpy()[keep], fit.labels.cpu().numpy()[keep])


# ---- whole fits --------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def ref_fit(name, method="eom"):
    c = next(c for c in CASES if c["name"] == name)
    return R.hdbscan(c["X"], c["mcs"], c["m"], method)


def as_fit(fit):
    return {"labels": fit.labels.cpu().numpy(), "prob": fit.probabilities.cpu().numpy(), "table": fit.clusters,
            "n_clusters": fit.n_clusters}


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_whole_fit(case):
    want = ref_fit(case["name"])
    fit = sfv.hdbscan(_dev(case["X"]), case["mcs"], case["m"])
    got = as_fit(fit)
    assert np.array_equal(fit.mst.edges.cpu().numpy(), want["edges"]) and np.array_equal(bits(fit.mst.d.cpu().numpy()), bits(want["d"]))
    assert R.same_fit(got, want) and fit.n_clusters == want["n_clusters"] == case["n_clusters"]
    assert fit.n_noise == int((want["labels"] < 0).sum()) and fit.labels.dtype == I32 and fit.probabilities.dtype == F64
    assert (fit.min_cluster_size, fit.min_samples, fit.cluster_selection_method) == (case["mcs"], case["m"], "eom")
    assert np.array_equal(bits(fit.core_distances.cpu().numpy()), bits(np.sqrt(want["core2"])))
    if case["agrees"]:
        assert R.same_partition(got["labels"], case["labels"]) and np.array_equal(bits(got["prob"]), bits(case["prob"]))
    leaf = sfv.hdbscan(None, case["mcs"], cluster_selection_method="leaf", mst=fit.mst)
    assert R.same_fit(as_fit(leaf), ref_fit(case["name"], "leaf"))
    for cut_distance, sk in case["cuts"]:
        labels, n = sfv.hdbscan_cut(fit, cut_distance, case["mcs"])
        ref_labels, ref_n = R.cut(want["edges"], want["d"], len(case["X"]), cut_distance, case["mcs"])
        assert np.array_equal(labels.cpu().numpy(), ref_labels) and n == ref_n and R.same_partition(ref_labels, sk)
    if case["m"] == case["mcs"]:
        assert R.same_fit(as_fit(sfv.hdbscan(_dev(case["X"]), case["mcs"])), want)        # min_samples defaults to it


def test_row_permutation():
    case = next(c for c in CASES if not c["agrees"])
    X = case["X"]
    perm = np.random.RandomState(6).permutation(len(X))
    a = sfv.hdbscan(_dev(X), case["mcs"], case["m"])
    b = sfv.hdbscan(_dev(X[perm]), case["mcs"], case["m"])
    la, lb = a.labels.cpu().numpy(), b.labels.cpu().numpy()
    assert R.same_partition(lb, la[perm]) and a.n_clusters == b.n_clusters
    assert np.array_equal(bits(b.probabilities.cpu().numpy()), bits(a.probabilities.cpu().numpy()[perm]))
    assert np.array_equal(bits(a.mst.d.cpu().numpy()), bits(b.mst.d.cpu().numpy()))


def test_sweep_cut_and_two_runs():
    case = next(c for c in CASES if c["name"] == "m5_a")
    Xd = _dev(case["X"])
    sizes = [5, 15, 40, 300]
    sweep = sfv.hdbscan_sweep(Xd, sizes, 5)
    for mcs, got in zip(sizes, sweep):
        alone = sfv.hdbscan(Xd, mcs, 5)
        assert R.same_fit(as_fit(got), as_fit(alone)) and got.min_cluster_size == mcs and got.n_rounds == alone.n_rounds
        assert torch.equal(got.mst.edges, alone.mst.edges) and torch.equal(got.mst.w2, alone.mst.w2)      # two runs, bit for bit
        assert R.same_fit(as_fit(got), R.hdbscan(case["X"], mcs, 5))
    assert sweep[-1].n_clusters == 0 and sweep[-1].n_noise == 300
    a, b = sfv.mutual_reachability_mst(Xd, 5), sfv.mutual_reachability_mst(Xd, 5)
    assert torch.equal(a.edges, b.edges) and torch.equal(a.d, b.d) and a.n_rounds == b.n_rounds
    d = a.d.cpu().numpy()
    for cut_distance in (0.0, float(d[100]), float(d[-1]), 1e9):
        labels, n = sfv.hdbscan_cut(a, cut_distance, 7)
        ref_labels, ref_n = R.cut(a.edges.cpu().numpy(), d, 300, cut_distance, 7)
        assert np.array_equal(labels.cpu().numpy(), ref_labels) and n == ref_n and labels.is_cuda
    assert sfv.hdbscan_cut(a, 1e9, 7)[1] == 1 and sfv.hdbscan_cut(a, 0.0, 7)[1] == 0


def test_latent_hdbscan_agrees_with_its_parts():
    X, s, tr = D.planted_chain(N=400, L=8, K=4, seed=7)
    F_ = len(X)
    x = torch.zeros(F_, 1, 1, 1, device="cuda")             # the latents are given: the frames only say how many there are
    cps = [t for t in range(1, F_) if s[t] != s[t - 1]]
    res = sfv.latent_hdbscan(None, x, range(F_), cps, min_cluster_size=10, min_samples=5, projections={"latents": _dev(X)})
    assert set(res) == {"latents", "labels", "fit", "agreement", "noise_fraction", "noise_near_change", "noise_runs", "boundaries"}
    fit = sfv.hdbscan(_dev(X), 10, 5)
    assert R.same_fit(as_fit(res["fit"]), as_fit(fit)) and R.same_fit(as_fit(fit), R.hdbscan(X, 10, 5))
    states, lab = res["labels"], fit.labels.cpu().numpy()
    assert [t for t in range(1, F_) if states[t] != states[t - 1]] == cps
    keep = lab >= 0
    assert res["noise_fraction"] == (~keep).sum() / F_ and res["noise_runs"] == sfv.noise_runs(lab)
    ref = sfv.clustering_agreement(states[keep], lab[keep].astype(np.int64), len(cps) + 1, max(fit.n_clusters, 1))
    assert all(res["agreement"][n] == ref[n] for n in ("ari", "nmi", "v_measure", "fowlkes_mallows"))
    want = sfv.boundary_agreement([(b + e) // 2 for b, e in sfv.noise_runs(lab)], cps, 2)
    assert all(np.array_equal(res["boundaries"][n], want[n], equal_nan=True) for n in want)
    p = fit.probabilities.cpu().numpy()
    print(f"latent_hdbscan on the planted chain: {fit.n_clusters} clusters, {fit.n_noise} noise rows, mean membership strength "
          f"{p[tr].mean():.3f} on the {int(tr.sum())} transition rows and {p[~tr].mean():.3f} elsewhere, {fit.n_rounds} rounds")


def test_refused_arguments_write_nothing():
    N = 300
    comp, edges, w2, state, ws = G(I32, N), G(I32, N - 1, 2), G(F64, N - 1), G(I32, 4), G(I64, 16 * N)
    X = torch.zeros((N, 129), dtype=torch.float32, device="cuda")
    c2 = torch.zeros(N + 1, dtype=F64, device="cuda")
    for n, L, match in ((1, 3, "N=1"), (16385, 3, "N=16385"), (8, 129, "L=129"), (8, 0, "L=0")):
        assert query("rbvae_mst_ok", n, L) == 0
        with pytest.raises(RuntimeError, match=match):
            call("rbvae_mst_round", X, c2, n, L, comp.t, edges.t, w2.t, state.t, ws.t)
        if L == 3:
            assert query("rbvae_mst_ws_bytes", n) == 0
            with pytest.raises(RuntimeError, match=match):
                call("rbvae_mst_start", n, comp.t, state.t, ws.t)
    ok = (X, c2, N, 3, comp.t, edges.t, w2.t, state.t, ws.t)
    for k in (0, 1, 4, 5, 6, 7, 8):
        with pytest.raises(ValueError, match="null"):
            call("rbvae_mst_round", *[None if q == k else a for q, a in enumerate(ok)])
    for args in ((N, None, state.t, ws.t), (N, comp.t, None, ws.t), (N, comp.t, state.t, None)):
        with pytest.raises(ValueError, match="null"):
            call("rbvae_mst_start", *args)
    half = ws.t.view(I32)[1:]                               # 4 bytes past an 8-byte boundary
    for k, bad in ((1, c2.view(I32)[1:]), (6, w2.t.view(I32)[1:]), (8, half)):
        with pytest.raises(ValueError, match="aligned"):
            call("rbvae_mst_round", *[bad if q == k else a for q, a in enumerate(ok)])
    with pytest.raises(ValueError, match="aligned"):
        call("rbvae_mst_start", N, comp.t, state.t, half)
    for k, other in ((5, comp.t), (7, comp.t), (8, w2.t), (4, X), (6, c2[1:]), (5, ws.t)):      # two buffers that overlap
        with pytest.raises(ValueError, match="overlap"):
            call("rbvae_mst_round", *[other if q == k else a for q, a in enumerate(ok)])
    with pytest.raises(ValueError, match="overlap"):
        call("rbvae_mst_start", N, ws.t, state.t, ws.t)
    for g, n in ((comp, "comp"), (edges, "edges"), (w2, "w2"), (state, "state"), (ws, "ws")):
        untouched(g, n)
    ok_X = torch.rand(40, 3, generator=torch.Generator().manual_seed(0)).cuda()
    bad, inf = ok_X.clone(), ok_X.clone()
    bad[2, 1], inf[0, 0] = float("nan"), float("inf")
    mst = sfv.mutual_reachability_mst(ok_X, 3)
    for fn, match in ((lambda: sfv.hdbscan(ok_X.cpu()), "GPU"), (lambda: sfv.hdbscan(bad), "NaN"), (lambda: sfv.hdbscan(inf), "NaN or infinite"),
                      (lambda: sfv.hdbscan(ok_X.double()), "float32"), (lambda: sfv.hdbscan(ok_X[:1].contiguous()), "N=1"),
                      (lambda: sfv.hdbscan(ok_X, 1), "min_cluster_size"), (lambda: sfv.hdbscan(ok_X, 41), "min_cluster_size"),
                      (lambda: sfv.hdbscan(ok_X, 2.5, 3), "min_cluster_size"), (lambda: sfv.hdbscan(ok_X, 5, 0), "min_samples"),
                      (lambda: sfv.hdbscan(ok_X, 5, 41), "min_samples"), (lambda: sfv.core_distances(ok_X, 41), "min_samples"),
                      (lambda: sfv.hdbscan(ok_X, 5, cluster_selection_method="mass"), "cluster_selection_method"),
                      (lambda: sfv.hdbscan(ok_X, 5, 4, mst=mst), "min_samples = 3"), (lambda: sfv.hdbscan(ok_X[:9].contiguous(), 5, mst=mst), "rows"),
                      (lambda: sfv.hdbscan(ok_X, 5, mst=(mst.edges, mst.d)), "mst must be"),
                      (lambda: sfv.hdbscan_sweep(ok_X, [5], None), "min_samples"), (lambda: sfv.hdbscan_sweep(ok_X, [5, 1], 3), "min_cluster_size"),
                      (lambda: sfv.hdbscan_cut(mst, -1.0), "cut_distance"), (lambda: sfv.hdbscan_cut(mst, float("nan")), "cut_distance"),
                      (lambda: sfv.hdbscan_cut(mst, 1.0, 1), "min_cluster_size"), (lambda: sfv.hdbscan_cut(None, 1.0), "mst must be"),
                      (lambda: sfv.latent_hdbscan(None, torch.zeros((2, 3, 8, 8), device="cuda"), [0], [1]), "frame indices")):
        with pytest.raises(ValueError, match=match):
            fn()
    big = torch.zeros((16385, 1), device="cuda")
    with pytest.raises(ValueError, match="N=16385"):
        sfv.hdbscan(big)
