"""CPU: tests/_umap_ref.py's restatement of UMAP pinned by properties that do not depend on this project's code (the
published curve parameters, the bisection's own target, the dense fuzzy union, the closed form of the edge schedule), the
host halves of projection.py against it, and each named defect rejected by the bound or equality the GPU tests use."""
import os

import numpy as np
import pytest
import torch

import _projection_ref as P
import _umap_ref as R
import sfv_amd as sfv

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def X():
    return np.load(os.path.join(GOLDEN, "projection.npz"))["X"]


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "umap.npz")))


@pytest.fixture(scope="module")
def layout(gold):
    """the fixture's schedule and its state before epoch 37, maps of three scales"""
    ip, ix, period, _, _ = R.schedule(gold["indptr"], gold["indices"], gold["data"], 500)
    nxt, neg = R.state_at(period, 37)
    r = np.random.RandomState(11)
    maps = {s: (s * r.randn(len(ip) - 1, 2)).astype(np.float32) for s in (0.3, 10.0)}
    return {"csr": (ip, ix, period), "state": (nxt, neg), "maps": maps, "a": float(gold["a"]), "b": float(gold["b"])}


@pytest.mark.parametrize("min_dist,a,b", [(0.1, 1.576943, 0.895061), (0.25, 1.121436, 1.057500), (0.001, 1.929073, 0.791505)])
def test_umap_ab(min_dist, a, b):
    for fn in (R.find_ab, sfv.umap_ab):
        got = fn(1.0, min_dist)
        assert abs(got[0] - a) < 1e-5 and abs(got[1] - b) < 1e-5, (fn, got)


@pytest.mark.parametrize("source,k", [("projection", 24), ("projection", 15), ("latent_scores", 24)])
def test_smooth_knn_properties(source, k):
    Xs = np.load(os.path.join(GOLDEN, source + ".npz"))["X"]
    idx, d2, _ = P.knn(Xs, k - 1)
    s = R.smooth_knn(d2)
    d = R.knn_dist(d2)
    assert not s["undecided"].any(), "a fixture row sits on a threshold"
    ok = ~s["floored"] & (s["steps"] < R.SMOOTH_ITERS)
    assert ok.mean() > 0.9
    ps = R.psum_at(d2, s["rho"], s["sigma"])
    assert np.all(np.abs(ps[ok] - np.log2(k)) < 1e-5)
    assert np.array_equal(s["rho"], np.where(d > 0, d, np.inf).min(1))
    w32 = s["w"].astype(np.float32)
    assert w32.max() <= 1.0 and w32.min() > 0.0 and np.all(w32[:, 0] == 1.0)       # the nearest neighbour: d = rho
    print(f"{source} k = {k}: steps {s['steps'].min()}..{s['steps'].max()}, {int(s['floored'].sum())} floored rows")


def test_smooth_knn_edge_cases():
    """duplicates: rows whose 14 neighbours all coincide with them (rho = 0, 64 evaluations, the global-mean floor,
    memberships 1), rows floored with rho > 0, and the all-identical input, where the floor is 0 and the 64 halvings
    leave sigma = 2^-64 (the text's sigma = 0 would need a 65th; the memberships are 1 either way)"""
    H = R.hard_codes_k15()
    idx, d2, _ = P.knn(H, 14)
    s = R.smooth_knn(d2)
    dup = s["rho"] == 0
    assert dup.any() and np.all(s["steps"][dup] == 64) and np.all(s["floored"][dup]) and np.all(s["w"][dup] == 1.0)
    assert np.all(s["sigma"][dup] == 1e-3 * R.knn_dist(d2).sum() / (len(H) * 15))
    assert np.any(s["floored"] & ~dup), "no row floored by its own mean"
    same = np.zeros((20, 14))
    s = R.smooth_knn(same)
    assert np.all(s["rho"] == 0) and np.all(s["sigma"] == 2.0 ** -64) and np.all(s["w"] == 1.0) and np.all(s["steps"] == 64)


def test_fuzzy_csr_is_the_dense_union(X):
    idx, d2, _ = P.knn(X, 23)
    w = R.smooth_knn(d2)["w"].astype(np.float32)
    W = R.fuzzy_dense(idx, w)
    assert np.array_equal(W, W.T) and W.max() <= 1.0 and W.min() >= 0.0
    for name, fn in (("restatement", R.fuzzy_csr), ("projection.fuzzy_csr", sfv.fuzzy_csr)):
        ip, ix, data = fn(idx, w)
        assert ip.dtype == np.int32 and ix.dtype == np.int32 and data.dtype == np.float32, name
        D = np.zeros_like(W)
        rows = np.repeat(np.arange(len(W)), np.diff(ip))
        assert np.all(np.diff(rows * len(W) + ix) > 0), f"{name}: not in (row, column) order"
        D[rows, ix] = data
        assert np.array_equal(D, W.astype(np.float32)), name
        assert data.min() > 0.0 and data.max() <= 1.0 and np.array_equal(D, D.T), name
    with pytest.raises(ValueError, match="outside"):
        sfv.fuzzy_csr(np.full((4, 2), 4, dtype=np.int32), np.ones((4, 2), dtype=np.float32))


def test_golden_graph_is_the_restatement(X, gold):
    idx, d2, _ = P.knn(X, 23)
    s = R.smooth_knn(d2)
    ip, ix, data = R.fuzzy_csr(idx, s["w"].astype(np.float32))
    assert np.array_equal(ip, gold["indptr"]) and np.array_equal(ix, gold["indices"]) and np.array_equal(data, gold["data"])
    assert np.array_equal(s["rho"].astype(np.float32), gold["rho"])
    assert np.array_equal(s["sigma"].astype(np.float32), gold["sigma"])
    assert abs(float(gold["a"]) - 1.121436) < 1e-5 and abs(float(gold["b"]) - 1.0575) < 1e-5
    assert len(gold["seq_ce"]) == 5 and gold["seq_ce"].max() < float(gold["ce_init"])


def test_schedule_closed_form():
    """activations of edge e through epoch n = the number of multiples of period_e that are <= n, on periods that are
    exact in f32; and the schedule keeps both directions of an edge (the graph stays symmetric)"""
    period = np.array([1.0, 1.25, 1.5, 2.0, 3.0, 7.75, 64.0, 499.0, 500.0, 1000.0], dtype=np.float32)
    for n_epochs in (1, 2, 38, 500):
        nxt, count = R.activations(period, n_epochs)
        want = np.floor((n_epochs - 1) / period.astype(np.float64)).astype(np.int64)
        assert np.array_equal(count, want), n_epochs
        assert np.array_equal(nxt, ((want + 1) * period.astype(np.float64)).astype(np.float32))
        assert np.array_equal(R.state_at(period, n_epochs)[0], nxt)
    W = np.array([[0, 1.0, 0.001], [1.0, 0, 0.5], [0.001, 0.5, 0]])
    for fn in (R.schedule, sfv.projection.umap_schedule):
        ip, ix, per, nxt, neg = fn(*R.dense_to_csr(W), 500)
        assert np.array_equal(ip, [0, 1, 3, 4]) and np.array_equal(ix, [1, 0, 2, 1])        # 0.001 < 1 / 500 is dropped
        assert np.array_equal(per, np.float32([1, 1, 2, 2])) and np.array_equal(nxt, per)
        assert np.array_equal(neg, per / np.float32(5))


def test_hash_restatement():
    """hash_u32 of csrc/common.h by hand on Python integers"""
    M = (1 << 64) - 1

    def h(seed, idx):
        x = ((idx + 1) * 0x9E3779B97F4A7C15 + seed) & M
        for _ in range(2):
            x ^= x >> 32
            x = (x * 0xD6E8FEB86659FD93) & M
        x ^= x >> 32
        return x & 0xFFFFFFFF

    keys = [0, 1, 255, (37 << 40) | (9801 << 8) | 31, (499 << 40) | (123456 << 8) | 7]
    assert [int(v) for v in R.hash_u32(42, np.array(keys, dtype=np.uint64))] == [h(42, k) for k in keys]
    e, p = np.array([9801, 123456]), np.array([31, 7])
    assert [int(v) for v in R.sample_index(42, 37, e[:1], p[:1], 320)] == [(h(42, keys[3]) * 320) >> 32]
    m = R.sample_index(7, 3, np.arange(100000), 0, 320)
    assert m.min() == 0 and m.max() == 319 and abs(np.bincount(m, minlength=320).std() - np.sqrt(100000 / 320)) < 5


@pytest.mark.parametrize("defect", R.SMOOTH_DEFECTS)
def test_smooth_knn_bound_rejects(X, defect):
    if defect == "self_in_psum":
        d2 = P.knn(X, 23)[1]
    else:
        d2 = P.knn(R.hard_codes_k15(), 14)[1]                # the floor is where the mean enters
    good, bad = R.smooth_knn(d2), R.smooth_knn(d2, defect)
    ref, bnd = R.stored(good["sigma"])
    assert not P.rejects(good["sigma"].astype(np.float32), ref, bnd)
    assert P.rejects(bad["sigma"].astype(np.float32), ref, bnd), f"{defect} passes the sigma bound"


def test_union_is_sum_rejected(X):
    idx, d2, _ = P.knn(X, 23)
    w = R.smooth_knn(d2)["w"].astype(np.float32)
    good, bad = R.fuzzy_csr(idx, w), R.fuzzy_csr(idx, w, "union_is_sum")
    assert np.array_equal(good[1], bad[1]) and not np.array_equal(good[2], bad[2])


@pytest.mark.parametrize("defect", R.EPOCH_DEFECTS)
def test_epoch_bound_rejects(layout, defect):
    a, b = layout["a"], layout["b"]
    Y = layout["maps"][0.3 if defect == "no_clip" else 10.0]
    args = (Y, *layout["csr"], *layout["state"], 37, 500, a, b)
    good, bad = R.epoch(*args), R.epoch(*args, defect=defect)
    assert good["active"].sum() > 100 and good["q"].sum() > 100
    assert not P.rejects(good["Y"].astype(np.float32), good["Y"], good["b_y"])
    if defect == "sample_may_be_self":                      # a self sample adds an exact zero: the index table shows it
        assert np.array_equal(bad["Y"], good["Y"])
        assert not np.array_equal(bad["samples"], good["samples"]), "no draw of this epoch hit its own vertex"
    else:
        assert P.rejects(bad["Y"], good["Y"], good["b_y"]), f"{defect} passes the Y bound"
    assert np.array_equal(bad["next"], good["next"]) and np.array_equal(bad["next_neg"], good["next_neg"])


def test_clip_is_active_on_the_close_map(layout):
    """|c D| of a negative sample exceeds 4 for 0.002 < r < 0.53 (b = 1.06): the scale-0.3 map has such pairs, the
    scale-10 map's sampled pairs almost never"""
    args = (*layout["csr"], *layout["state"], 37, 500, layout["a"], layout["b"])
    close, free = R.epoch(layout["maps"][0.3], *args), R.epoch(layout["maps"][0.3], *args, defect="no_clip")
    assert np.abs(free["Y"] - close["Y"]).max() > 1.0


def test_initial_map_and_cross_entropy(X, gold):
    Y0 = R.initial_map(P.pca(X, 2)[0], 42)
    assert np.array_equal(Y0, gold["Y0"]) and np.array_equal(Y0, sfv.projection.umap_initial_map(P.pca(X, 2)[0], 42))
    assert Y0.dtype == np.float32 and np.all(Y0.min(0) == 0.0) and np.all(Y0.max(0) == 10.0)
    ce = R.cross_entropy(Y0, gold["indptr"], gold["indices"], gold["data"], float(gold["a"]), float(gold["b"]))
    assert abs(ce - float(gold["ce_init"])) <= 1e-9 * ce
    # two points, one edge of weight 1/2 at distance 1: v = 1 / (1 + a)
    a, b = 1.5, 0.9
    two = R.cross_entropy(np.array([[0.0, 0.0], [1.0, 0.0]]), *R.dense_to_csr(np.array([[0, 0.5], [0.5, 0]])), a, b)
    v = 1.0 / (1.0 + a)
    assert abs(two - (0.5 * np.log(0.5 / v) + 0.5 * np.log(0.5 / (1.0 - v)))) < 1e-15


def test_cpu_inputs_and_arguments_raise():
    z = torch.zeros((8, 3))
    with pytest.raises(ValueError, match="GPU"):
        sfv.umap_project(z)
    with pytest.raises(ValueError, match="GPU"):
        sfv.fuzzy_graph(torch.zeros((8, 3), dtype=torch.int32), torch.zeros((8, 3), dtype=torch.float64), 4)
    with pytest.raises(ValueError, match="GPU"):
        sfv.umap_optimise(torch.zeros((8, 2)), None)
    protos = sfv._lib.parse_header()
    for name in ("rbvae_umap_smooth_knn_ok", "rbvae_umap_smooth_knn", "rbvae_umap_epoch_ok", "rbvae_umap_epoch",
                 "rbvae_umap_epoch_samples"):
        assert name in protos
    q = sfv._lib.query
    assert q("rbvae_umap_smooth_knn_ok", 2, 1) == 1 and q("rbvae_umap_smooth_knn_ok", 320, 127) == 1
    assert q("rbvae_umap_smooth_knn_ok", 320, 128) == 0 and q("rbvae_umap_smooth_knn_ok", 0, 3) == 0
    assert q("rbvae_umap_epoch_ok", 2, 500, 5) == 1 and q("rbvae_umap_epoch_ok", 16384, 200, 5) == 1
    assert q("rbvae_umap_epoch_ok", 16385, 200, 5) == 0 and q("rbvae_umap_epoch_ok", 1, 200, 5) == 0
    assert q("rbvae_umap_epoch_ok", 320, 0, 5) == 0 and q("rbvae_umap_epoch_ok", 320, 500, 0) == 0
