"""GPU: the UMAP kernels (csrc/umap.hip) element by element against tests/_umap_ref.py's f64 restatement and the bounds its
docstring derives, inside sentinel guard bands, and projection.py's umap_project end to end against the recorded
sequential runs of tests/golden/umap.npz (tools/make_umap_golden.py).

Whole run (umap_project(X, 24, 0.25) on the 320-row fixture, 500 epochs).  The fuzzy-set cross entropy over all pairs, in
f64 on the host, must be <= 1.05 x the mean of five runs of _umap_ref.layout_sequential (umap-learn's edge-by-edge loop in
f64, both ends moved, RandomState negatives) and below the midpoint between that mean and the initial map's, and
trustworthiness(n_neighbors=24) >= the sequential mean - 0.005.  Recorded sequential runs, seeds 42..46: cross entropy
6408.8, 6337.6, 6402.8, 6410.7, 6317.5 (mean 6375.5), trustworthiness 0.98983, 0.99013, 0.98991, 0.99026, 0.98986 (mean
0.99000); the initial map: 9381.6 and 0.98771.  An f64 numpy run of the synchronous scheme ends at 6557.5 and 0.98892.
Measured on one MI355X: cross entropy 6577.5, trustworthiness 0.98903, the map spans 31.7 x 23.7; bounds 6694.3 (1.05 x the
mean), 7878.6 (the midpoint) and 0.98500."""
import os

import numpy as np
import pytest
import torch

import _projection_ref as P
import _umap_ref as R
import sfv_amd as sfv

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N_EPOCHS, SEED = 500, 42
GUARD = 4096
SENT = {torch.float64: (torch.int64, 0x7FF8DEADDEADBEEF), torch.float32: (torch.int32, 0x7FC0DEAD),
        torch.int32: (torch.int32, -0x21524111)}


class Guarded:
    """n elements of dtype inside GUARD sentinel elements on each side (NaN sentinels for the float types), as
    test_projection_gpu.Guarded"""

    def __init__(self, dtype, *shape):
        self.n = int(np.prod(shape))
        raw, self.sent = SENT[dtype]
        self.buf = torch.full((GUARD + self.n + GUARD,), self.sent, dtype=raw, device="cuda")
        self.t = self.buf[GUARD:GUARD + self.n].view(dtype).view(*shape)

    def check(self, what, untouched=False):
        bits = self.buf.cpu().numpy()
        inner = np.zeros(bits.shape, dtype=bool)
        inner[GUARD:GUARD + self.n] = True
        stray = np.nonzero((bits != self.sent) & ~inner)[0]
        assert stray.size == 0, f"{what}: {stray.size} elements outside the output were written; first at {stray[0] - GUARD}"
        unwritten = np.nonzero((bits == self.sent) & inner)[0]
        if untouched:
            assert unwritten.size == self.n, f"{what}: a refused call wrote {self.n - unwritten.size} elements"
        else:
            assert unwritten.size == 0, f"{what}: {unwritten.size} elements never written; first at {unwritten[0] - GUARD}"
        return self.t.cpu().numpy()


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


@pytest.fixture(scope="module")
def X():
    return np.load(os.path.join(GOLDEN, "projection.npz"))["X"]


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "umap.npz")))


# ---- smooth kNN distances ------------------------------------------------------------------------------------------------

def _smooth(d2):
    N, K1 = d2.shape
    out = {"dsum": Guarded(torch.float64, 1), "rho": Guarded(torch.float32, N), "sigma": Guarded(torch.float32, N),
           "w": Guarded(torch.float32, N, K1), "steps": Guarded(torch.int32, N)}
    assert sfv._lib.query("rbvae_umap_smooth_knn_ok", N, K1) == 1
    sfv._lib.call("rbvae_umap_smooth_knn", _dev(d2), N, K1, *(out[n].t for n in ("dsum", "rho", "sigma", "w", "steps")))
    return {n: g.check(n) for n, g in out.items()}


def _check_smooth(d2, what, fixture=False):
    got, ref = _smooth(d2), R.smooth_knn(d2)
    ok = ~ref["undecided"]
    assert ok.mean() >= 0.99 and (ok.all() or not fixture), f"{what}: {int((~ok).sum())} undecided rows"
    assert np.array_equal(got["rho"].view(np.int32), ref["rho"].astype(np.float32).view(np.int32)), "rho"
    assert np.array_equal(got["steps"][ok], ref["steps"][ok]), "steps"
    total = float(ref["d"].astype(np.longdouble).sum())
    assert abs(got["dsum"][0] - total) <= 1e-12 * total
    ws = P.within(got["sigma"][ok], *R.stored(ref["sigma"][ok]), f"sigma ({what})")
    ww = P.within(got["w"][ok], *R.stored(ref["w"][ok]), f"w ({what})")
    print(f"smooth kNN {what}: {int((~ok).sum())} undecided rows, steps {got['steps'].min()}..{got['steps'].max()}, "
          f"{int(ref['floored'].sum())} floored, worst |err|/bound sigma {ws:.3g}, w {ww:.3g}")
    return got, ref


@pytest.mark.parametrize("N,k", [(2, 2), (65, 64), (257, 15), (320, 24), (320, 128)])
def test_smooth_knn(X, N, k):
    if N == 320:
        Xs = X
    else:
        r = np.random.RandomState(N + k)
        Xs = (1.0 / (1.0 + np.exp(-2.0 * r.randn(N, 7)))).astype(np.float32)
    _check_smooth(P.knn(Xs, k - 1)[1], f"({N}, {k})", fixture=N == 320)


def test_smooth_knn_second_fixture():
    Xs = np.load(os.path.join(GOLDEN, "latent_scores.npz"))["X"]
    _check_smooth(P.knn(Xs, 23)[1], "latent_scores X, k = 24", fixture=True)


def test_smooth_knn_duplicates():
    """hard codes at k = 15: rows whose 14 neighbours all coincide with them (rho = 0, 64 evaluations, the global-mean
    floor, memberships 1), rows floored by their own mean; and all rows identical: the floor is 0, the 64 halvings leave
    sigma = 2^-64, memberships 1"""
    got, ref = _check_smooth(P.knn(R.hard_codes_k15(), 14)[1], "hard codes")
    dup = ref["rho"] == 0
    assert dup.any() and np.any(ref["floored"] & ~dup) and not ref["undecided"].any()
    assert np.all(got["steps"][dup] == 64) and np.all(got["w"][dup] == 1.0) and np.all(got["rho"][dup] == 0.0)
    got, ref = _check_smooth(np.zeros((20, 14)), "identical rows")
    assert np.all(got["sigma"] == np.float32(2.0 ** -64)) and np.all(got["w"] == 1.0) and np.all(got["steps"] == 64)
    assert got["dsum"][0] == 0.0


def test_fuzzy_graph(X, gold):
    idx, d2 = sfv.knn_graph(_dev(X), 23)
    g = sfv.fuzzy_graph(idx, d2, 24)
    w = g.membership.cpu().numpy()
    ip, ix, data = R.fuzzy_csr(idx.cpu().numpy(), w)        # the union of the device's own memberships: bit-equal
    assert np.array_equal(g.indptr.cpu().numpy(), ip) and np.array_equal(g.indices.cpu().numpy(), ix)
    assert np.array_equal(g.data.cpu().numpy().view(np.int32), data.view(np.int32))
    assert np.array_equal(ip, gold["indptr"]) and np.array_equal(ix, gold["indices"])
    assert np.abs(g.data.cpu().numpy().astype(np.float64) / gold["data"] - 1.0).max() <= 4 * R.V
    assert np.array_equal(g.rho.cpu().numpy(), gold["rho"])
    assert np.abs(g.sigma.cpu().numpy().astype(np.float64) / gold["sigma"] - 1.0).max() <= 2 * R.V


# ---- one epoch -----------------------------------------------------------------------------------------------------------

def _epoch(Y, ip, ix, period, nxt, neg, n, n_epochs, a, b, gamma=1.0, rate=5, seed=SEED):
    """-> (Y_out, next, next_neg, count, samples) from the device, every output inside guard bands, Y checked untouched"""
    N, E = len(Y), len(ix)
    assert sfv._lib.query("rbvae_umap_epoch_ok", N, n_epochs, rate) == 1
    Yg, Yo = Guarded(torch.float32, N, 2), Guarded(torch.float32, N, 2)
    nx, ng = Guarded(torch.float32, E), Guarded(torch.float32, E)
    cnt, smp = Guarded(torch.int32, E), Guarded(torch.int32, E, R.MAX_SAMPLES)
    Yg.t.copy_(_dev(Y))
    nx.t.copy_(_dev(nxt))
    ng.t.copy_(_dev(neg))
    dip, dix, dper = _dev(ip), _dev(ix), _dev(period)
    sfv._lib.call("rbvae_umap_epoch_samples", dip, dper, nx.t, ng.t, N, n, n_epochs, rate, seed, cnt.t, smp.t)
    assert np.array_equal(nx.check("next"), nxt) and np.array_equal(ng.check("next_neg"), neg)
    sfv._lib.call("rbvae_umap_epoch", Yg.t, Yo.t, dip, dix, dper, nx.t, ng.t, N, n, n_epochs, a, b, gamma, rate, seed)
    assert np.array_equal(Yg.check("Y").view(np.int32), Y.view(np.int32)), "Y was written"
    return Yo.check("Y_out"), nx.check("next"), ng.check("next_neg"), cnt.check("count"), smp.check("samples")


def _check_epoch(Y, csr, state, n, n_epochs, a, b, what, **kw):
    got = _epoch(Y, *csr, *state, n, n_epochs, a, b, **kw)
    ref = R.epoch(Y, *csr, *state, n, n_epochs, a, b, gamma=kw.get("gamma", 1.0), negative_sample_rate=kw.get("rate", 5),
                  seed=kw.get("seed", SEED))
    assert np.array_equal(got[3], ref["q"]), f"{what}: sample counts"
    assert np.array_equal(got[4], ref["samples"]), f"{what}: sampled indices"
    assert np.array_equal(got[1].view(np.int32), ref["next"].view(np.int32)), f"{what}: next"
    assert np.array_equal(got[2].view(np.int32), ref["next_neg"].view(np.int32)), f"{what}: next_neg"
    w = P.within(got[0], ref["Y"], ref["b_y"], f"Y_out ({what})")
    again = _epoch(Y, *csr, *state, n, n_epochs, a, b, **kw)
    assert all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(got, again)), f"{what}: two runs differ"
    moved = float(np.abs(ref["Y"] - Y).max())
    print(f"epoch {what}: {int(ref['active'].sum())} active edges, {int(ref['q'].sum())} samples "
          f"({int(((ref['samples'] < 0) & (np.arange(R.MAX_SAMPLES) < ref['q'][:, None])).sum())} own vertex), largest "
          f"move {moved:.3g}, worst |err|/bound {w:.3g}")
    return ref


@pytest.fixture(scope="module")
def fixture_layout(gold):
    ip, ix, period, _, _ = R.schedule(gold["indptr"], gold["indices"], gold["data"], N_EPOCHS)
    return (ip, ix, period), {n: R.state_at(period, n) for n in (0, 1, 37, N_EPOCHS - 1)}


@pytest.mark.parametrize("scale", [1e-4, 0.3, 10.0, 50.0])
@pytest.mark.parametrize("n", [0, 1, 37, N_EPOCHS - 1])
def test_epoch_on_the_fixture_graph(gold, fixture_layout, n, scale):
    """maps of scale 1e-4 with coincident points (the r2 = 0 branches), 0.3 (where the clip of the negative samples is
    active: |c D| > 4 for 0.002 < r < 0.53), 10 and 50"""
    csr, states = fixture_layout
    N = len(csr[0]) - 1
    Y = (scale * np.random.RandomState(int(n) + 7).randn(N, 2)).astype(np.float32)
    if scale == 1e-4:
        Y[N // 2:] = Y[:N - N // 2]                         # every point has a twin
    ref = _check_epoch(Y, csr, states[n], n, N_EPOCHS, float(gold["a"]), float(gold["b"]), f"n = {n}, scale {scale}")
    assert (ref["active"].sum() > 0) == (n > 0)             # next = period >= 1: epoch 0 moves nothing
    if n == 0:
        assert np.array_equal(ref["Y"], Y.astype(np.float64))
    if n == 37 and scale == 0.3:
        free = R.epoch(Y, *csr, *states[n], n, N_EPOCHS, float(gold["a"]), float(gold["b"]), seed=SEED, defect="no_clip")
        assert np.abs(free["Y"] - ref["Y"]).max() > 1.0, "the clip is not active on this map"


@pytest.mark.parametrize("n", [1, 5])
def test_epoch_star_graph(n):
    """the hub's row has 199 edges: four chunks of 64, the last one partial; other parameters than the defaults"""
    N = 200
    ip, ix, data = R.star_graph(N)
    assert np.diff(ip).max() == N - 1
    ip, ix, period, _, _ = R.schedule(ip, ix, data, 11, 3)
    Y = (2.0 * np.random.RandomState(n).randn(N, 2)).astype(np.float32)
    ref = _check_epoch(Y, (ip, ix, period), R.state_at(period, n, 3), n, 11, 1.576943, 0.895061, f"star, n = {n}",
                       gamma=0.5, rate=3, seed=(1 << 40) + 9)
    hub = np.nonzero(ref["active"][:N - 1])[0]
    assert hub.size > 0 and (n == 1 or (hub.size > 32 and hub.min() < 64 and hub.max() >= 128))


def test_epoch_two_points():
    ip, ix, data = R.dense_to_csr(np.array([[0.0, 1.0], [1.0, 0.0]]))
    ip, ix, period, _, _ = R.schedule(ip, ix, data, 10)
    for n in (1, 9):
        Y = np.array([[0.0, 0.0], [3.0, -1.0]], dtype=np.float32)
        ref = _check_epoch(Y, (ip, ix, period), R.state_at(period, n), n, 10, 1.121436, 1.0575, f"N = 2, n = {n}")
        assert ref["active"].all() and np.abs(ref["Y"] - Y).max() > 0


def test_refused_arguments_write_nothing():
    ip, ix, data = R.dense_to_csr(np.array([[0.0, 1.0], [1.0, 0.0]]))
    ip, ix, period, nxt, neg = (_dev(x) for x in R.schedule(ip, ix, data, 10))
    Y, Yo = Guarded(torch.float32, 2, 2), Guarded(torch.float32, 2, 2)
    nx, ng = Guarded(torch.float32, 2), Guarded(torch.float32, 2)
    cnt, smp = Guarded(torch.int32, 2), Guarded(torch.int32, 2, R.MAX_SAMPLES)
    call = sfv._lib.call

    def epoch(**kw):
        p = dict(Y=Y.t, Yo=Yo.t, N=2, n=1, n_epochs=10, a=1.1, b=1.0, gamma=1.0, rate=5)
        p.update(kw)
        call("rbvae_umap_epoch", p["Y"], p["Yo"], ip, ix, period, nx.t, ng.t, p["N"], p["n"], p["n_epochs"], p["a"], p["b"],
             p["gamma"], p["rate"], 42)

    for match, kw in (("Y_out", dict(Yo=Y.t)), ("N=1", dict(N=1)), ("N=16385", dict(N=16385)), ("epoch=10", dict(n=10)),
                      ("epoch=-1", dict(n=-1)), ("n_epochs=0", dict(n_epochs=0, n=0)), ("a=0", dict(a=0.0)),
                      ("b=-1", dict(b=-1.0)), ("gamma", dict(gamma=-1.0)), ("neg_rate=0", dict(rate=0)),
                      ("null", dict(Yo=None)), ("aligned", dict(Yo=Yo.t.view(-1)[1:3]))):
        with pytest.raises(ValueError, match=match):
            epoch(**kw)
    with pytest.raises(ValueError, match="epoch=10"):
        call("rbvae_umap_epoch_samples", ip, period, nx.t, ng.t, 2, 10, 10, 5, 42, cnt.t, smp.t)
    with pytest.raises(ValueError, match="null"):
        call("rbvae_umap_epoch_samples", ip, period, nx.t, ng.t, 2, 1, 10, 5, 42, None, smp.t)
    for g, name in ((Y, "Y"), (Yo, "Y_out"), (nx, "next"), (ng, "next_neg"), (cnt, "count"), (smp, "samples")):
        g.check(name, untouched=True)
    d2 = torch.ones((4, 128), dtype=torch.float64, device="cuda")
    out = [Guarded(torch.float64, 1), Guarded(torch.float32, 4), Guarded(torch.float32, 4), Guarded(torch.float32, 4, 128),
           Guarded(torch.int32, 4)]
    with pytest.raises(ValueError, match="K1=128"):
        call("rbvae_umap_smooth_knn", d2, 4, 128, *(g.t for g in out))
    with pytest.raises(ValueError, match="N=0"):
        call("rbvae_umap_smooth_knn", d2, 0, 3, *(g.t for g in out))
    with pytest.raises(ValueError, match="null"):
        call("rbvae_umap_smooth_knn", d2, 4, 3, out[0].t, None, out[2].t, out[3].t, out[4].t)
    for g in out:
        g.check("smooth kNN output", untouched=True)
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")       # noqa: E731
    for k in (1, 9, 129):
        with pytest.raises(ValueError, match="n_neighbors"):
            sfv.umap_project(z(8, 3) if k < 129 else z(200, 3), n_neighbors=k)
    idx, dd = sfv.knn_graph(z(8, 3), 3)
    with pytest.raises(ValueError, match="columns"):
        sfv.fuzzy_graph(idx, dd, 5)
    with pytest.raises(ValueError, match="init"):
        sfv.umap_project(z(8, 3), n_neighbors=4, init=z(7, 2))


# ---- whole run -----------------------------------------------------------------------------------------------------------

def test_umap_project_whole_run(X, gold):
    from sklearn.manifold import trustworthiness
    Xd = _dev(X)
    r1 = sfv.umap_project(Xd, 24, 0.25)
    r2 = sfv.umap_project(Xd, 24, 0.25)
    Ya, Yb = r1.embedding.cpu().numpy(), r2.embedding.cpu().numpy()
    assert Ya.dtype == np.float32 and Ya.shape == (len(X), 2) and np.isfinite(Ya).all()
    assert np.array_equal(Ya.view(np.int32), Yb.view(np.int32)), "two runs differ"
    assert r1.n_epochs == N_EPOCHS and abs(r1.a - float(gold["a"])) < 1e-9 and abs(r1.b - float(gold["b"])) < 1e-9
    ce = R.cross_entropy(Ya, gold["indptr"], gold["indices"], gold["data"], float(gold["a"]), float(gold["b"]))
    trust = trustworthiness(X, Ya, n_neighbors=24)
    seq_ce, seq_trust, ce0 = float(gold["seq_ce"].mean()), float(gold["seq_trust"].mean()), float(gold["ce_init"])
    print(f"whole run: cross entropy {ce:.1f} (sequential mean {seq_ce:.1f}, initial map {ce0:.1f}), trustworthiness "
          f"{trust:.5f} (sequential mean {seq_trust:.5f}), span {np.ptp(Ya, axis=0)}")
    assert ce <= 1.05 * seq_ce
    assert ce < 0.5 * (seq_ce + ce0)
    assert trust >= seq_trust - 0.005
    other = sfv.umap_project(Xd, 24, 0.25, seed=43).embedding.cpu().numpy()
    assert not np.array_equal(other, Ya)
    Y0 = _dev(gold["Y0"])
    graph = sfv.fuzzy_graph(*sfv.knn_graph(Xd, 23), 24)
    res = sfv.umap_optimise(Y0, graph, a=r1.a, b=r1.b)
    assert np.array_equal(gold["Y0"], Y0.cpu().numpy()), "the initial map was written"
    init = sfv.umap_project(Xd, 24, 0.25, init=Y0).embedding
    assert torch.equal(res.embedding, init)


# ---- the script's loop ---------------------------------------------------------------------------------------------------

def test_latent_projections_with_umap():
    F_, RES, LD = 48, 64, 16
    torch.manual_seed(0)
    model = sfv.Seq2SeqBinaryVAE(3, 3, LD, LD, variant="contrastive", input_hw=(RES, RES), compute_dtype="f32").cuda().eval()
    x = torch.rand(F_, 3, RES, RES, generator=torch.Generator().manual_seed(1)).cuda()
    u = torch.rand(F_, LD, generator=torch.Generator().manual_seed(2))
    flags = [10, 30]
    kw = dict(u=u, frame_indices=range(F_), flags=flags, perplexity=5.0, max_iter=250)
    plain = sfv.latent_projections(model, x, **kw)
    assert sorted(plain) == ["labels", "latents", "pca", "tsne"]
    cfg = {"n_neighbors": 24, "min_dist": 0.25, "seed": 42}
    out = sfv.latent_projections(model, x, umap=cfg, **kw)
    assert sorted(out) == ["labels", "latents", "pca", "tsne", "umap"]
    assert torch.equal(out["latents"], plain["latents"]) and torch.equal(out["tsne"].embedding, plain["tsne"].embedding)
    want = sfv.umap_project(out["latents"], **cfg)
    assert tuple(out["umap"].embedding.shape) == (F_, 2) and torch.equal(out["umap"].embedding, want.embedding)
    assert bool(torch.isfinite(out["umap"].embedding).all())
    s_plain = sfv.latent_scores(model, x, range(F_), flags, projections=plain, n_neighbors=5, u=u)
    s = sfv.latent_scores(model, x, range(F_), flags, projections=out, n_neighbors=5, u=u)
    assert sorted(set(s) - set(s_plain)) == ["continuity_umap", "trustworthiness_umap"]
    assert s["trustworthiness_umap"] == sfv.trustworthiness(out["latents"], out["umap"].embedding, 5)
    assert s["continuity_umap"] == sfv.continuity(out["latents"], out["umap"].embedding, 5)
    assert 0.0 <= s["trustworthiness_umap"] <= 1.0 and s["trustworthiness_tsne"] == s_plain["trustworthiness_tsne"]
