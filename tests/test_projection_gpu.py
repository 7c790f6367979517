"""GPU: the projection kernels (csrc/project.hip) element by element against tests/_projection_ref.py's f64 restatement
and the bounds its docstring derives, inside sentinel guard bands, and projection.py end to end against the
scikit-learn fixture tests/golden/projection.npz (tools/make_projection_golden.py).

Whole run (tsne_project on the fixture, 1000 iterations): the final KL, recomputed in f64 from the device's map and
scikit-learn's joint P, must be <= 1.05 x scikit-learn's kl_divergence_ (0.1262), and trustworthiness(n_neighbors=24)
>= scikit-learn's (0.99610) - 0.005.  Measured on one MI355X: KL 0.12035, trustworthiness 0.99584, n_iter 999 (f64
numpy runs of the same scheme end at KL 0.1196 to 0.1219 and trustworthiness 0.99587 to 0.99603, depending on how the
initial map is rounded: the trajectory is sensitive to the last bit, the objective is not)."""
import os

import numpy as np
import pytest
import torch

import _projection_ref as R
import sfv_amd as sfv

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "projection.npz")
K, PERPLEXITY = 91, 30.0
GUARD = 4096
SENT = {torch.float64: (torch.int64, 0x7FF8DEADDEADBEEF), torch.float32: (torch.int32, 0x7FC0DEAD),
        torch.int32: (torch.int32, -0x21524111)}


class Guarded:
    """n elements of dtype inside GUARD sentinel elements on each side (NaN sentinels for the float types)"""

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
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def graph(gold):
    idx, d2, decided = R.knn(gold["X"], K)
    P, beta, steps, near = R.perplexity_search(d2, PERPLEXITY)
    return {"idx": idx, "d2": d2, "decided": decided, "P": P, "beta": beta, "steps": steps, "near": near}


def _csr(gold):
    return gold["joint_indptr"], gold["joint_indices"], gold["joint_data"].astype(np.float32)


# ---- kNN ---------------------------------------------------------------------------------------------------------------

def _knn_guarded(X, k):
    N, Ld = X.shape
    idx, d2 = Guarded(torch.int32, N, k), Guarded(torch.float64, N, k)
    sfv._lib.call("rbvae_knn", _dev(X), N, Ld, k, idx.t, d2.t)
    return idx.check("idx"), d2.check("d2")


@pytest.mark.parametrize("N,Ld,k", [(2, 1, 1), (65, 3, 64), (257, 50, 91), (320, 50, 91), (700, 128, 24)])
def test_knn(gold, N, Ld, k):
    fixture = (N, Ld, k) == (320, 50, 91)
    if fixture:
        X = gold["X"]
    else:
        r = np.random.RandomState(N + Ld)
        X = (1.0 / (1.0 + np.exp(-2.0 * r.randn(N, Ld)))).astype(np.float32)
    assert sfv._lib.query("rbvae_knn_ok", N, Ld, k) == 1
    idx, d2 = _knn_guarded(X, k)
    ridx, rd2, decided = R.knn(X, k)
    assert decided.mean() >= 0.99 and (decided.all() or not fixture)
    assert np.array_equal(idx[decided], ridx[decided])
    w = R.within(d2[decided], rd2[decided], (Ld + 1) * R.U * rd2[decided] + R.TINY, f"d2 ({N}, {Ld}, {k})")
    print(f"kNN ({N}, {Ld}, {k}): {int((~decided).sum())} undecided rows, worst |err|/bound {w:.3g}")
    assert not np.any(idx == np.arange(N)[:, None]) and idx.min() >= 0 and idx.max() < N
    assert np.all(np.diff(d2, axis=1) >= 0)
    if fixture:
        assert np.array_equal(idx, gold["nn_idx"])
        i2, dd2 = sfv.knn_graph(_dev(X), k)
        assert np.array_equal(i2.cpu().numpy(), idx) and np.array_equal(dd2.cpu().numpy().view(np.int64), d2.view(np.int64))


def _knn_ref_blocked(X, k, block=1024):
    """R.knn's keys for sizes whose N x N matrix does not belong on the host: the same f64 arithmetic in the same order
    (l ascending, each square rounded once) in torch's element-wise f64 operations, a block of query rows at a time, and
    a stable sort, which orders equal distances by index.  -> (idx, d2, decided) as R.knn"""
    Xd = torch.from_numpy(X).cuda().double()
    N, Ld = Xd.shape
    out_i, out_d, out_ok = [], [], []
    for i0 in range(0, N, block):
        rows = torch.arange(i0, min(N, i0 + block), device="cuda")
        D = torch.zeros((len(rows), N), dtype=torch.float64, device="cuda")
        for l in range(Ld):
            df = Xd[rows, l][:, None] - Xd[None, :, l]
            D += df * df
        D[torch.arange(len(rows), device="cuda"), rows] = float("inf")
        srt, order = torch.sort(D, dim=1, stable=True)
        head = srt[:, :min(k + 1, N - 1)]
        gap = head[:, 1:] - head[:, :-1]
        out_ok.append(((gap == 0) | (gap >= 1e-12 * head[:, 1:])).all(dim=1))
        out_i.append(order[:, :k].to(torch.int32))
        out_d.append(srt[:, :k])
    return torch.cat(out_i).cpu().numpy(), torch.cat(out_d).cpu().numpy(), torch.cat(out_ok).cpu().numpy()


@pytest.mark.parametrize("N,Ld,k", [(12298, 50, 91), (16384, 2, 3)])
def test_knn_large(N, Ld, k):
    """the whole video's size (98 KB of LDS: the opt-in above 64 KB) and then the cap (131 KB: the reservation grows),
    every row against the blocked reference"""
    r = np.random.RandomState(N + Ld)
    X = (1.0 / (1.0 + np.exp(-2.0 * r.randn(N, Ld)))).astype(np.float32)
    assert sfv._lib.query("rbvae_knn_ok", N, Ld, k) == 1
    idx, d2 = _knn_guarded(X, k)
    ridx, rd2, decided = _knn_ref_blocked(X, k)
    assert decided.mean() >= 0.99
    assert np.array_equal(idx[decided], ridx[decided])
    w = R.within(d2[decided], rd2[decided], (Ld + 1) * R.U * rd2[decided] + R.TINY, f"d2 ({N}, {Ld}, {k})")
    print(f"kNN ({N}, {Ld}, {k}): {int((~decided).sum())} undecided rows, worst |err|/bound {w:.3g}")
    assert not np.any(idx == np.arange(N)[:, None]) and idx.min() >= 0 and idx.max() < N
    assert np.all(np.diff(d2, axis=1) >= 0)


def test_knn_ties_go_to_the_lower_index():
    """hard 0/1 codes with many duplicates: integer distances, zeros, exact ties, all exact in f64"""
    X = R.hard_codes()
    idx, d2 = _knn_guarded(X, 64)
    ridx, rd2, decided = R.knn(X, 64)
    assert decided.all() and np.any(rd2 == 0.0) and np.any(np.diff(rd2, axis=1) == 0)
    assert np.array_equal(d2, rd2) and np.array_equal(idx, ridx)


# ---- perplexity --------------------------------------------------------------------------------------------------------

def test_perplexity_search(gold, graph):
    N = len(graph["d2"])
    P, beta, steps = Guarded(torch.float64, N, K), Guarded(torch.float64, N), Guarded(torch.int32, N)
    sfv._lib.call("rbvae_tsne_perplexity", _dev(graph["d2"]), N, K, PERPLEXITY, P.t, beta.t, steps.t)
    Ph, bh, sh = P.check("P"), beta.check("beta"), steps.check("steps")
    ok = ~graph["near"]
    assert ok.mean() >= 0.99 and ok.all(), "the fixture must have no row on the tolerance threshold"
    assert np.array_equal(sh[ok], graph["steps"][ok])
    w = R.within(Ph[ok], graph["P"][ok], 1e-12 * graph["P"][ok] + R.TINY, "conditional P")
    wb = R.within(bh[ok], graph["beta"][ok], 1e-12 * graph["beta"][ok], "beta")
    print(f"perplexity: worst |err|/bound P {w:.3g}, beta {wb:.3g}; steps {sh.min()}..{sh.max()}")
    assert np.all(np.abs(Ph.sum(1) - 1.0) <= 1e-12)
    assert np.abs(Ph / gold["cond_P"] - 1.0).max() <= 1e-9          # and scikit-learn's own output


# ---- repulsion ---------------------------------------------------------------------------------------------------------

def _repulse(Y):
    N = len(Y)
    splits = sfv._lib.query("rbvae_tsne_repulse_splits", N)
    part = Guarded(torch.float32, splits, N, 3)
    sfv._lib.call("rbvae_tsne_repulse", _dev(Y), N, part.t)
    ph = part.check(f"part (N = {N})")
    Z = Guarded(torch.float64, 1)
    sfv._lib.call("rbvae_tsne_zsum", part.t, N, Z.t)
    return ph, float(Z.check("Z")[0]), part, Z


def _combine(part):
    """the slices added in f32, s ascending, as the step kernel adds them"""
    acc = part[0].copy()
    for s in range(1, part.shape[0]):
        acc = (acc + part[s]).astype(np.float32)
    return acc


@pytest.mark.parametrize("scale", [1e-4, 3.0, 50.0])
@pytest.mark.parametrize("N", [1, 2, 63, 64, 257, 700, 1100])
def test_repulsion(N, scale):
    Y = (scale * np.random.RandomState(N).randn(N, 2)).astype(np.float32)
    part, Z, _, _ = _repulse(Y)
    splits = R.repulse_shape(N)[0]
    assert part.shape[0] == splits and (splits > 1) == (N > 256)
    got = _combine(part)
    Rr, Zi, S_R, S_Z = R.repulsion(Y)
    wr = R.within(got[:, :2], Rr, R.repulsion_bound(N, S_R), f"R (N = {N}, scale {scale})")
    wz = R.within(got[:, 2], Zi, R.repulsion_bound(N, S_Z), f"Z_i (N = {N}, scale {scale})")
    zref = float(part[:, :, 2].astype(np.float64).sum())
    assert abs(Z - zref) <= N * splits * R.U * zref + R.TINY
    print(f"repulsion N = {N}, scale {scale}, {splits} splits: worst |err|/bound R {wr:.3g}, Z_i {wz:.3g}")
    if N == 1:
        assert np.all(got == 0.0) and Z == 0.0


def _repulsion_ref_blocked(Y, block=512):
    """R.repulsion's sums for an N whose N x N matrices do not belong on the host: the same f64 expressions in torch's
    element-wise f64 operations, a block of i rows at a time.  Its own rounding (about N 2^-53 S) is 1e-9 of the bound."""
    Yd = torch.from_numpy(Y).cuda().double()
    N = len(Yd)
    Rr, S_R, Zi = [], [], []
    for i0 in range(0, N, block):
        rows = torch.arange(i0, min(N, i0 + block), device="cuda")
        d = Yd[rows][:, None, :] - Yd[None, :, :]
        q = 1.0 / (1.0 + (d * d).sum(-1))
        q[torch.arange(len(rows), device="cuda"), rows] = 0.0
        q2 = (q * q)[:, :, None]
        Rr.append((q2 * d).sum(1))
        S_R.append((q2 * d.abs()).sum(1))
        Zi.append(q.sum(1))
    return torch.cat(Rr).cpu().numpy(), torch.cat(Zi).cpu().numpy(), torch.cat(S_R).cpu().numpy()


@pytest.mark.parametrize("N,scale", [(8449, 1e-4), (8449, 3.0), (8449, 50.0), (12298, 3.0)])
def test_repulsion_several_chunks_per_slice(N, scale):
    """above N = 8192 a slice of j holds more than one LDS chunk (2 at 8449, 3 at 12 298, a partial last chunk in both):
    the chunk is reloaded under the barrier, chunk sums are added, and c_chain's chunks-per-slice term counts; every i
    and every partial"""
    Y = (scale * np.random.RandomState(N).randn(N, 2)).astype(np.float32)
    part, Z, _, _ = _repulse(Y)
    splits, _, per = R.repulse_shape(N)
    assert part.shape[0] == splits and per == {8449: 2, 12298: 3}[N]
    got = _combine(part)
    Rr, Zi, S_R = _repulsion_ref_blocked(Y)
    wr = R.within(got[:, :2], Rr, R.repulsion_bound(N, S_R), f"R (N = {N}, scale {scale})")
    wz = R.within(got[:, 2], Zi, R.repulsion_bound(N, Zi), f"Z_i (N = {N}, scale {scale})")
    zref = float(part[:, :, 2].astype(np.float64).sum())
    assert abs(Z - zref) <= N * splits * R.U * zref + R.TINY
    print(f"repulsion N = {N}, scale {scale}, {splits} splits x {per} chunks: worst |err|/bound R {wr:.3g}, Z_i {wz:.3g}")


# ---- step --------------------------------------------------------------------------------------------------------------

def _step(Y, update, gains, csr, sched, part_t, Z_t):
    N = len(Y)
    Yo, up, gn = Guarded(torch.float32, N, 2), Guarded(torch.float32, N, 2), Guarded(torch.float32, N, 2)
    up.t.copy_(_dev(update))
    gn.t.copy_(_dev(gains))
    stats = Guarded(torch.float64, sfv._lib.query("rbvae_tsne_step_parts", N), 3)
    sfv._lib.call("rbvae_tsne_step", _dev(Y), Yo.t, up.t, gn.t, _dev(csr[0]), _dev(csr[1]), _dev(csr[2]), part_t, Z_t,
                  _dev(np.array(sched, dtype=np.float32)), N, stats.t)
    return Yo.check("Y_out"), up.check("update"), gn.check("gains"), stats.check("stats")


def test_step(gold):
    Y, csr = gold["Y"], _csr(gold)
    N = len(Y)
    rng = np.random.RandomState(3)
    update = (0.05 * rng.randn(N, 2)).astype(np.float32)
    gains = (0.5 + rng.rand(N, 2)).astype(np.float32)
    gains[::7] = 0.0101                                     # the floor at 0.01 is reached
    update[::11] = 0.0                                      # update x g == 0: the gain shrinks
    sched = (12.0, 0.5, 200.0)
    part, Z, part_g, Z_g = _repulse(Y)
    Yo, up, gn, stats = _step(Y, update, gains, csr, sched, part_g.t, Z_g.t)
    ref = R.step(Y, update, gains, *csr, sched, part, Z)
    fixed = ~ref["free"]
    assert fixed.mean() >= 0.99
    assert np.array_equal(gn[fixed], ref["gains"][fixed]), "gains"
    assert gn.min() >= np.float32(0.01) and np.any(gn == np.float32(0.01))
    wu = R.within(up[fixed], ref["update"][fixed], ref["b_u"][fixed], "update")
    wy = R.within(Yo[fixed], ref["Y"][fixed], ref["b_y"][fixed], "Y")
    s = stats.sum(0)
    print(f"step: worst |err|/bound update {wu:.3g}, Y {wy:.3g}; |g|^2 {s[0]:.6g} (ref {ref['gg']:.6g}, bound "
          f"{ref['b_gg']:.3g}), KL {s[2]:.9g} (ref {ref['kl']:.9g}, bound {ref['b_kl']:.3g})")
    assert abs(s[0] - ref["gg"]) <= ref["b_gg"]
    assert abs(s[1] - ref["sgg"]) <= ref["b_sgg"]
    assert abs(s[2] - ref["kl"]) <= ref["b_kl"]


def test_step_gradient_against_sklearn(gold):
    """zero update, unit gains, momentum 0, learning rate 1, no exaggeration: update' = -(0.8 g), so the kernel's gradient
    can be read off and compared with _kl_divergence_bh(angle=0)'s: within scikit-learn's f32 (1e-6 max |g|, the figure the
    CPU test holds the f64 restatement to) plus the kernel's own bound"""
    Y, csr = gold["Y"], _csr(gold)
    N = len(Y)
    part, Z, part_g, Z_g = _repulse(Y)
    Yo, up, gn, stats = _step(Y, np.zeros((N, 2), np.float32), np.ones((N, 2), np.float32), csr, (1.0, 0.0, 1.0),
                              part_g.t, Z_g.t)
    assert np.all(gn == np.float32(0.8))
    g = -up.astype(np.float64) / float(np.float32(0.8))
    ref = R.step(Y, np.zeros((N, 2)), np.ones((N, 2)), *csr, (1.0, 0.0, 1.0), part, Z)
    own = ref["b_g"] + 2 * R.V * np.abs(ref["g"])           # the kernel's bound, and the two roundings of 0.8 g
    d = np.abs(g - gold["grad"])
    print(f"gradient: max |device - sklearn| {d.max():.3g}, scikit-learn's f32 {1e-6 * np.abs(gold['grad']).max():.3g}, "
          f"own bound up to {own.max():.3g}; KL {stats.sum(0)[2]:.7f} against {float(gold['error']):.7f}")
    R.within(g, gold["grad"], 1e-6 * np.abs(gold["grad"]).max() + own, "g against scikit-learn")
    R.within(g, ref["g"], own, "g")
    assert abs(stats.sum(0)[2] - ref["kl"]) <= ref["b_kl"]


# ---- whole run ---------------------------------------------------------------------------------------------------------

def test_tsne_project_whole_run(gold):
    from sklearn.manifold import trustworthiness
    X = _dev(gold["X"])
    a = sfv.tsne_project(X)
    b = sfv.tsne_project(X)
    Ya, Yb = a.embedding.cpu().numpy(), b.embedding.cpu().numpy()
    assert Ya.dtype == np.float32 and Ya.shape == (len(gold["X"]), 2) and np.isfinite(Ya).all()
    assert np.array_equal(Ya.view(np.int32), Yb.view(np.int32)), "two runs differ"
    assert (a.kl_divergence, a.n_iter) == (b.kl_divergence, b.n_iter)
    kl = R.kl_of(Ya, *_csr(gold))
    trust = trustworthiness(gold["X"], Ya, n_neighbors=24)
    print(f"whole run: n_iter {a.n_iter}, device KL {a.kl_divergence:.5f}, f64 KL under scikit-learn's P {kl:.5f} "
          f"(scikit-learn {float(gold['tsne_kl']):.5f}), trustworthiness {trust:.5f} (scikit-learn "
          f"{float(gold['tsne_trust']):.5f})")
    assert a.n_iter == int(gold["tsne_n_iter"]) == 999
    assert abs(a.kl_divergence - kl) <= 1e-3 * kl           # the device's figure is the KL before the last update
    assert kl <= 1.05 * float(gold["tsne_kl"])
    assert trust >= float(gold["tsne_trust"]) - 0.005


def test_affinities_against_sklearn(gold, graph):
    idx, d2 = sfv.knn_graph(_dev(gold["X"]), K)
    aff = sfv.tsne_affinities(idx, d2, PERPLEXITY)
    assert np.array_equal(aff.indptr.cpu().numpy(), gold["joint_indptr"])
    assert np.array_equal(aff.indices.cpu().numpy(), gold["joint_indices"])
    assert aff.data.dtype == torch.float32
    assert np.abs(aff.data.cpu().numpy().astype(np.float64) / gold["joint_data"] - 1.0).max() <= 1e-7
    assert np.array_equal(aff.steps.cpu().numpy(), graph["steps"])


# ---- PCA ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,Ld", [(2, 1), (320, 50), (700, 128), (1000, 7)])
def test_pca_moments(gold, N, Ld):
    X = gold["X"] if (N, Ld) == (320, 50) else np.random.RandomState(N).randn(N, Ld).astype(np.float32) * 3 + 1
    mean, cov = Guarded(torch.float64, Ld), Guarded(torch.float64, Ld, Ld)
    sfv._lib.call("rbvae_pca_moments", _dev(X), N, Ld, mean.t, cov.t)
    mh, ch = mean.check("mean"), cov.check("cov")
    rm, _, b_m, _ = R.moments(X)
    wm = R.within(mh, rm, b_m, "mean")
    _, rc, _, b_c = R.moments(X, mean=mh)
    wc = R.within(ch, rc, b_c, "covariance")
    print(f"moments ({N}, {Ld}): worst |err|/bound mean {wm:.3g}, covariance {wc:.3g}")
    assert np.array_equal(ch, ch.T)


def test_pca_project_against_sklearn(gold):
    res = sfv.pca_project(_dev(gold["X"]), 2)
    emb = res.embedding.cpu().numpy()
    lim = 100 * 3.4e-14                                     # 100 x the disagreement of scikit-learn's two exact solvers
    d = np.abs(emb - gold["pca_Y"]).max()
    print(f"PCA: max |device - sklearn| {d:.3g} at scale {np.abs(gold['pca_Y']).max():.3g}")
    assert emb.dtype == np.float64 and d <= lim
    assert np.array_equal(np.sign(res.components), np.sign(gold["pca_components"]))
    assert np.abs(res.components - gold["pca_components"]).max() <= lim
    assert np.abs(res.explained_variance - gold["pca_explained_variance"]).max() <= lim
    assert np.abs(res.mean - gold["pca_mean"]).max() <= lim
    out = Guarded(torch.float64, len(emb), 2)
    sfv._lib.call("rbvae_pca_project", _dev(gold["X"]), len(emb), 50, _dev(res.mean), _dev(res.components), 2, out.t)
    assert np.array_equal(out.check("projection").view(np.int64), emb.view(np.int64))


def test_pca_rank_deficient():
    r = np.random.RandomState(8)
    X = (r.randn(100, 6) * np.array([5.0, 3.0, 1.0, 0.5, 0.2, 1.0])).astype(np.float32)
    X[:, 5] = X[:, 2]                                       # a duplicated column: one zero eigenvalue
    res = sfv.pca_project(_dev(X), 2)
    emb, comp, var, _ = R.pca(X, 2)
    assert np.isfinite(res.embedding.cpu().numpy()).all()
    assert np.array_equal(np.sign(res.components), np.sign(comp))
    assert np.abs(res.embedding.cpu().numpy() - emb).max() <= 1e-10 * np.abs(emb).max()
    assert np.abs(res.explained_variance - var).max() <= 1e-12 * var.max()
    mean, cov = sfv.projection.pca_moments(_dev(X))
    w = np.linalg.eigvalsh(cov.cpu().numpy())
    assert abs(w[0]) <= 1e-12 * w[-1]
    c = cov.cpu().numpy()
    assert np.array_equal(c[5], c[2]) and np.array_equal(c[:, 5], c[:, 2])


# ---- arguments ---------------------------------------------------------------------------------------------------------

def test_invalid_arguments():
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")       # noqa: E731
    with pytest.raises(ValueError, match="L=129"):
        sfv.knn_graph(z(4, 129), 2)
    with pytest.raises(ValueError, match="k=4"):
        sfv.knn_graph(z(4, 3), 4)
    with pytest.raises(ValueError, match="k=129"):
        sfv.knn_graph(z(200, 3), 129)
    with pytest.raises(ValueError, match="N=16385"):
        sfv.knn_graph(z(16385, 2), 3)
    with pytest.raises(ValueError, match="contiguous"):
        sfv.knn_graph(z(3, 8).t(), 2)
    with pytest.raises(ValueError, match="GPU"):
        sfv.knn_graph(z(8, 3).cpu(), 2)
    with pytest.raises(ValueError, match="float32"):
        sfv.knn_graph(z(8, 3).double(), 2)
    bad = z(8, 3)
    bad[2, 1] = float("nan")
    with pytest.raises(ValueError, match="NaN"):
        sfv.knn_graph(bad, 3)
    idx, d2 = sfv.knn_graph(z(8, 3), 3)
    with pytest.raises(ValueError, match="outside"):
        sfv.projection.joint_csr(np.full((8, 3), 8, dtype=np.int32), np.ones((8, 3)))
    for p in (3.0, 4.5, 0.0):
        with pytest.raises(ValueError, match="perplexity"):
            sfv.tsne_affinities(idx, d2, p)
    with pytest.raises(ValueError, match="perplexity"):
        sfv.tsne_project(z(8, 3), perplexity=8.0)
    with pytest.raises(ValueError, match="max_iter"):
        sfv.tsne_project(z(40, 3), perplexity=5.0, max_iter=100)
    with pytest.raises(ValueError, match="GPU"):
        sfv.pca_project(z(8, 3).cpu())
    with pytest.raises(ValueError, match="n_components"):
        sfv.pca_project(z(8, 3), 4)
    with pytest.raises(ValueError, match="L=129"):
        sfv.pca_project(z(8, 129), 2)
    # a refused call launches nothing: the outputs keep their sentinels
    out_i, out_d = Guarded(torch.int32, 4, 2), Guarded(torch.float64, 4, 2)
    with pytest.raises(ValueError, match="L=129"):
        sfv._lib.call("rbvae_knn", z(4, 129), 4, 129, 2, out_i.t, out_d.t)
    with pytest.raises(ValueError, match="null"):
        sfv._lib.call("rbvae_knn", z(4, 3), 4, 3, 2, None, out_d.t)
    out_i.check("idx", untouched=True)
    out_d.check("d2", untouched=True)
    y, f, d, i = z(8, 2), z(64), torch.zeros(64, dtype=torch.float64, device="cuda"), \
        torch.zeros(64, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="Y_out"):
        sfv._lib.call("rbvae_tsne_step", y, y, f, f, i, i, f, f, d, f, 8, d)
    with pytest.raises(ValueError, match="N=1"):
        sfv._lib.call("rbvae_tsne_step", y, z(8, 2), f, f, i, i, f, f, d, f, 1, d)
    with pytest.raises(ValueError, match="N=0"):
        sfv._lib.call("rbvae_tsne_repulse", y, 0, f)
    with pytest.raises(ValueError, match="N=1"):
        sfv._lib.call("rbvae_pca_moments", y, 1, 2, d, d)


# ---- the script's loop -------------------------------------------------------------------------------------------------

def test_latent_projections():
    F_, RES, LD = 48, 64, 16
    torch.manual_seed(0)
    model = sfv.Seq2SeqBinaryVAE(3, 3, LD, LD, variant="contrastive", input_hw=(RES, RES), compute_dtype="f32").cuda().eval()
    x = torch.rand(F_, 3, RES, RES, generator=torch.Generator().manual_seed(1)).cuda()
    u = torch.rand(F_, LD, generator=torch.Generator().manual_seed(2))
    flags = [10, 30]
    out = sfv.latent_projections(model, x, u=u, frame_indices=range(F_), flags=flags, perplexity=5.0, max_iter=250)
    z = model.encode(x[:, None], temperature=0.2, hard=False, noise_ratio=0.3, u=u.cuda())[:, 0]
    assert torch.equal(out["latents"], z) and tuple(z.shape) == (F_, LD)
    assert np.array_equal(out["labels"], [sfv.assign_label(f, flags) for f in range(F_)])
    assert torch.equal(out["pca"].embedding, sfv.pca_project(z.contiguous(), 2).embedding)
    assert tuple(out["tsne"].embedding.shape) == (F_, 2) and out["tsne"].n_iter == 249
    assert torch.equal(out["tsne"].embedding, sfv.tsne_project(z.contiguous(), perplexity=5.0, max_iter=250).embedding)
    assert np.isfinite(out["tsne"].kl_divergence) and not model.training
