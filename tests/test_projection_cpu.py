"""CPU: tests/_projection_ref.py (the f64 restatement the GPU tests compare the kernels with) against the scikit-learn
fixture tests/golden/projection.npz (tools/make_projection_golden.py), the host part of projection.py (the joint CSR,
the argument checks) against the same fixture, and each element-wise bound of the GPU tests against the named defects it
has to reject.  Nothing here reads the reference or scikit-learn."""
import os

import numpy as np
import pytest
import torch

import _projection_ref as R
import sfv_amd as sfv

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "projection.npz")
K, PERPLEXITY = 91, 30.0
# PCA: scikit-learn's two exact solvers (covariance_eigh, LAPACK full) disagree by 3.4e-14 on this fixture at a coordinate
# scale of 2.2; the restatement is the first, the fixture holds the second
PCA_SOLVERS = 3.4e-14


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def graph(gold):
    idx, d2, decided = R.knn(gold["X"], K)
    P, beta, steps, near = R.perplexity_search(d2, PERPLEXITY)
    return {"idx": idx, "d2": d2, "decided": decided, "P": P, "beta": beta, "steps": steps, "near": near}


def test_fixture_is_decided(gold, graph):
    """the neighbour order of every fixture row is decided far above f64 rounding, and no row of the perplexity search
    sits on the tolerance threshold: the GPU tests may exclude such rows but the fixture must have none"""
    assert graph["decided"].all()
    gap = R.smallest_relative_gap(gold["X"], K)
    print(f"smallest relative gap {gap:.3g}")
    assert gap > 1e-9
    assert not graph["near"].any()
    assert os.path.getsize(GOLD) <= 1 << 20


def test_neighbours_identical(gold, graph):
    assert np.array_equal(graph["idx"], gold["nn_idx"])
    assert not np.any(graph["idx"] == np.arange(len(graph["idx"]))[:, None])
    assert np.all(np.diff(graph["d2"], axis=1) >= 0)


def test_conditional_p(gold, graph):
    ref = gold["cond_P"]
    rel = np.abs(graph["P"] - ref) / ref
    print(f"conditional P: worst relative difference {rel.max():.3g}; steps {graph['steps'].min()}..{graph['steps'].max()}")
    assert rel.max() <= 1e-9
    assert np.all(np.abs(graph["P"].sum(1) - 1.0) <= 1e-12)
    assert graph["steps"].max() < 100


def test_joint_csr(gold, graph):
    for name, fn in (("restatement", R.joint_csr), ("projection.joint_csr", sfv.projection.joint_csr)):
        indptr, indices, data = fn(graph["idx"], graph["P"])
        assert np.array_equal(indptr, gold["joint_indptr"]), name
        assert np.array_equal(indices, gold["joint_indices"]), name
        ref = gold["joint_data"]
        assert np.abs(data.astype(np.float64) - ref).max() <= 1e-7 * ref.max(), name
        assert np.abs(data.astype(np.float64) / ref - 1.0).max() <= 1e-7, name
    assert indptr.dtype == np.int32 and indices.dtype == np.int32 and data.dtype == np.float32


def test_gradient_against_sklearn(gold):
    g, kl = R.gradient(gold["Y"], gold["joint_indptr"], gold["joint_indices"], gold["joint_data"].astype(np.float32))
    lim = 1e-6 * np.abs(gold["grad"]).max()
    d = np.abs(g - gold["grad"]).max()
    print(f"gradient: max |restatement - sklearn| {d:.3g} against max |g| {np.abs(gold['grad']).max():.3g}; KL {kl:.7f} "
          f"against {float(gold['error']):.7f}")
    assert d <= lim
    # scikit-learn adds the error's terms in a C float: (n - 1) v sum |terms| at worst
    Zi = R.repulsion(gold["Y"])[1]
    klt = R.attraction(gold["Y"], gold["joint_indptr"], gold["joint_indices"], gold["joint_data"].astype(np.float32), 1.0,
                       Zi.sum())[2]
    assert abs(kl - float(gold["error"])) <= len(klt) * R.V * np.abs(klt).sum()


def test_pca_against_sklearn(gold):
    emb, comp, var, mean = R.pca(gold["X"].astype(np.float64), 2)
    assert np.array_equal(np.sign(comp[np.arange(2), np.abs(comp).argmax(1)]), [1.0, 1.0])
    assert np.array_equal(np.sign(comp), np.sign(gold["pca_components"]))
    d = np.abs(emb - gold["pca_Y"]).max()
    print(f"PCA: max |restatement - sklearn| {d:.3g} at scale {np.abs(gold['pca_Y']).max():.3g}")
    assert d <= PCA_SOLVERS
    assert np.abs(comp - gold["pca_components"]).max() <= PCA_SOLVERS
    assert np.abs(var - gold["pca_explained_variance"]).max() <= PCA_SOLVERS
    assert np.abs(mean - gold["pca_mean"]).max() <= PCA_SOLVERS


# ---- the bounds reject the named defects -------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [257, 700])
@pytest.mark.parametrize("scale", [1e-4, 3.0, 50.0])
@pytest.mark.parametrize("defect", ["self_in_z", "drop_tail", "drop_split"])
def test_repulsion_bound_rejects(N, scale, defect):
    Y = (scale * np.random.RandomState(N).randn(N, 2)).astype(np.float32)
    R_, Z, S_R, S_Z = R.repulsion(Y)
    assert R.repulse_shape(N)[0] > 1
    bR, bZ = R.repulsion_bound(N, S_R), R.repulsion_bound(N, S_Z)
    assert not R.rejects(R_, R_, bR) and not R.rejects(Z, Z, bZ)
    Rd, Zd, _, _ = R.repulsion(Y, defect)
    assert R.rejects(Zd, Z, bZ), f"{defect} passes the Z bound"
    if defect != "self_in_z":                               # the j = i term of R is zero
        assert R.rejects(Rd, R_, bR), f"{defect} passes the R bound"
    # an f32 evaluation in another order stays inside
    y = Y.astype(np.float32)
    d = y[:, None, :] - y[None, :, :]
    q = np.float32(1.0) / (np.float32(1.0) + (d * d).sum(-1, dtype=np.float32))
    np.fill_diagonal(q, 0.0)
    R.within(((q * q)[:, :, None] * d).sum(1, dtype=np.float32), R_, bR, "f32 R")
    R.within(q.sum(1, dtype=np.float32), Z, bZ, "f32 Z")


def test_tie_rule_rejected():
    X = R.hard_codes()
    idx, d2, decided = R.knn(X, 64)
    assert decided.all() and np.any(d2 == 0.0) and np.all(d2 == np.round(d2))
    assert np.any(np.diff(d2, axis=1) == 0)
    bad, _, _ = R.knn(X, 64, defect="tie_high")
    assert not np.array_equal(bad, idx)


def test_gains_sign_rejected(gold):
    N = len(gold["Y"])
    rng = np.random.RandomState(3)
    update = (0.05 * rng.randn(N, 2)).astype(np.float32)
    gains = (0.5 + rng.rand(N, 2)).astype(np.float32)
    Rr, Zi, _, _ = R.repulsion(gold["Y"])
    part = np.concatenate([Rr, Zi[:, None]], axis=1).astype(np.float32)[None]
    args = (gold["Y"], update, gains, gold["joint_indptr"], gold["joint_indices"], gold["joint_data"].astype(np.float32),
            (12.0, 0.5, 200.0), part, float(Zi.sum()))
    good, bad = R.step(*args), R.step(*args, defect="wrong_sign")
    assert not good["free"].any()
    assert np.any(good["gains"] != bad["gains"])
    assert R.rejects(bad["update"], good["update"], good["b_u"]) and R.rejects(bad["Y"], good["Y"], good["b_y"])
    # the bounds are tight enough to mean something: a relative error of 1e-4 in g is outside
    assert R.rejects(good["g"] * (1 + 1e-4), good["g"], good["b_g"])
    assert good["b_kl"] <= 1e-5 * abs(good["kl"]) and good["b_gg"] <= 1e-4 * good["gg"]


# ---- the host side of the package --------------------------------------------------------------------------------------

def test_cpu_inputs_raise():
    X = torch.zeros((8, 4))
    with pytest.raises(ValueError, match="GPU"):
        sfv.knn_graph(X, 3)
    with pytest.raises(ValueError, match="GPU"):
        sfv.pca_project(X)
    with pytest.raises(ValueError, match="GPU"):
        sfv.tsne_project(X, perplexity=2.0)
    with pytest.raises(ValueError, match="GPU"):
        sfv.tsne_affinities(torch.zeros((8, 3), dtype=torch.int32), torch.zeros((8, 3), dtype=torch.float64), 2.0)
    with pytest.raises(ValueError, match="GPU"):
        sfv.latent_projections(None, torch.zeros((2, 3, 8, 8)))
    with pytest.raises(ValueError, match="tensor"):
        sfv.knn_graph(np.zeros((8, 4), dtype=np.float32), 3)
    for name in ("rbvae_knn", "rbvae_knn_ok", "rbvae_tsne_perplexity", "rbvae_tsne_repulse", "rbvae_tsne_repulse_splits",
                 "rbvae_tsne_zsum", "rbvae_tsne_step", "rbvae_tsne_step_parts", "rbvae_pca_moments", "rbvae_pca_project"):
        assert name in sfv._lib.parse_header()
    q = sfv._lib.query
    assert q("rbvae_knn_ok", 12298, 50, 91) == 1 and q("rbvae_knn_ok", 16384, 128, 128) == 1
    assert q("rbvae_knn_ok", 16385, 50, 91) == 0 and q("rbvae_knn_ok", 100, 129, 9) == 0
    assert q("rbvae_knn_ok", 10, 4, 10) == 0 and q("rbvae_knn_ok", 2, 1, 1) == 1
    for N in (1, 2, 63, 64, 257, 700, 12298, 16384):
        assert q("rbvae_tsne_repulse_splits", N) == R.repulse_shape(N)[0]
