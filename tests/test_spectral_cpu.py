"""CPU: tests/_spectral_ref.py's restatement of the spectral kernels and solver against independent yardsticks (a dense
numpy.linalg.eigh, closed forms, scikit-learn's spectral_embedding, all recorded in tests/golden/spectral.npz by
tools/make_spectral_golden.py), through the gates the GPU tests put the device through, and each named defect of the
restatement rejected by one of those gates."""
import os

import numpy as np
import pytest

import _spectral_ref as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-10
EIGEN_TOL = 1e-12                                           # ARPACK's, in the golden scikit-learn embedding


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "spectral.npz")))


def _csr(gold, nn):
    return gold[f"indptr_{nn}"], gold[f"indices_{nn}"], gold[f"data_{nn}"]


@pytest.fixture(scope="module")
def solved(gold):
    """the restated embedding solve (q0 locked, 8 pairs) of both fixture graphs, shared and left unchanged"""
    return {nn: S.spectral_embedding(*_csr(gold, nn), 8) for nn in (24, 15)}


def test_golden_is_what_the_tool_writes(gold):
    X = np.load(os.path.join(GOLDEN, "latent_scores.npz"))["X"]
    for nn in (24, 15):
        csr = S.fuzzy_fixture(X, nn)
        want = _csr(gold, nn)
        assert np.array_equal(csr[0], want[0]) and np.array_equal(csr[1], want[1])
        assert np.abs(csr[2].astype(np.float64) / want[2] - 1.0).max() <= 4 * 2.0 ** -24    # another libm's exp
        lam, vec, _ = S.dense_eigh(*csr, 12)
        assert np.abs(lam - gold[f"lam_{nn}"]).max() <= 320 * 2.0 ** -52 + 8 * 2.0 ** -24     # and its weights
    assert len(gold["cl_K"]) >= 2 and set(gold["cl_K"].tolist()) >= {2, 8}


@pytest.mark.parametrize("nn", [24, 15])
def test_dense_eigenvalues_and_vectors(gold, solved, nn):
    _, r = solved[nn]
    N = len(gold[f"indptr_{nn}"]) - 1
    assert r["converged"] and r["why"] == "tol" and r["steps"] <= 104
    ge = S.eigenvalue_gate(r["eigenvalues"], gold[f"lam_{nn}"][1:9], TOL, N)
    gv = S.vector_gate(r["vectors"], r["residuals"], gold[f"vec_{nn}"], gold[f"lam_{nn}"], range(1, 9), N)
    go = S.orth_gate(r["vectors"], 1, r["steps"])
    print(f"n_neighbors {nn}: {r['steps']} steps, worst |err|/bound eigenvalues {ge:.3g}, vectors {gv:.3g}, "
          f"orthonormality {go:.3g}, largest residual {r['residuals'].max():.3g}")
    assert ge <= 1 and gv <= 1 and go <= 1
    assert np.all(r["residuals"] <= S.residual_cap(TOL, 1, r["steps"], N, int(np.diff(gold[f"indptr_{nn}"]).max())))


def test_layout_is_eigenvectors_one_and_two(gold):
    lay, r = S.spectral_layout(*_csr(gold, 24), 2)
    assert S.vector_gate(lay, r["residuals"], gold["vec_24"], gold["lam_24"], (1, 2), 320) <= 1
    q0 = S.trivial_vector(*_csr(gold, 24))
    assert np.abs(q0 - gold["vec_24"][:, 0]).max() <= 320 * 2.0 ** -52 / gold["lam_24"][1]


@pytest.mark.parametrize("n", [64, 1000])
def test_path_graph_closed_form(n):
    csr = S.path_graph(n)
    r = S.lanczos(*csr, 4, fast=n > 64)
    assert S.eigenvalue_gate(r["eigenvalues"], S.path_eigenvalues(n, 4), TOL, n) <= 1
    assert np.all(r["residuals"] <= S.residual_cap(TOL, 0, r["steps"], n, 2))


def test_path_graph_breaks_down_with_the_full_spectrum():
    n = 64
    csr = S.path_graph(n)
    r = S.lanczos(*csr, n - 1, locked=S.trivial_vector(*csr), max_steps=n - 1)
    assert r["why"] == "invariant" and r["converged"] and r["steps"] == n - 1
    assert S.eigenvalue_gate(r["eigenvalues"], S.path_eigenvalues(n, n)[1:], TOL, n) <= 1


def test_complete_graph_and_cycle():
    r = S.lanczos(*S.complete_graph(8), 2)
    assert r["why"] == "invariant" and r["converged"] and r["steps"] == 2
    assert S.eigenvalue_gate(r["eigenvalues"], [0.0, 8.0 / 7.0], TOL, 8) <= 1
    r = S.lanczos(*S.complete_graph(8), 3)
    assert r["why"] == "invariant" and not r["converged"] and len(r["eigenvalues"]) == 2 and r["vectors"].shape == (8, 2)
    lay, r = S.spectral_layout(*S.cycle_graph(6), 2)
    assert r["steps"] >= 2                                  # q0 locked: the regular graph does not break down at step 1
    assert abs(r["eigenvalues"][0] - (1 - np.cos(2 * np.pi / 6))) <= TOL + 6 * 2.0 ** -52 and r["residuals"][0] <= TOL


def _sk_gate_cols(emb, r, gold, nn, N):
    """scikit-learn's array holds eigenvectors 1..8 over sqrt(deg): Davis-Kahan with ARPACK's tolerance added, scaled by
    the largest 1 / sqrt(deg)"""
    ref = gold[f"sk_emb_{nn}"]
    if emb.shape != ref.shape:
        return np.inf
    bound = r["isd"].max() * S.davis_kahan(r["residuals"] + EIGEN_TOL, S.gaps(gold[f"lam_{nn}"], range(1, 9)), N)
    return float(np.max(np.linalg.norm(emb - ref, axis=0) / bound))


@pytest.mark.parametrize("nn", [24, 15])
def test_scikit_learn_convention(gold, solved, nn):
    emb, r = solved[nn]
    g = _sk_gate_cols(emb, r, gold, nn, 320)
    print(f"n_neighbors {nn}: worst |err|/bound against sklearn.manifold.spectral_embedding {g:.3g}")
    assert g <= 1
    full, _ = S.spectral_embedding(*_csr(gold, nn), 3, drop_first=False)
    assert full.shape == (320, 3) and np.ptp(full[:, 0]) <= 4 * S.U * full[0, 0] and full[0, 0] > 0
    assert np.abs(full[:, 1:] - emb[:, :2]).max() <= 1e-9


# ---- the named defects, each through a gate of the GPU tests --------------------------------------------------------------

def test_defect_no_reorth_grows_ghosts(gold):
    csr = _csr(gold, 24)
    r = S.lanczos(*csr, 9, tol=0.0, max_steps=88, defect="no_reorth")
    good = S.lanczos(*csr, 9, tol=0.0, max_steps=88)
    assert S.eigenvalue_gate(good["eigenvalues"], gold["lam_24"][:9], TOL, 320) <= 1
    assert S.eigenvalue_gate(r["eigenvalues"], gold["lam_24"][:9], TOL, 320) > 1
    assert np.sum(np.abs(r["eigenvalues"]) < 1e-6) >= 2     # ghost copies of the top eigenvalue of S


def test_defect_single_pass_gs_is_not_separated(gold):
    """one Gram-Schmidt pass: on this fixture the vectors stay orthonormal well inside the bound on |Y^T Y - I| and the
    eigenvalues inside theirs, so no gate is claimed to reject it (the second pass is there for graphs with tighter
    clusters of eigenvalues, where one pass loses orthogonality)"""
    csr = _csr(gold, 24)
    r = S.lanczos(*csr, 8, locked=S.trivial_vector(*csr), defect="single_pass_gs")
    assert S.orth_gate(r["vectors"], 1, r["steps"]) <= 1
    assert S.eigenvalue_gate(r["eigenvalues"], gold["lam_24"][1:9], TOL, 320) <= 1


def test_defect_alpha_first_pass_only(gold):
    """on a basis that is orthonormal only to 1e-6 the second pass's coefficient on v_j is about 1e-6"""
    csr = _csr(gold, 24)
    base = S.lanczos(*csr, 3, tol=0.0, max_steps=8, keep_basis=True)
    V = base["V"].copy()
    V[:6] += 1e-6 * np.random.RandomState(5).randn(6, 320)
    good = S.step(csr, base["isd"], V, 0, 5)
    bad = S.step(csr, base["isd"], V, 0, 5, defect="alpha_first_pass_only")
    assert abs(bad["alpha"] - good["alpha"]) > (1 + 1e-5) * good["D_a"] > 0
    assert np.abs(bad["v"] - good["v"]).max() == 0


def test_defect_chunk_tail_dropped():
    N = 70
    W = np.zeros((N, N))
    W[0, 1:66] = W[1:66, 0] = 0.5 + 0.5 * np.random.RandomState(1).rand(65)     # row 0 has 65 edges
    csr = S.to_csr(W)
    isd = S.degree(*csr)[1]
    x = np.random.RandomState(2).randn(N)
    y, b = S.matvec(*csr, isd, x)
    exact = S.matvec_exact(*csr, isd, x)
    assert np.all(np.abs(y - exact) <= b)
    bad, _ = S.matvec(*csr, isd, x, defect="chunk_tail_dropped")
    assert np.abs(bad[0] - exact[0]) > b[0] and np.all(np.abs(bad[66:] - exact[66:]) <= b[66:])


def test_defects_of_the_conventions(gold, solved):
    csr = _csr(gold, 24)
    lam, vec = gold["lam_24"], gold["vec_24"]
    for defect in ("unnormalised_laplacian", "keeps_first"):
        lay, r = S.spectral_layout(*csr, 2, defect=defect)
        res = r.get("residuals", np.full(2, TOL))
        assert S.vector_gate(lay, res, vec, lam, (1, 2), 320) > 1, defect
    emb, r = solved[24]
    bad, rb = S.spectral_embedding(*csr, 8, defect="divide_by_deg")
    assert _sk_gate_cols(bad, rb, gold, 24, 320) > 1
    first_negative = [i for i in range(1, 9) if vec[0, i] < 0]
    assert first_negative, "no reference eigenvector starts with a negative entry: the defect cannot show"
    bad = S.lanczos(*csr, 8, locked=S.trivial_vector(*csr), defect="sign_by_first_entry")
    assert S.vector_gate(bad["vectors"], bad["residuals"], vec, lam, range(1, 9), 320) > 1


def test_kernel_restatements_against_extended_precision():
    r = np.random.RandomState(0)
    for N, nv in ((1023, 1), (1025, 65), (3073, 2)):
        V, w = r.randn(nv, N), r.randn(N)
        c, b = S.dots(V, w)
        exact = (V.astype(np.longdouble) * w.astype(np.longdouble)).sum(1)
        assert np.all(np.abs(c - exact) <= b)
        cc = r.randn(nv)
        out, bw = S.update(V, cc, w)
        exact = w.astype(np.longdouble) - (cc.astype(np.longdouble)[:, None] * V.astype(np.longdouble)).sum(0)
        assert np.all(np.abs(out - exact) <= bw)
