"""CPU: tests/_kmeans_ref.py (the f64 restatement the GPU tests compare the k-means kernels and symbols.py with) against the
scikit-learn fixture tests/golden/kmeans.npz (tools/make_kmeans_golden.py), each check of the GPU tests against the named
defect it has to reject, and the host side of symbols.py.  Nothing here reads the reference or scikit-learn.

Measured here, over K in {2, 8, 17, 32} x seed in {0, 42}: init indices, labels and n_iter (5 to 15) equal scikit-learn's
and every fit ends "strict"; centres within 4.4e-16 (the gate is 1e-12), inertia within 2.2e-16 relative (1e-12); the six
agreement scores differ by 0.0 from the fixture's on all eight labellings and on lab_edge (1e-15); Davies-Bouldin within
2.3e-14 (K = 2, seed 42; 1.8e-15 for the states) and Calinski-Harabasz within 1.8e-15 (1e-12 both).  The smallest cluster
holds 2 rows; none is empty."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _kmeans_ref as R
import sfv_amd as sfv

HERE = os.path.dirname(os.path.abspath(__file__))
KS, SEEDS = (2, 8, 17, 32), (0, 42)
TOL_CASE = (8, 42, 0.1)                 # K, seed, tol: stops on the centres' shift at iteration 11 instead of strictly at 13


@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(os.path.join(HERE, "golden", "kmeans.npz")))
    g.update({k: v for k, v in np.load(os.path.join(HERE, "golden", "latent_scores.npz")).items() if k in ("X", "lab", "lab_edge")})
    return g


@pytest.fixture(scope="module")
def fits(gold):
    return {(K, s): R.lloyd(gold["X"], gold["X"][gold[f"pp_{K}_{s}"]].astype(np.float64)) for K in KS for s in SEEDS}


def test_fixture_size():
    assert os.path.getsize(os.path.join(HERE, "golden", "kmeans.npz")) <= 200 * 1024


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("K", KS)
def test_fit_equals_sklearn(gold, fits, K, seed):
    t, fit = f"{K}_{seed}", fits[(K, seed)]
    assert np.array_equal(R.kmeans_pp(gold["X"], K, seed), gold["pp_" + t])
    assert np.array_equal(fit["labels"], gold["labels_" + t]) and fit["n_iter"] == int(gold["n_iter_" + t])
    dc = np.abs(fit["centers"] - gold["centers_" + t]).max()
    di = abs(fit["inertia"] / float(gold["inertia_" + t]) - 1.0)
    print(f"K = {K}, seed {seed}: {fit['n_iter']} iterations ({fit['converged']}), centres within {dc:.3g}, inertia within "
          f"{di:.3g} relative, smallest cluster {fit['counts'].min()}")
    assert fit["converged"] == "strict" and dc <= 1e-12 and di <= 1e-12 and fit["counts"].min() >= 1
    D = np.sort(R.d2_to(gold["X"], fit["centers"]), axis=1)
    if K > 1:
        assert (D[:, 1] - D[:, 0]).min() > 1e-4             # no row is undecided between two centres


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("K", KS)
def test_scores_equal_sklearn(gold, fits, K, seed):
    t, lab = f"{K}_{seed}", fits[(K, seed)]["labels"]
    ag = R.agreement(R.contingency(gold["lab"], lab, 8, K))
    d = max(abs(ag[n] - gold["agree_" + t][i]) for i, n in enumerate(R.SCORES))
    ddb = abs(R.davies_bouldin(gold["X"], lab) - float(gold["db_" + t]))
    dch = abs(R.calinski_harabasz(gold["X"], lab) - float(gold["ch_" + t]))
    print(f"K = {K}, seed {seed}: ARI {ag['ari']:.4f}, NMI {ag['nmi']:.4f}; agreement within {d:.3g}, DB within {ddb:.3g}, "
          f"CH within {dch:.3g}")
    assert d <= 1e-15 and ddb <= 1e-12 and dch <= 1e-12
    assert 0.05 < ag["ari"] < 0.95 and 0.05 < ag["nmi"] < 0.95      # nothing saturates


def test_scores_of_the_states(gold):
    ag = R.agreement(R.contingency(gold["lab"], gold["lab_edge"]))
    assert max(abs(ag[n] - gold["agree_edge"][i]) for i, n in enumerate(R.SCORES)) <= 1e-15
    for name in ("lab", "lab_edge"):
        assert abs(R.davies_bouldin(gold["X"], gold[name]) - float(gold["db_" + name])) <= 1e-12
        assert abs(R.calinski_harabasz(gold["X"], gold[name]) - float(gold["ch_" + name])) <= 1e-12
    one, two = np.zeros(6, dtype=np.int64), np.array([0, 0, 0, 1, 1, 1])
    assert R.agreement(R.contingency(one, one)) == dict(zip(R.SCORES, (1.0, 1.0, 1.0, 1.0, 1.0, 1.0)))
    assert R.agreement(R.contingency(two, one)) == dict(zip(R.SCORES, (0.0, 0.0, 0.0, 1.0, 0.0, float(np.sqrt(12 / 30) * np.sqrt(12 / 12)))))


@pytest.mark.parametrize("N,Ld,K", R.ASSIGN_CASES)
def test_assign_cases_are_decided(N, Ld, K):
    """the synthetic inputs of the GPU assign test: no row is undecided, and the chunk shapes are what they are meant to be"""
    X, C = R.assign_case(N, Ld, K)
    D = R.d2_to(X, C, R.LD)
    assert R.decided(D, Ld).all()
    assert np.array_equal(R.assign(X, C)[0], np.argmin(D, axis=1))
    R.within(R.assign(X, C)[1], D.min(axis=1), R.d2_bound(Ld, D.min(axis=1)), "f64 d2 against long double")
    if Ld == 128:
        assert R.chunk_centres(Ld) == 32 and (K == 33 or K > 4 * 32)


# ---- the checks reject the named defects -----------------------------------------------------------------------------------

def test_tie_high_rejected():
    X, C = R.tie_case()
    lab, d2 = R.assign(X, C)
    D = R.d2_to(X, C)
    tied = np.sort(D, axis=1)[:, 0] == np.sort(D, axis=1)[:, 1]            # the first twelve centres are six, twice
    assert tied.mean() > 0.5 and not tied.all()
    high = R.assign(X, C, "tie_high")[0]
    assert np.all(high[tied] > lab[tied]) and np.array_equal(high[~tied], lab[~tied])


def test_empty_centre_zeroed_rejected():
    X, C = R.assign_case(300, 128, 33)
    lab = R.update_labels(300, 33, "empty")
    good, n, shift2, _, _ = R.update(X, lab, C)
    bad = R.update(X, lab, C, defect="empty_centre_zeroed")[0]
    empty = n == 0
    assert empty.sum() >= 10 and np.array_equal(good[empty], C[empty]) and np.all(shift2[empty] == 0.0)
    assert not np.array_equal(bad[empty], C[empty])


def test_stopping_defects_rejected(gold, fits):
    K, seed, tol = TOL_CASE
    C0 = gold["X"][gold[f"pp_{K}_{seed}"]].astype(np.float64)
    good = R.lloyd(gold["X"], C0, tol=tol)
    assert good["converged"] == "tol" and good["n_iter"] == 11 < fits[(K, seed)]["n_iter"]
    assert np.array_equal(good["labels"], R.assign(gold["X"], good["centers"])[0])
    assert R.lloyd(gold["X"], C0, tol=tol, defect="shift_not_squared")["n_iter"] != good["n_iter"]
    late = R.lloyd(gold["X"], C0, tol=tol, defect="no_final_assign_after_tol")
    assert late["n_iter"] == good["n_iter"] and not np.array_equal(late["labels"], good["labels"])
    for (k, s), fit in fits.items():
        bad = R.lloyd(gold["X"], gold["X"][gold[f"pp_{k}_{s}"]].astype(np.float64), defect="n_iter_off_by_one")
        assert bad["n_iter"] != int(gold[f"n_iter_{k}_{s}"]) == fit["n_iter"]
    short = R.lloyd(gold["X"], C0, max_iter=3)
    assert short["converged"] == "max_iter" and short["n_iter"] == 3
    assert np.array_equal(short["labels"], R.assign(gold["X"], short["centers"])[0])


def test_kmeans_pp_defects_rejected(gold):
    wrong = [not np.array_equal(R.kmeans_pp(gold["X"], K, s, "pp_first_trial_wins"), gold[f"pp_{K}_{s}"]) for K in KS for s in SEEDS]
    assert sum(wrong) >= 6
    # searchsorted names row N only for a value above the last cumulative sum, which no fixture draw is: shown on the
    # function both implementations draw their candidates with
    closest = R.d2_to(gold["X"], gold["X"][:1])[:, 0]
    vals = np.array([0.0, 0.5, 1.0, 1.0 + 1e-15]) * np.cumsum(closest)[-1]
    good = R.pp_candidates(closest, vals)
    assert good[-1] == 319 and good[0] == 0 and np.all(np.diff(good) >= 0)
    assert np.array_equal(sfv.symbols._pp_candidates(closest, vals), good)
    assert not np.array_equal(R.pp_candidates(closest, vals, "pp_unclipped_index"), good)


@pytest.mark.parametrize("defect,key", [("ari_unadjusted", "ari"), ("nmi_geometric", "nmi")])
def test_agreement_defects_rejected(gold, fits, defect, key):
    i = R.SCORES.index(key)
    for (K, s), fit in fits.items():
        T = R.contingency(gold["lab"], fit["labels"], 8, K)
        assert abs(R.agreement(T, defect)[key] - gold[f"agree_{K}_{s}"][i]) > 1e-9, f"{defect} passes at K = {K}"        # the gate is 1e-15


def test_index_defects_rejected(gold, fits):
    for name, lab in [("lab", gold["lab"]), ("lab_edge", gold["lab_edge"])] + [(f"{K}_{s}", f["labels"]) for (K, s), f in fits.items()]:
        assert abs(R.davies_bouldin(gold["X"], lab, "db_squared_spread") - float(gold["db_" + name])) > 1e-3
        assert abs(R.calinski_harabasz(gold["X"], lab, "ch_dof_swapped") - float(gold["ch_" + name])) > 1e-3


def test_bounds_mean_something(gold, fits):
    """a dropped row or a relative error of 1e-12 is outside the centre and sum bounds; an f64 sum in another order inside"""
    X, fit = gold["X"], fits[(8, 42)]
    lab = fit["labels"]
    C, n, _, _, _ = R.update(X, lab, np.zeros((8, 50)))
    bnd = R.centre_bound(X, lab, C)
    plain = np.stack([X[lab == k][::-1].astype(np.float64).sum(0) / n[k] for k in range(8)])
    R.within(plain, C, bnd, "f64 means in reverse order")
    short = lab.copy()
    short[np.nonzero(lab == 0)[0][0]] = 1
    assert R.rejects(R.update(X, short, np.zeros((8, 50)))[0][0], C[0], bnd[0])
    assert R.rejects(C * (1 + 1e-12), C, bnd)
    d2 = R.assign(X, C)[1]
    _, _, _, wi, sp = R.update(X, lab, C, d2)
    bw, bs = R.sum_bounds(n, wi, sp)
    assert R.rejects(wi * (1 + 1e-12), wi, bw) and R.rejects(sp * (1 + 1e-12), sp, bs)
    R.within(np.array([d2[lab == k][::-1].sum() for k in range(8)]), wi, bw, "f64 within in reverse order")


# ---- the host side of the package ------------------------------------------------------------------------------------------

NEW = ("rbvae_kmeans_ok", "rbvae_kmeans_chunk_centres", "rbvae_kmeans_ws_bytes", "rbvae_kmeans_assign", "rbvae_kmeans_update",
       "rbvae_kmeans_decide", "rbvae_kmeans_pp_trials")


def test_header_and_library():
    protos = sfv._lib.parse_header()
    raw = ctypes.CDLL(sfv._lib.LIB_PATH)
    for name in NEW:
        assert name in protos and hasattr(raw, name), name
    assert [len(protos[n][1]) for n in NEW] == [3, 1, 3, 11, 14, 6, 10]
    q = sfv._lib.query
    assert q("rbvae_kmeans_ok", 12298, 50, 17) == 1 and q("rbvae_kmeans_ok", 1 << 20, 128, 256) == 1
    assert q("rbvae_kmeans_ok", 1, 1, 1) == 1 and q("rbvae_kmeans_ok", (1 << 20) + 1, 2, 2) == 0
    assert q("rbvae_kmeans_ok", 3, 2, 4) == 0 and q("rbvae_kmeans_ok", 300, 129, 4) == 0
    assert q("rbvae_kmeans_ok", 300, 4, 257) == 0 and q("rbvae_kmeans_ok", 300, 0, 4) == 0 and q("rbvae_kmeans_ok", 300, 4, 0) == 0
    for Ld in (1, 3, 50, 128):
        assert q("rbvae_kmeans_chunk_centres", Ld) == R.chunk_centres(Ld)
    assert q("rbvae_kmeans_ws_bytes", 300, 129, 4) == 0
    assert q("rbvae_kmeans_ws_bytes", 12298, 50, 17) == 8 * 49 * 17 * 53
    assert q("rbvae_kmeans_ws_bytes", 1 << 20, 128, 256) == 8 * 256 * 256 * 131
    assert q("rbvae_kmeans_ws_bytes", 1 << 20, 1, 1) == 8 * 8 * 4096      # the k-means++ trials' partial sums


def test_cpu_inputs_raise():
    X, lab = torch.zeros((8, 4)), np.array([0, 0, 0, 0, 1, 1, 1, 1])
    for call in (lambda: sfv.kmeans(X, 2), lambda: sfv.kmeans_plusplus(X, 2), lambda: sfv.code_symbols(X),
                 lambda: sfv.davies_bouldin(X, lab), lambda: sfv.calinski_harabasz(X, lab),
                 lambda: sfv.contingency(torch.from_numpy(lab), torch.from_numpy(lab), 2, 2),
                 lambda: sfv.latent_symbols(None, torch.zeros((2, 3, 8, 8)), [0, 1], [1])):
        with pytest.raises(ValueError, match="GPU"):
            call()
    with pytest.raises(ValueError, match="tensor"):
        sfv.kmeans(np.zeros((8, 4), dtype=np.float32), 2)
    assert sfv.symbols.kmeans is sfv.kmeans and sfv.symbols.MAX_CLUSTERS == 256 and sfv.symbols.ENQUEUE == 8
