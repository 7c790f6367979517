"""Write tests/golden/spectral.npz: what the spectral tests hold the device to, from numpy, scipy, scikit-learn and the
f64 references under tests/ alone (no GPU, nothing of the package).  On tests/golden/latent_scores.npz's X, for
n_neighbors = 24 (suffix _24) and 15 (suffix _15):
  indptr, indices, data   the fuzzy graph (tests/_umap_ref.py's smooth kNN distances and union)
  lam, vec                numpy.linalg.eigh of the dense L = I - D^-1/2 W D^-1/2: the 12 lowest eigenpairs, sign-fixed
  sk_emb                  sklearn.manifold.spectral_embedding(W, 8, eigen_solver="arpack", eigen_tol=1e-12, random_state=0)
and for n_neighbors = 24 only:
  cl_K, cl_seed, cl_labels   the reference clustering: the dense eigh vectors 0..K-1 times 1 / sqrt(deg), sign-flipped,
                          rounded to f32, KMeans(K, n_init=1, random_state=seed).  Only (K, seed) pairs are kept whose labels
                          are the same on every row when ARPACK's vectors (eigen_tol 1e-12) replace eigh's: the reference
                          is then stable under a perturbation of the size any correct solver makes
  a, b, Y0, ce_init, trust_init, seq_seeds, seq_ce, seq_trust
                          as tests/golden/umap.npz records them for the PCA start, from the spectral initial map
                          (_umap_ref.initial_map of eigenvectors 1..2, seed 42): five _umap_ref.layout_sequential runs

    python tools/make_spectral_golden.py [--seeds 42 43 44 45 46] [--jobs 5]
"""
import argparse
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import _spectral_ref as S  # noqa: E402
import _umap_ref as R  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
N_NEIGHBORS, MIN_DIST, N_EIG, N_EMB = 24, 0.25, 12, 8
CANDIDATES = [(K, seed) for K in (2, 3, 4, 8) for seed in (0, 1, 2)]


def _X():
    return np.load(os.path.join(GOLDEN, "latent_scores.npz"))["X"]


def _scipy(csr, N):
    from scipy.sparse import csr_matrix
    return csr_matrix((csr[2].astype(np.float64), csr[1], csr[0]), shape=(N, N))


def _problem():
    X = _X()
    csr = S.fuzzy_fixture(X, N_NEIGHBORS)
    a, b = R.find_ab(1.0, MIN_DIST)
    _, vec, _ = S.dense_eigh(*csr, 3)
    return X, csr, a, b, R.initial_map(vec[:, 1:3], 42)


def _run(seed):
    from sklearn.manifold import trustworthiness
    X, csr, a, b, Y0 = _problem()
    n_epochs = R.default_epochs(len(X))
    ip, ix, period, _, _ = R.schedule(*csr, n_epochs)
    Y = R.layout_sequential(Y0, ip, ix, period, n_epochs, a, b, seed=seed)
    return R.cross_entropy(Y, *csr, a, b), float(trustworthiness(X, Y, n_neighbors=N_NEIGHBORS))


def _cluster_inputs(csr, N):
    """the f32 embeddings of the reference pipeline from eigh's vectors and from ARPACK's, all N_EMB + 1 columns"""
    from scipy.sparse.linalg import eigsh
    _, vec, _ = S.dense_eigh(*csr, N_EMB + 1)
    isd = S.degree(*csr)[1]
    Sm = _scipy(csr, N).multiply(isd[:, None]).multiply(isd[None, :]).tocsr()
    v0 = np.random.RandomState(0).uniform(-1, 1, N)
    th, av = eigsh(Sm, k=N_EMB + 1, which="LA", tol=1e-12, v0=v0)
    av = av[:, np.argsort(-th)]
    return [S.sign_fix((v * isd[:, None]).T).T.astype(np.float32) for v in (vec, av)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, nargs="+", default=[42, 43, 44, 45, 46])
    ap.add_argument("--jobs", type=int, default=5)
    args = ap.parse_args()
    from sklearn.cluster import KMeans
    from sklearn.manifold import spectral_embedding, trustworthiness
    X = _X()
    N = len(X)
    out = {}
    for nn in (24, 15):
        csr = S.fuzzy_fixture(X, nn)
        lam, vec, _ = S.dense_eigh(*csr, N_EIG)
        sk = spectral_embedding(_scipy(csr, N), n_components=N_EMB, eigen_solver="arpack", eigen_tol=1e-12, random_state=0)
        out.update({f"indptr_{nn}": csr[0], f"indices_{nn}": csr[1], f"data_{nn}": csr[2], f"lam_{nn}": lam,
                    f"vec_{nn}": vec, f"sk_emb_{nn}": sk})
        print(f"n_neighbors {nn}: {len(csr[1])} directed edges, largest row {np.diff(csr[0]).max()}, lowest eigenvalues "
              f"{np.array2string(lam[:4], precision=6)}", flush=True)
    csr = tuple(out[f"{n}_24"] for n in ("indptr", "indices", "data"))
    dense, arpack = _cluster_inputs(csr, N)
    kept = []
    for K, seed in CANDIDATES:
        la = KMeans(K, n_init=1, random_state=seed).fit(dense[:, :K]).labels_
        lb = KMeans(K, n_init=1, random_state=seed).fit(arpack[:, :K]).labels_
        same = bool(np.array_equal(la, lb))
        print(f"clustering K = {K}, seed {seed}: eigh and ARPACK labels {'agree' if same else 'DIFFER: dropped'}, "
              f"sizes {np.bincount(la).tolist()}", flush=True)
        if same:
            kept.append((K, seed, la))
    _, csr_, a, b, Y0 = _problem()
    ce0, tr0 = R.cross_entropy(Y0, *csr, a, b), float(trustworthiness(X, Y0, n_neighbors=N_NEIGHBORS))
    print(f"spectral initial map: cross entropy {ce0:.1f}, trustworthiness {tr0:.5f}", flush=True)
    with multiprocessing.Pool(args.jobs) as pool:
        res = pool.map(_run, args.seeds)
    for s, (ce, tr) in zip(args.seeds, res):
        print(f"seed {s}: cross entropy {ce:.1f}, trustworthiness {tr:.5f}")
    np.savez_compressed(os.path.join(GOLDEN, "spectral.npz"), **out, cl_K=np.array([k[0] for k in kept]),
                        cl_seed=np.array([k[1] for k in kept]), cl_labels=np.array([k[2] for k in kept], dtype=np.int32),
                        a=a, b=b, Y0=Y0, ce_init=ce0, trust_init=tr0, seq_seeds=np.array(args.seeds),
                        seq_ce=np.array([r[0] for r in res]), seq_trust=np.array([r[1] for r in res]))
    print(f"mean cross entropy {np.mean([r[0] for r in res]):.1f}, mean trustworthiness "
          f"{np.mean([r[1] for r in res]):.5f}")


if __name__ == "__main__":
    main()
