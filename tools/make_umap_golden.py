"""Write tests/golden/umap.npz: what the UMAP tests hold the device to, from tests/_umap_ref.py, scipy and
scikit-learn alone (no GPU, nothing of the package).  Recorded results only:
  a, b                    scipy's curve fit at min_dist 0.25, spread 1
  rho, sigma, indptr, indices, data
                          the fuzzy graph of tests/golden/projection.npz's X at n_neighbors = 24
  Y0                      the initial map (exact PCA, seed 42)
  ce_init, trust_init     its fuzzy-set cross entropy and trustworthiness(n_neighbors=24)
  seq_seeds, seq_ce, seq_trust
                          the same two figures after _umap_ref.layout_sequential (umap-learn's edge-by-edge loop in f64,
                          500 epochs) with five seeds of negatives, well under a minute each

    python tools/make_umap_golden.py [--seeds 42 43 44 45 46] [--jobs 5]
"""
import argparse
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import _projection_ref as P  # noqa: E402
import _umap_ref as R  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
N_NEIGHBORS, MIN_DIST = 24, 0.25


def _problem():
    X = np.load(os.path.join(GOLDEN, "projection.npz"))["X"]
    a, b = R.find_ab(1.0, MIN_DIST)
    idx, d2, _ = P.knn(X, N_NEIGHBORS - 1)
    sm = R.smooth_knn(d2)
    csr = R.fuzzy_csr(idx, sm["w"].astype(np.float32))
    Y0 = R.initial_map(P.pca(X.astype(np.float32), 2)[0], 42)
    return X, a, b, sm, csr, Y0


def _run(seed):
    from sklearn.manifold import trustworthiness
    X, a, b, _, csr, Y0 = _problem()
    n_epochs = R.default_epochs(len(X))
    ip, ix, period, _, _ = R.schedule(*csr, n_epochs)
    Y = R.layout_sequential(Y0, ip, ix, period, n_epochs, a, b, seed=seed)
    return R.cross_entropy(Y, *csr, a, b), float(trustworthiness(X, Y, n_neighbors=N_NEIGHBORS))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, nargs="+", default=[42, 43, 44, 45, 46])
    ap.add_argument("--jobs", type=int, default=5)
    args = ap.parse_args()
    from sklearn.manifold import trustworthiness
    X, a, b, sm, csr, Y0 = _problem()
    ce0, tr0 = R.cross_entropy(Y0, *csr, a, b), float(trustworthiness(X, Y0, n_neighbors=N_NEIGHBORS))
    print(f"a {a:.6f} b {b:.6f}; {len(csr[1])} directed edges, largest row {np.diff(csr[0]).max()}; steps "
          f"{sm['steps'].min()}..{sm['steps'].max()}; initial map: cross entropy {ce0:.1f}, trustworthiness {tr0:.5f}",
          flush=True)
    with multiprocessing.Pool(args.jobs) as pool:
        res = pool.map(_run, args.seeds)
    for s, (ce, tr) in zip(args.seeds, res):
        print(f"seed {s}: cross entropy {ce:.1f}, trustworthiness {tr:.5f}")
    np.savez_compressed(os.path.join(GOLDEN, "umap.npz"), a=a, b=b, rho=sm["rho"].astype(np.float32),
                        sigma=sm["sigma"].astype(np.float32), indptr=csr[0], indices=csr[1], data=csr[2], Y0=Y0,
                        ce_init=ce0, trust_init=tr0, seq_seeds=np.array(args.seeds), seq_ce=np.array([r[0] for r in res]),
                        seq_trust=np.array([r[1] for r in res]))
    print(f"mean cross entropy {np.mean([r[0] for r in res]):.1f}, mean trustworthiness "
          f"{np.mean([r[1] for r in res]):.5f}")


if __name__ == "__main__":
    main()
