"""Writes tests/golden/kmeans.npz from scikit-learn 1.7.2 alone (the reference is not involved): what
symbols-from-video_amd/symbols.py and tests/_kmeans_ref.py are pinned to.

    python tools/make_kmeans_golden.py

Input: X, lab and lab_edge of tests/golden/latent_scores.npz (tools/make_scores_golden.py); only results are stored.
    pp_K_S                  kmeans_plusplus(X64, K, random_state=S)'s indices, K in KS, S in SEEDS
    labels_K_S, centers_K_S, inertia_K_S, n_iter_K_S
                            KMeans(K, init=X64[pp_K_S], n_init=1, algorithm="lloyd", tol=1e-4).fit(X64)
    agree_K_S               adjusted_rand_score, normalized_mutual_info_score, homogeneity, completeness, v_measure and
                            fowlkes_mallows_score of lab against labels_K_S, in that order; agree_edge: of lab against lab_edge
    db_*, ch_*              davies_bouldin_score and calinski_harabasz_score of X64 for lab, lab_edge and each labels_K_S
    sym_m, uniq_m, cnt_m    np.unique(X[:, :m] > 0.5, axis=0, return_inverse=True, return_counts=True), m in (1, 6, 50)
"""
import os

import numpy as np
import sklearn
from sklearn.cluster import KMeans, kmeans_plusplus
from sklearn.metrics import (adjusted_rand_score, calinski_harabasz_score, davies_bouldin_score, fowlkes_mallows_score,
                             homogeneity_completeness_v_measure, normalized_mutual_info_score)

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
KS, SEEDS, BITS = (2, 8, 17, 32), (0, 42), (1, 6, 50)


def six(a, b):
    h, c, v = homogeneity_completeness_v_measure(a, b)
    return np.array([adjusted_rand_score(a, b), normalized_mutual_info_score(a, b), h, c, v, fowlkes_mallows_score(a, b)])


def main():
    assert sklearn.__version__ == "1.7.2", sklearn.__version__
    src = np.load(os.path.join(GOLDEN, "latent_scores.npz"))
    X, lab, lab_edge = src["X"], src["lab"], src["lab_edge"]
    X64 = X.astype(np.float64)
    out, said = {}, []
    for name, labels in (("lab", lab), ("lab_edge", lab_edge)):
        out["db_" + name] = np.float64(davies_bouldin_score(X64, labels))
        out["ch_" + name] = np.float64(calinski_harabasz_score(X64, labels))
    out["agree_edge"] = six(lab, lab_edge)
    for K in KS:
        for seed in SEEDS:
            _, idx = kmeans_plusplus(X64, K, random_state=seed)
            km = KMeans(K, init=X64[idx].copy(), n_init=1, algorithm="lloyd", tol=1e-4).fit(X64.copy())
            t = f"{K}_{seed}"
            out["pp_" + t] = idx.astype(np.int32)
            out["labels_" + t] = km.labels_.astype(np.int32)
            out["centers_" + t] = km.cluster_centers_
            out["inertia_" + t] = np.float64(km.inertia_)
            out["n_iter_" + t] = np.int32(km.n_iter_)
            out["agree_" + t] = six(lab, km.labels_)
            out["db_" + t] = np.float64(davies_bouldin_score(X64, km.labels_))
            out["ch_" + t] = np.float64(calinski_harabasz_score(X64, km.labels_))
            said.append(f"K={K} seed={seed}: {km.n_iter_} iterations, inertia {km.inertia_:.4f}, smallest cluster "
                        f"{np.bincount(km.labels_, minlength=K).min()}, ARI {out['agree_' + t][0]:.3f}, NMI "
                        f"{out['agree_' + t][1]:.3f}, DB {out['db_' + t]:.4f}, CH {out['ch_' + t]:.4f}")
    for m in BITS:
        u, inv, cnt = np.unique(X[:, :m] > 0.5, axis=0, return_inverse=True, return_counts=True)
        out[f"uniq_{m}"], out[f"sym_{m}"], out[f"cnt_{m}"] = u, inv.reshape(-1).astype(np.int64), cnt.astype(np.int64)
        said.append(f"{m} bits: {len(u)} distinct codes")
    path = os.path.join(GOLDEN, "kmeans.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes\n  states: DB {out['db_lab']:.4f}, CH {out['ch_lab']:.4f}\n  "
          + "\n  ".join(said))


if __name__ == "__main__":
    main()
