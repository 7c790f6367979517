"""Writes tests/golden/projection.npz from scikit-learn 1.7.2 alone (the reference is not involved): what
symbols-from-video_amd/projection.py and tests/_projection_ref.py are pinned to.

    python tools/make_projection_golden.py

The fixture: 320 soft latents of 50 values in 8 clusters,
    r = RandomState(1); cent = r.randint(0, 2, (8, 50)); lab = sort(r.randint(0, 8, 320))
    X = sigmoid((2 cent[lab] - 1) 3 + 1.5 r.randn(320, 50)).astype(float32)
and, for perplexity 30 (k = 91):
    nn_idx             NearestNeighbors(91).kneighbors() of X as f64 (neighbours by distance, self excluded)
    cond_P             _binary_search_perplexity of the squared distances of those neighbours, rounded to f32
    joint_*            _joint_probabilities_nn of the kneighbors_graph, as TSNE._fit calls it (CSR)
    Y, grad, error     Y = 3 RandomState(2).randn(320, 2) as f32; _kl_divergence_bh(Y, P, 1, 320, 2, angle=0.0)
    pca_*              PCA(n_components=2) on X.astype(float64): fit_transform, components_, explained_variance_, mean_
    tsne_*             TSNE(n_components=2, random_state=42, perplexity=30).fit(X): kl_divergence_, n_iter_ and
                       trustworthiness(X, embedding_, n_neighbors=24)
"""
import os

import numpy as np
import sklearn
from sklearn.decomposition import PCA
from sklearn.manifold import TSNE, _t_sne, _utils, trustworthiness
from sklearn.neighbors import NearestNeighbors

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "projection.npz")
PERPLEXITY, K = 30.0, 91


def fixture():
    r = np.random.RandomState(1)
    cent = r.randint(0, 2, (8, 50))
    lab = np.sort(r.randint(0, 8, 320))
    X = (1.0 / (1.0 + np.exp(-((2 * cent[lab] - 1) * 3 + 1.5 * r.randn(320, 50))))).astype(np.float32)
    return X, lab


def main():
    assert sklearn.__version__ == "1.7.2", sklearn.__version__
    X, lab = fixture()
    N = len(X)
    X64 = X.astype(np.float64)
    knn = NearestNeighbors(algorithm="auto", n_neighbors=K, metric="euclidean").fit(X64)
    dist, nn_idx = knn.kneighbors()
    cond_P = _utils._binary_search_perplexity((dist ** 2).astype(np.float32), PERPLEXITY, 0)
    graph = knn.kneighbors_graph(mode="distance")
    graph.data **= 2
    P = _t_sne._joint_probabilities_nn(graph, PERPLEXITY, 0)
    P.sort_indices()
    Y = (3.0 * np.random.RandomState(2).randn(N, 2)).astype(np.float32)
    error, grad = _t_sne._kl_divergence_bh(Y.ravel().copy(), P, 1, N, 2, angle=0.0, compute_error=True, num_threads=1)
    pca = PCA(n_components=2)
    pca_Y = pca.fit_transform(X64)
    tsne = TSNE(n_components=2, random_state=42, perplexity=PERPLEXITY)
    emb = tsne.fit_transform(X)
    np.savez_compressed(
        OUT, X=X, labels=lab.astype(np.int32), nn_idx=nn_idx.astype(np.int32), cond_P=cond_P,
        joint_indptr=P.indptr.astype(np.int32), joint_indices=P.indices.astype(np.int32), joint_data=P.data,
        Y=Y, grad=grad.reshape(N, 2).astype(np.float32), error=np.float64(error),
        pca_Y=pca_Y, pca_components=pca.components_, pca_explained_variance=pca.explained_variance_, pca_mean=pca.mean_,
        tsne_kl=np.float64(tsne.kl_divergence_), tsne_n_iter=np.int32(tsne.n_iter_),
        tsne_trust=np.float64(trustworthiness(X, emb, n_neighbors=24)))
    print(f"{OUT}: {os.path.getsize(OUT)} bytes; KL {tsne.kl_divergence_:.4f} after {tsne.n_iter_} iterations, "
          f"trustworthiness {trustworthiness(X, emb, n_neighbors=24):.5f}, error at Y {error:.6f}, "
          f"max |grad| {np.abs(grad).max():.3e}, {P.nnz} joint entries")


if __name__ == "__main__":
    main()
