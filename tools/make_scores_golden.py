"""Writes tests/golden/latent_scores.npz from scikit-learn 1.7.2 alone (the reference is not involved): what
symbols-from-video_amd/scores.py and tests/_scores_ref.py are pinned to.

    python tools/make_scores_golden.py

The fixture: 320 soft latents of 50 values in 8 states whose separation is deliberately poor, so that no score saturates,
    r = RandomState(3); cent = r.randn(8, 50); lab = sort(r.randint(0, 8, 320))
    X = sigmoid(0.7 cent[lab] + 1.5 r.randn(320, 50)).astype(float32); Y = PCA(2).fit_transform(X as f64).astype(float32)
and
    lab_edge                lab with state 3 renamed 9 and row 0 made state 10: a gap in the labels and a singleton
    trust_k, cont_k         trustworthiness(X64, Y64, n_neighbors=k) and trustworthiness(Y64, X64, n_neighbors=k), k in K_TRUST
    sil_{euclid,hamming}[_edge]   silhouette_samples for both label vectors; Hamming on (X > 0.5)
    nn_k                    NearestNeighbors(k).kneighbors() of X64 (self excluded), k in K_VOTE, and from those indices
    purity_k, pred_k, acc_k the share of neighbours with the row's label, the vote (ties to the smallest label, what
                            KNeighborsClassifier(k) does with kneighbors() of its training set) and its accuracy
"""
import os

import numpy as np
import sklearn
from sklearn.decomposition import PCA
from sklearn.manifold import trustworthiness
from sklearn.metrics import silhouette_samples
from sklearn.neighbors import NearestNeighbors

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "latent_scores.npz")
K_TRUST, K_VOTE = (5, 24, 91), (5, 24)


def fixture():
    r = np.random.RandomState(3)
    cent = r.randn(8, 50)
    lab = np.sort(r.randint(0, 8, 320))
    X = (1.0 / (1.0 + np.exp(-(0.7 * cent[lab] + 1.5 * r.randn(320, 50))))).astype(np.float32)
    Y = PCA(n_components=2).fit_transform(X.astype(np.float64)).astype(np.float32)
    return X, lab, Y


def edge_labels(lab):
    e = lab.copy()
    e[e == 3] = 9
    e[0] = 10
    return e


def vote(lab, idx):
    """the label with the most votes among a row's neighbours, ties to the smallest label"""
    votes = np.zeros((len(lab), int(lab.max()) + 1), dtype=np.int64)
    np.add.at(votes, (np.repeat(np.arange(len(lab)), idx.shape[1]), lab[idx].reshape(-1)), 1)
    tied = int(((votes == votes.max(1, keepdims=True)).sum(1) > 1).sum())
    return votes.argmax(1), tied


def main():
    assert sklearn.__version__ == "1.7.2", sklearn.__version__
    X, lab, Y = fixture()
    X64, Y64, B = X.astype(np.float64), Y.astype(np.float64), X > 0.5
    lab_edge = edge_labels(lab)
    out = {"X": X, "Y": Y, "lab": lab.astype(np.int32), "lab_edge": lab_edge.astype(np.int32)}
    said = []
    for k in K_TRUST:
        out[f"trust_{k}"] = np.float64(trustworthiness(X64, Y64, n_neighbors=k))
        out[f"cont_{k}"] = np.float64(trustworthiness(Y64, X64, n_neighbors=k))
        said.append(f"trustworthiness k={k} {out[f'trust_{k}']:.5f} (continuity {out[f'cont_{k}']:.5f})")
    for name, labels in (("", lab), ("_edge", lab_edge)):
        out["sil_euclid" + name] = silhouette_samples(X64, labels, metric="euclidean")
        out["sil_hamming" + name] = silhouette_samples(B, labels, metric="hamming")
        said.append(f"silhouette{name} {out['sil_euclid' + name].mean():.4f} / Hamming {out['sil_hamming' + name].mean():.4f}")
    for k in K_VOTE:
        idx = NearestNeighbors(n_neighbors=k, metric="euclidean").fit(X64).kneighbors(return_distance=False)
        pred, tied = vote(lab, idx)
        out[f"nn_{k}"] = idx.astype(np.int32)
        out[f"purity_{k}"] = np.float64((lab[idx] == lab[:, None]).mean())
        out[f"pred_{k}"] = pred.astype(np.int32)
        out[f"acc_{k}"] = np.float64((pred == lab).mean())
        said.append(f"k={k}: purity {out[f'purity_{k}']:.3f}, accuracy {out[f'acc_{k}']:.3f}, {tied} tied votes")
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes\n  " + "\n  ".join(said))


if __name__ == "__main__":
    main()
