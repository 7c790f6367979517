"""Writes tests/golden/dbscan.npz from scikit-learn 1.7.2's DBSCAN alone, on the CPU: the labels and the core rows that
symbols-from-video_amd/density.py and tests/_dbscan_ref.py must equal on every row.

    python tools/make_dbscan_golden.py

Per case NAME: NAME/X f32 [N, L], NAME/min_samples, NAME/eps (Euclidean: sklearn's eps) or NAME/bits (Hamming: the number of
differing bits; sklearn gets eps = (bits + 0.5) / L), NAME/labels int32 [N] = labels_, NAME/core_sample_indices int32 =
core_sample_indices_.  Two strings: names (the cases, comma-separated) and sklearn (its version).

The cases (a few hundred rows each):
    blobs, blobs_ms1, blobs_ms9     Euclidean, L = 8: four blobs of different spread, rows on the bridges between them and
                                    scattered rows; min_samples 5, 1 and 9
    sparse                          Euclidean: scattered rows only, no core row
    contested                       Euclidean, L = 1: {0, .1, .2, .3, .4}, {2, .., 2.4}, 1.2 and a far point, eps 0.85, rows
                                    permuted: 1.2 is a non-core row with core neighbours in both clusters
    codes, codes_ms1, codes_tight   Hamming, L = 32: five prototypes with flipped bits and random codes; (bits, min_samples)
                                    (3, 5), (2, 1) and (0, 3)
    codes_sparse                    Hamming: random codes only, no core row
This script asserts what makes the comparison meaningful, and tests/test_dbscan_cpu.py asserts it again: no pair of a
Euclidean case lies within a relative 1e-9 of eps^2 (so sklearn's distance arithmetic cannot disagree with the kernel's), each
metric has a case with border rows, one case has a contested border row (and it takes label 0 under 50 other permutations as
well), one has noise, one no core row, one min_samples = 1.
"""
import os
import sys

import numpy as np
import sklearn
from sklearn.cluster import DBSCAN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _dbscan_ref as R  # noqa: E402

CONTESTED = np.array([0, .1, .2, .3, .4, 2, 2.1, 2.2, 2.3, 2.4, 1.2, 10.0])


def blobs(seed=3):
    r = np.random.RandomState(seed)
    L = 8
    centres = r.randn(4, L) * 3.0
    parts = [centres[k] + s * r.randn(n, L) for k, (n, s) in enumerate(((90, 0.25), (70, 0.3), (60, 0.35), (40, 0.45)))]
    for a, b in ((0, 1), (1, 2), (2, 3)):
        t = np.linspace(0.1, 0.9, 9)[:, None]
        parts.append((1 - t) * centres[a] + t * centres[b] + 0.05 * r.randn(9, L))
    parts.append(r.randn(23, L) * 4.0)
    X = np.concatenate(parts)
    return X[r.permutation(len(X))].astype(np.float32)


def codes(seed=5):
    r = np.random.RandomState(seed)
    L = 32
    proto = r.rand(5, L) < 0.5
    lab = r.randint(5, size=260)
    X = proto[lab] ^ (r.rand(260, L) < 0.04)
    X = np.concatenate([X, r.rand(40, L) < 0.5])
    return X[r.permutation(len(X))].astype(np.float32)


def cases():
    r = np.random.RandomState(11)
    B, C = blobs(), codes()
    return [("blobs", B, "euclidean", 1.1, 5), ("blobs_ms1", B, "euclidean", 1.1, 1), ("blobs_ms9", B, "euclidean", 0.9, 9),
            ("sparse", (r.randn(150, 8) * 4.0).astype(np.float32), "euclidean", 0.5, 3),
            ("contested", CONTESTED[r.permutation(len(CONTESTED))].astype(np.float32)[:, None], "euclidean", 0.85, 5),
            ("codes", C, "hamming", 3, 5), ("codes_ms1", C, "hamming", 2, 1), ("codes_tight", C, "hamming", 0, 3),
            ("codes_sparse", (r.rand(120, 32) < 0.5).astype(np.float32), "hamming", 2, 2)]


def sk_fit(X, metric, eps, m):
    X64 = X.astype(np.float64)
    e = eps if metric == "euclidean" else (eps + 0.5) / X.shape[1]
    return DBSCAN(eps=e, min_samples=m, metric=metric, algorithm="brute").fit(X64)


def eps_margin(X, eps):
    """the smallest |d2 / eps^2 - 1| over all pairs of a Euclidean case"""
    return float(np.abs(R.d2_matrix(X) / (float(eps) * float(eps)) - 1.0).min())


def properties(X, metric, eps, m, labels, core_idx):
    """what a case shows: border rows, contested border rows, noise rows, core rows"""
    A = R.case_adjacency(X, metric, eps)
    core = np.zeros(len(X), dtype=bool)
    core[core_idx] = True
    border = ~core & (labels >= 0)
    contested = [i for i in np.flatnonzero(border) if len(set(labels[np.flatnonzero(A[i] & core)])) > 1]
    return {"border": int(border.sum()), "contested": len(contested), "noise": int((labels < 0).sum()), "core": int(core.sum()),
            "clusters": int(labels.max()) + 1}


def main():
    assert sklearn.__version__ == "1.7.2", sklearn.__version__
    out, seen = {}, []
    for name, X, metric, eps, m in cases():
        fit = sk_fit(X, metric, eps, m)
        labels, core_idx = fit.labels_.astype(np.int32), fit.core_sample_indices_.astype(np.int32)
        ref = R.dbscan(R.case_adjacency(X, metric, eps), m)
        assert np.array_equal(ref["labels"], labels) and np.array_equal(ref["core_sample_indices"], core_idx), name
        p = properties(X, metric, eps, m, labels, core_idx)
        if metric == "euclidean":
            p["margin"] = eps_margin(X, eps)
            assert p["margin"] > 1e-9, (name, p)
        print(f"{name}: {X.shape[0]} x {X.shape[1]} {metric} eps {eps} min_samples {m}: {p}")
        seen.append((name, metric, m, p))
        out[name + "/X"], out[name + "/min_samples"] = X, np.int32(m)
        out[name + ("/eps" if metric == "euclidean" else "/bits")] = np.float64(eps) if metric == "euclidean" else np.int32(eps)
        out[name + "/labels"], out[name + "/core_sample_indices"] = labels, core_idx
    for metric in ("euclidean", "hamming"):
        assert any(mt == metric and p["border"] for _, mt, _, p in seen), metric + ": no case with border rows"
    assert any(p["contested"] for _, _, _, p in seen) and any(p["noise"] for _, _, _, p in seen)
    assert any(p["core"] == 0 for _, _, _, p in seen) and any(m == 1 for _, _, m, _ in seen)
    r = np.random.RandomState(0)
    for _ in range(50):                                     # the contested row takes label 0 wherever it and the blobs stand
        perm = r.permutation(len(CONTESTED))
        lab = sk_fit(CONTESTED[perm].astype(np.float32)[:, None], "euclidean", 0.85, 5).labels_
        assert lab[np.flatnonzero(perm == 10)[0]] == 0 and set(lab) == {-1, 0, 1}
    out["names"], out["sklearn"] = ",".join(n for n, _, _, _ in seen), sklearn.__version__
    path = R.GOLDEN
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes, {len(seen)} cases")


if __name__ == "__main__":
    main()
