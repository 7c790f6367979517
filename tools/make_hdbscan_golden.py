"""Writes tests/golden/hdbscan.npz from scikit-learn 1.7.2's HDBSCAN and scipy's minimum spanning tree, on the CPU: what
tests/_hdbscan_ref.py (and through it csrc/hdbscan.hip) is held to.

    python tools/make_hdbscan_golden.py

scikit-learn is fed the exact f64 distance matrix sqrt(d2) of tests/_dbscan_ref.d2_matrix as metric="precomputed", so its
core distances and mutual reachabilities are the restatement's bit for bit and only its tie-breaking (the visiting order of its
Prim, an unstable argsort of the tree's edges) can differ.  Per case NAME: NAME/X f32 [N, L], NAME/m (min_samples), NAME/mcs
(min_cluster_size), NAME/labels int32 = labels_, NAME/prob f64 = probabilities_, NAME/n_clusters, NAME/mst_w f64 [N - 1] =
scipy.sparse.csgraph.minimum_spanning_tree's weights of the mutual reachability matrix, sorted, NAME/cut_distances f64 [3] with
NAME/cut0..2 int32 = dbscan_clustering(cut_distance, mcs), and NAME/agrees: whether the restatement's labels (as a partition)
and probabilities (bit for bit) equal scikit-learn's.  Three strings: names, sklearn, and permutation_note (below).

The cases are planted blobs of unequal spread with thin bridges (tests/_hdbscan_ref.blobs), rows shuffled.  This script asserts:
every m = 1 case agrees (a seed that does not is passed over: without structural ties only a collapse of two weights under sqrt
can make it differ); at least three cases with m >= 2 agree; n_clusters is equal on every case; at least one case does not
agree, and it is kept and marked; every named defect of the restatement (_hdbscan_ref.DEFECTS) changes its answer on some case
-- but for "eom_ge", which needs two stabilities to be equal and has a hand-made tree in tests/test_hdbscan_cpu.py instead; no cut distance lies within a relative 1e-9 of a tree weight.  For the first case that does not agree it fits scikit-learn again
on a row permutation of the same matrix and records in permutation_note whether its own labels survived.
"""
import os
import sys

import numpy as np
import sklearn
from scipy.sparse.csgraph import minimum_spanning_tree
from sklearn.cluster import HDBSCAN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _dbscan_ref as D  # noqa: E402
import _hdbscan_ref as R  # noqa: E402

# (name, N, L, blobs, m, mcs, must agree)
SPECS = [("m1_a", 200, 2, 4, 1, 5, True), ("m1_b", 300, 8, 5, 1, 10, True), ("m1_c", 130, 50, 3, 1, 5, True),
         ("m1_d", 400, 3, 6, 1, 15, True),
         ("m5_a", 300, 8, 5, 5, 15, True), ("m5_b", 130, 2, 3, 5, 5, True), ("m3_a", 250, 3, 4, 3, 10, False),
         ("m2_a", 200, 16, 4, 2, 8, True), ("m10_a", 400, 8, 6, 10, 10, False), ("m5_c", 160, 50, 4, 5, 5, False),
         ("m4_a", 600, 2, 7, 4, 20, False)]
SEEDS = 100


def sklearn_fit(dist, m, mcs):
    return HDBSCAN(min_cluster_size=mcs, min_samples=m, metric="precomputed", copy=True).fit(dist)


def one_case(N, L, K, m, mcs, seed):
    X = R.blobs(N, L, K, seed)
    D2 = D.d2_matrix(X)
    assert (D2[~np.eye(N, dtype=bool)] > 0).all(), "duplicate rows: scipy reads a zero as no edge"
    dist = np.sqrt(D2)
    sk = sklearn_fit(dist, m, mcs)
    ref = R.hdbscan(X, mcs, m)
    c = np.sqrt(R.core2(D2, m))
    mr = np.maximum(np.maximum(c[:, None], c[None, :]), dist)
    np.fill_diagonal(mr, 0.0)
    mst_w = np.sort(minimum_spanning_tree(mr).data)
    assert len(mst_w) == N - 1 and np.array_equal(mst_w, ref["d"]), "the spanning trees' weights differ"
    levels = np.unique(mst_w)
    cuts = []
    for q in (0.5, 0.8, 0.95):
        k = min(int(q * len(levels)), len(levels) - 2)
        e = 0.5 * (levels[k] + levels[k + 1])
        assert np.abs(mst_w / e - 1.0).min() > 1e-9
        lab = sk.dbscan_clustering(e, min_cluster_size=mcs).astype(np.int32)
        assert R.same_partition(lab, R.cut(ref["edges"], ref["d"], N, e, mcs)[0]), "a cut differs"
        cuts.append((e, lab))
    labels = sk.labels_.astype(np.int32)
    n = int(labels.max()) + 1
    agrees = R.same_partition(labels, ref["labels"]) and np.array_equal(sk.probabilities_.view(np.int64), ref["prob"].view(np.int64))
    return dict(X=X, m=m, mcs=mcs, labels=labels, prob=sk.probabilities_.astype(np.float64), n_clusters=n, mst_w=mst_w,
                cuts=cuts, agrees=agrees, same_count=n == ref["n_clusters"], ref=ref, dist=dist)


def permutation_note(name, c):
    N = len(c["X"])
    perm = np.random.RandomState(1).permutation(N)
    again = sklearn_fit(c["dist"][np.ix_(perm, perm)], c["m"], c["mcs"])
    same = R.same_partition(again.labels_, c["labels"][perm])
    same_p = np.array_equal(again.probabilities_, c["prob"][perm])
    X = c["X"][perm]
    ours = R.hdbscan(X, c["mcs"], c["m"])
    assert R.same_partition(ours["labels"], c["ref"]["labels"][perm]) and np.array_equal(ours["prob"], c["ref"]["prob"][perm])
    return (f"case {name}: scikit-learn {sklearn.__version__} refitted on a row permutation of the same distance matrix gives "
            f"{'the same' if same else 'ANOTHER'} partition and {'the same' if same_p else 'OTHER'} probabilities; the restatement "
            "gives the same partition and probabilities")


def main():
    out, names, notes = {}, [], None
    seen_defect = {d: False for d in R.DEFECTS if d != "eom_ge"}
    for name, N, L, K, m, mcs, must in SPECS:
        for seed in range(SEEDS):
            try:
                c = one_case(N, L, K, m, mcs, seed)
            except AssertionError as e:
                print(f"{name}: seed {seed} passed over ({e})")
                continue
            if c["same_count"] and (c["agrees"] or not must):
                break
            print(f"{name}: seed {seed} passed over (agrees {c['agrees']}, same count {c['same_count']})")
        else:
            raise SystemExit(f"{name}: no seed below {SEEDS} serves")
        print(f"{name}: N={N} L={L} m={m} mcs={mcs} seed={seed}: {c['n_clusters']} clusters, "
              f"{int((c['labels'] < 0).sum())} noise, agrees={c['agrees']}")
        for d in seen_defect:
            bad = R.hdbscan(c["X"], mcs, m, defect=d)
            if not R.same_fit(bad, c["ref"]):
                seen_defect[d] = True
        if not c["agrees"] and notes is None:
            notes = permutation_note(name, c)
            print(notes)
        names.append(name)
        for k in ("X", "labels", "prob", "mst_w"):
            out[f"{name}/{k}"] = c[k]
        for k in ("m", "mcs", "n_clusters", "agrees"):
            out[f"{name}/{k}"] = np.array(c[k])
        out[name + "/cut_distances"] = np.array([e for e, _ in c["cuts"]])
        for q, (_, lab) in enumerate(c["cuts"]):
            out[f"{name}/cut{q}"] = lab
    agree = [n for n in names if bool(out[n + "/agrees"])]
    assert all(n in agree for n in names if int(out[n + "/m"]) == 1)
    assert sum(int(out[n + "/m"]) >= 2 for n in agree) >= 3
    assert len(agree) < len(names) and notes is not None, "no case that does not agree"
    assert all(seen_defect.values()), seen_defect
    path = os.path.join(ROOT, "tests", "golden", "hdbscan.npz")
    np.savez_compressed(path, names=",".join(names), sklearn=sklearn.__version__, permutation_note=notes, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(agree)} of {len(names)} cases agree")


if __name__ == "__main__":
    main()
