"""Latent-space projections (embedding_umap.py's PCA, t-SNE and UMAP) of synthetic soft latents: the device time of the kNN
graph, the perplexity search, the t-SNE iterations (repulsion, Z sum and step apart, from device events) and the PCA, the
wall time of each phase, and -- with --host -- scikit-learn's time for the same array.  --umap runs the UMAP leg alone
(kNN, smooth kNN distances, the host's CSR, the epochs, wall time) and writes it to --umap-out.

    python tools/run_projection.py [N L] [--clusters 17] [--perplexity 30] [--max-iter 1000] [--host] [--out FILE]
    python tools/run_projection.py [N L] --umap [--n-neighbors 24] [--min-dist 0.25] [--umap-out profiles/umap_times.txt]

Default size: 12298 x 50, the whole video the other tools use.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import sfv_amd as sfv  # noqa: E402


def soft_latents(N, Ld, clusters, seed=1):
    """sigmoid((2 centre - 1) 3 + 1.5 noise): soft codes around `clusters` random binary centres, labels sorted"""
    r = np.random.RandomState(seed)
    cent = r.randint(0, 2, (clusters, Ld))
    lab = np.sort(r.randint(0, clusters, N))
    return (1.0 / (1.0 + np.exp(-((2 * cent[lab] - 1) * 3 + 1.5 * r.randn(N, Ld))))).astype(np.float32), lab


def umap_leg(a, say):
    """umap_project on the synthetic latents: device events per phase, the host's share, wall time with and without them"""
    N, Ld = a.shape
    Xh, _ = soft_latents(N, Ld, a.clusters)
    X = torch.from_numpy(Xh).cuda()
    sfv.umap_project(X[:256].contiguous(), a.n_neighbors, a.min_dist, n_epochs=2)    # library and scipy loaded
    torch.cuda.synchronize()
    say(f"{N} x {Ld} soft latents, {a.clusters} clusters, UMAP n_neighbors {a.n_neighbors}, min_dist {a.min_dist:g}")
    tm = {}
    t0 = time.perf_counter()
    res = sfv.umap_project(X, a.n_neighbors, a.min_dist, timings=tm)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    say(f"UMAP: a {res.a:.6f}, b {res.b:.6f}, {res.n_epochs} epochs; wall {wall:.2f} s including the curve fit, the host's "
        f"CSR and schedule and the event bookkeeping")
    say(f"  kNN graph        {tm['knn']:10.2f} ms   (k = {a.n_neighbors - 1})")
    say(f"  smooth kNN       {tm['smooth_knn']:10.2f} ms   (distance sum and bisection, two launches)")
    say(f"  fuzzy union      {tm['fuzzy_csr']:10.2f} ms   host wall: the wait for the two launches above, read-back, CSR")
    say(f"  PCA (initial map){tm['pca']:10.2f} ms   (moments, host eigh, projection)")
    say(f"  epochs           {tm['epochs']:10.2f} ms   {1e3 * tm['epochs'] / res.n_epochs:8.1f} us per epoch, one launch each")
    t0 = time.perf_counter()
    again = sfv.umap_project(X, a.n_neighbors, a.min_dist)
    torch.cuda.synchronize()
    say(f"UMAP again without events: wall {time.perf_counter() - t0:.2f} s; bit-identical map: "
        f"{bool(torch.equal(again.embedding, res.embedding))}")
    Y = res.embedding
    say(f"  map finite: {bool(torch.isfinite(Y).all())}, span {(Y.max(0).values - Y.min(0).values).cpu().numpy()}")
    sub = torch.from_numpy(np.random.RandomState(0).permutation(N)[:min(N, 2000)]).cuda()
    say(f"  trustworthiness(n_neighbors={a.n_neighbors}) on {len(sub)} rows: "
        f"{sfv.trustworthiness(X[sub].contiguous(), Y[sub].contiguous(), a.n_neighbors):.5f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--umap", action="store_true", help="run the UMAP leg instead of t-SNE and PCA")
    ap.add_argument("--n-neighbors", type=int, default=24)
    ap.add_argument("--min-dist", type=float, default=0.25)
    ap.add_argument("--umap-out", default=None, help="also write the UMAP leg's report to this file")
    ap.add_argument("shape", nargs="*", type=int, default=[12298, 50], help="N L")
    ap.add_argument("--clusters", type=int, default=17)
    ap.add_argument("--perplexity", type=float, default=30.0)
    ap.add_argument("--max-iter", type=int, default=1000)
    ap.add_argument("--host", action="store_true", help="also time scikit-learn's PCA and TSNE on the same array")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    N, Ld = a.shape
    out = open(a.umap_out if a.umap else a.out, "w") if (a.umap_out if a.umap else a.out) else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()

    if a.umap:
        umap_leg(a, say)
        if out:
            out.close()
        return
    Xh, _ = soft_latents(N, Ld, a.clusters)
    X = torch.from_numpy(Xh).cuda()
    k = min(N - 1, int(3 * a.perplexity + 1))
    sfv.knn_graph(X[:256].contiguous(), min(k, 255))        # load the library before the clock starts
    torch.cuda.synchronize()
    say(f"{N} x {Ld} soft latents, {a.clusters} clusters, perplexity {a.perplexity:g} (k = {k}), {a.max_iter} iterations")

    tm = {}
    t0 = time.perf_counter()
    res = sfv.tsne_project(X, perplexity=a.perplexity, max_iter=a.max_iter, timings=tm)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    its = res.n_iter + 1
    say(f"t-SNE: KL {res.kl_divergence:.4f} after {its} iterations; wall {wall:.2f} s including the host's CSR and the "
        f"event bookkeeping")
    say(f"  kNN graph        {tm['knn']:10.2f} ms")
    say(f"  perplexity       {tm['perplexity']:10.2f} ms")
    say(f"  PCA (initial map){tm['pca']:10.2f} ms   (moments, host eigh, projection)")
    loop = tm["repulse"] + tm["zsum"] + tm["step"]
    say(f"  iterations       {loop:10.2f} ms   device time of {its} x 3 launches")
    for name in ("repulse", "zsum", "step"):
        say(f"    {name:8s}       {tm[name]:10.2f} ms   {1e3 * tm[name] / its:8.1f} us per iteration")
    pairs = float(N) * N
    say(f"    repulsion: {pairs * its / (tm['repulse'] * 1e-3) / 1e12:.2f} T pairs/s "
        f"({sfv._lib.query('rbvae_tsne_repulse_splits', N)} j slices)")

    t0 = time.perf_counter()
    sfv.tsne_project(X, perplexity=a.perplexity, max_iter=a.max_iter)
    torch.cuda.synchronize()
    say(f"t-SNE again without events: wall {time.perf_counter() - t0:.2f} s")
    t0 = time.perf_counter()
    p = sfv.pca_project(X, 2)
    torch.cuda.synchronize()
    say(f"PCA alone: wall {1e3 * (time.perf_counter() - t0):.2f} ms; explained variance {p.explained_variance}")

    if a.host:
        try:
            from sklearn.decomposition import PCA
            from sklearn.manifold import TSNE, trustworthiness
        except ImportError:
            say("scikit-learn does not import here: no host timing")
        else:
            t0 = time.perf_counter()
            PCA(n_components=2).fit_transform(Xh)
            t_pca = time.perf_counter() - t0
            t0 = time.perf_counter()
            ts = TSNE(n_components=2, random_state=42, perplexity=a.perplexity, max_iter=a.max_iter)
            emb = ts.fit_transform(Xh)
            t_tsne = time.perf_counter() - t0
            say(f"scikit-learn on the host ({os.environ.get('OMP_NUM_THREADS', '?')} threads): PCA {1e3 * t_pca:.1f} ms, "
                f"TSNE (Barnes-Hut, angle 0.5) {t_tsne:.1f} s, KL {ts.kl_divergence_:.4f}")
            sub = np.random.RandomState(0).permutation(N)[:min(N, 2000)]
            say(f"  trustworthiness(n_neighbors=24) on {len(sub)} rows: device {trustworthiness(Xh[sub], res.embedding.cpu().numpy()[sub], n_neighbors=24):.5f}, "
                f"host {trustworthiness(Xh[sub], emb[sub], n_neighbors=24):.5f}")
    if out:
        out.close()


if __name__ == "__main__":
    main()
