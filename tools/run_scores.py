"""Latent scores (trustworthiness / continuity of a map, silhouette, kNN label agreement) of synthetic soft latents: the
device time of the rank kernel, both per-state sum kernels and the two kNN graphs they sit on (device events, the fastest
of three runs after a warm-up), the scores themselves, and -- with --host -- scikit-learn's trustworthiness and
silhouette_score on the same arrays.

    python tools/run_scores.py [N L S] [--k 24] [--host] [--host-limit-gb 8] [--tsne] [--out FILE]

Default size: 12298 x 50 in 17 states, k = 24, the map is the exact PCA of the latents.  --host skips scikit-learn's
trustworthiness when its three dense N x N arrays would exceed --host-limit-gb, and says so.  --tsne adds the scores of
a whole t-SNE run on tools/run_projection.py's (well separated) latents of the same size: all rows, and the 2000 sampled
rows that tool reports from the host.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import sfv_amd as sfv  # noqa: E402


def soft_latents(N, Ld, states, seed=1):
    """sigmoid(0.7 centre + 1.5 noise): poorly separated soft codes around `states` random centres, labels sorted"""
    r = np.random.RandomState(seed)
    cent = r.randn(states, Ld)
    lab = np.sort(r.randint(0, states, N))
    return (1.0 / (1.0 + np.exp(-(0.7 * cent[lab] + 1.5 * r.randn(N, Ld))))).astype(np.float32), lab


def device_ms(fn, repeat=3):
    fn()
    best = float("inf")
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b))
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shape", nargs="*", type=int, default=[12298, 50, 17], help="N L S")
    ap.add_argument("--k", type=int, default=24)
    ap.add_argument("--host", action="store_true", help="also time scikit-learn on the same arrays")
    ap.add_argument("--host-limit-gb", type=float, default=8.0)
    ap.add_argument("--tsne", action="store_true", help="also score tsne_project's map of run_projection.py's latents")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    N, Ld, S = a.shape
    k = a.k
    out = open(a.out, "w") if a.out else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()

    Xh, lab = soft_latents(N, Ld, S)
    X = torch.from_numpy(Xh).cuda()
    Y = sfv.pca_project(X, 2).embedding.float().contiguous()
    C = (X > 0.5).float().contiguous()
    call = sfv._lib.call
    say(f"{N} x {Ld} soft latents in {S} states of {np.bincount(lab).min()}..{np.bincount(lab).max()} rows, k = {k}, "
        f"map: exact PCA")

    idx_y = torch.empty((N, k), dtype=torch.int32, device="cuda")
    idx_x = torch.empty((N, k), dtype=torch.int32, device="cuda")
    d2 = torch.empty((N, k), dtype=torch.float64, device="cuda")
    rank = torch.empty((N, k), dtype=torch.int32, device="cuda")
    excess = torch.empty(N, dtype=torch.int32, device="cuda")
    order = torch.from_numpy(np.argsort(lab, kind="stable").astype(np.int32)).cuda()
    seg = torch.from_numpy(np.concatenate([[0], np.cumsum(np.bincount(lab, minlength=S))]).astype(np.int32)).cuda()
    sums = torch.empty((N, S), dtype=torch.float64, device="cuda")
    hsums = torch.empty((N, S), dtype=torch.int32, device="cuda")

    t_ky = device_ms(lambda: call("rbvae_knn", Y, N, 2, k, idx_y, d2))
    t_kx = device_ms(lambda: call("rbvae_knn", X, N, Ld, k, idx_x, d2))
    t_rx = device_ms(lambda: call("rbvae_nbr_ranks", X, N, Ld, idx_y, k, rank, excess))
    t_ry = device_ms(lambda: call("rbvae_nbr_ranks", Y, N, 2, idx_x, k, rank, excess))
    t_se = device_ms(lambda: call("rbvae_label_dist_sums", X, N, Ld, order, seg, S, sums))
    t_sh = device_ms(lambda: call("rbvae_label_hamming_sums", C, N, Ld, order, seg, S, hsums))
    pairs = float(N) * N
    say(f"  kNN graph of the map (L = 2)        {t_ky:9.3f} ms")
    say(f"  kNN graph of the latents (L = {Ld:3d})  {t_kx:9.3f} ms")
    say(f"  ranks in the latents (trustworth.)  {t_rx:9.3f} ms   {pairs * Ld / (t_rx * 1e-3) / 1e12:6.2f} T coordinate "
        f"pairs/s, {pairs * k / (t_rx * 1e-3) / 1e12:6.2f} T comparisons/s")
    say(f"  ranks in the map (continuity)       {t_ry:9.3f} ms   {pairs * k / (t_ry * 1e-3) / 1e12:6.2f} T comparisons/s")
    say(f"  Euclidean sums per state            {t_se:9.3f} ms   {pairs * Ld / (t_se * 1e-3) / 1e12:6.2f} T coordinate "
        f"pairs/s, {pairs / (t_se * 1e-3) / 1e9:6.1f} G square roots/s")
    say(f"  Hamming sums per state              {t_sh:9.3f} ms   {pairs / (t_sh * 1e-3) / 1e12:6.2f} T key pairs/s")

    t0 = time.perf_counter()
    trust, cont = sfv.trustworthiness(X, Y, k), sfv.continuity(X, Y, k)
    sil, sil_h = sfv.silhouette_score(X, lab, S), sfv.silhouette_score(C, lab, S, metric="hamming")
    agree = sfv.knn_label_agreement(X, lab, k, S)
    torch.cuda.synchronize()
    say(f"device scores (wall {time.perf_counter() - t0:.3f} s for all of them, host finish and copies included): "
        f"trustworthiness {trust:.5f}, continuity {cont:.5f}, silhouette {sil:.5f} (Hamming {sil_h:.5f}), kNN purity "
        f"{agree['purity']:.4f}, kNN accuracy {agree['accuracy']:.4f}")

    if a.host:
        try:
            from sklearn.manifold import trustworthiness
            from sklearn.metrics import silhouette_score
        except ImportError:
            say("scikit-learn does not import here: no host timing")
        else:
            threads = os.environ.get("OMP_NUM_THREADS", "?")
            t0 = time.perf_counter()
            h_sil = silhouette_score(Xh.astype(np.float64), lab)
            say(f"scikit-learn on the host ({threads} threads): silhouette_score {time.perf_counter() - t0:.2f} s, "
                f"{h_sil:.5f} (device - host {sil - h_sil:.2e})")
            need = 3 * 8.0 * N * N / 1e9
            if need > a.host_limit_gb:
                say(f"  trustworthiness on the host was not taken: its three dense N x N arrays need {need:.1f} GB "
                    f"(limit {a.host_limit_gb:g} GB)")
            else:
                t0 = time.perf_counter()
                h_trust = trustworthiness(Xh.astype(np.float64), Y.cpu().numpy().astype(np.float64), n_neighbors=k)
                say(f"  trustworthiness {time.perf_counter() - t0:.2f} s, {h_trust:.5f} (device - host {trust - h_trust:.2e}; "
                    f"{need:.1f} GB of N x N arrays)")
    if a.tsne:
        from run_projection import soft_latents as separated_latents
        Zh, _ = separated_latents(N, Ld, S)
        Z = torch.from_numpy(Zh).cuda()
        res = sfv.tsne_project(Z)
        t0 = time.perf_counter()
        trust, cont = sfv.trustworthiness(Z, res.embedding, k), sfv.continuity(Z, res.embedding, k)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        sub = torch.from_numpy(np.sort(np.random.RandomState(0).permutation(N)[:min(N, 2000)])).cuda()
        say(f"t-SNE map of run_projection.py's latents (KL {res.kl_divergence:.4f}): trustworthiness {trust:.5f} and "
            f"continuity {cont:.5f} over all {N} rows (wall {wall:.3f} s for both); on {len(sub)} sampled rows "
            f"{sfv.trustworthiness(Z[sub].contiguous(), res.embedding[sub].contiguous(), k):.5f}")
    if out:
        out.close()


if __name__ == "__main__":
    main()
