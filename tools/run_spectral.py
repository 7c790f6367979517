"""Spectral layout of the fuzzy neighbour graph of synthetic soft latents: the device time of the normalised product, of a
whole Lanczos step at j = 8, 64 and 256 (device events, the fastest of three runs after a warm-up; the basis rows below
j hold random vectors, the arithmetic is the same), of the Ritz launch, and the wall time of the whole spectral_layout,
and -- with --host -- scipy.sparse.linalg.eigsh on the same matrix.  Nothing is gated on these times.

    python tools/run_spectral.py [N L k] [--host] [--neighbors 24] [--out FILE]

Default size: 12298 x 50 in 17 states, n_neighbors 24, k = 2 eigenvectors.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import sfv_amd as sfv  # noqa: E402
from run_scores import device_ms, soft_latents  # noqa: E402

M_MAX = 300


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shape", nargs="*", type=int, default=[12298, 50, 2], help="N L k")
    ap.add_argument("--neighbors", type=int, default=24)
    ap.add_argument("--host", action="store_true", help="also run scipy.sparse.linalg.eigsh on the same matrix")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    N, Ld, k = a.shape
    out = open(a.out, "w") if a.out else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()

    Xh, _ = soft_latents(N, Ld, 17)
    X = torch.from_numpy(Xh).cuda()
    call, query = sfv._lib.call, sfv._lib.query
    t0 = time.perf_counter()
    ug = sfv.fuzzy_graph(*sfv.knn_graph(X, a.neighbors - 1), a.neighbors)
    torch.cuda.synchronize()
    t_graph = time.perf_counter() - t0
    t0 = time.perf_counter()
    g = sfv.normalized_graph(ug)
    torch.cuda.synchronize()
    t_norm = time.perf_counter() - t0
    E = int(g.indices.numel())
    say(f"{N} x {Ld} soft latents, n_neighbors {a.neighbors}: {E} directed edges, {g.n_components} component(s); kNN and fuzzy "
        f"graph {t_graph:.3f} s, normalized_graph (host checks, components, degree launch) {t_norm:.3f} s (wall)")

    q = 1
    V = torch.randn((q + M_MAX + 1, N), dtype=torch.float64, device="cuda") / np.sqrt(N)
    alpha, beta = (torch.zeros(M_MAX, dtype=torch.float64, device="cuda") for _ in range(2))
    state = torch.zeros(2, dtype=torch.int32, device="cuda")
    nbytes = query("rbvae_spectral_ws_bytes", N, M_MAX, q)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
    y = torch.empty(N, dtype=torch.float64, device="cuda")
    t_mv = device_ms(lambda: call("rbvae_spectral_matvec", g.indptr, g.indices, g.data, g.isd, N, V[0], y))
    say(f"  product                     {t_mv:9.4f} ms   {(E * 24.0 + N * 28.0) / (t_mv * 1e-3) / 1e9:8.2f} GB/s "
        "(12 B of CSR and a 16 B gather of isd and x per edge)")
    for j in (8, 64, 256):
        def step():
            call("rbvae_spectral_step", g.indptr, g.indices, g.data, g.isd, N, V, q, j, M_MAX, alpha, beta, state, ws, nbytes)
        t = device_ms(step)
        nv = q + j + 1
        say(f"  step at j = {j:3d} (10 launches) {t:9.4f} ms   {4.0 * nv * N * 8 / (t * 1e-3) / 1e9:8.2f} GB/s of basis "
            f"(four passes over {nv} vectors)")
    assert state.cpu().tolist()[0] == 0
    s = torch.randn((M_MAX, 32), dtype=torch.float64, device="cuda")
    Y = torch.empty((32, N), dtype=torch.float64, device="cuda")
    for cols in (k, 32):
        t = device_ms(lambda: call("rbvae_spectral_ritz", V, q, M_MAX, N, s[:, :cols].contiguous(), cols, Y))
        say(f"  Ritz vectors, {cols:2d} columns of {M_MAX} steps {t:9.4f} ms   {M_MAX * N * 8.0 / (t * 1e-3) / 1e9:8.2f} GB/s of basis")

    if g.n_components > 1:
        say("the graph is not connected: no layout")
    else:
        sfv.spectral._layout(g, k, max_steps=8)             # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = sfv.spectral._layout(g, k)
        torch.cuda.synchronize()
        t_lay = time.perf_counter() - t0
        say(f"whole spectral_layout (wall): {t_lay:.3f} s, {r.steps} steps ({r.why}), eigenvalues "
            f"{np.array2string(r.eigenvalues, precision=8)}, residuals {np.array2string(r.residuals, precision=2)}")
        if a.host:
            from scipy.sparse import csr_matrix
            from scipy.sparse.linalg import eigsh
            isd = g.isd.cpu().numpy()
            W = csr_matrix((g.data.cpu().numpy().astype(np.float64), g.indices.cpu().numpy(), g.indptr.cpu().numpy()),
                           shape=(N, N))
            Sm = csr_matrix(W.multiply(isd[:, None]).multiply(isd[None, :]))
            v0 = np.random.RandomState(0).uniform(-1, 1, N)
            t0 = time.perf_counter()
            th, _ = eigsh(Sm, k=k + 1, which="LA", tol=1e-10, v0=v0)
            t_host = time.perf_counter() - t0
            lam = np.sort(1.0 - th)[1:]
            say(f"scipy on the host ({os.environ.get('OMP_NUM_THREADS', '?')} threads): eigsh(k = {k + 1}, which='LA', tol 1e-10) "
                f"{t_host:.3f} s, eigenvalues within {np.abs(lam - r.eigenvalues).max():.2e} of the device's")
    if out:
        out.close()


if __name__ == "__main__":
    main()
