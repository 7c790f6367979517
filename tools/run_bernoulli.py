"""Bernoulli models of a synthetic sequence of hard codes (bernoulli.py, csrc/bernoulli.hip): the device time of every entry of
an iteration of the mixture and of the hidden Markov model (device events, the fastest of three runs after a warm-up) with the
bytes each launch moves over its time, rbvae_hmm_emit and rbvae_gmm_mstep at the same (N, L, K) beside them, and the wall time of
both fits from a perturbed labelling.

    python tools/run_bernoulli.py [N L K] [--launches-only] [--out FILE]

Default size: 12298 x 50 in 17 states (tools/run_hmm.py's shape).  The codes are a planted chain: K prototypes, every bit flipped
with probability 0.25, the chain staying with probability 0.98; the start is the states' own labelling with every tenth row
moved to the next state.  Bytes moved: what a launch must read and write once (codes or packed words, tables, resp / logb / e
and the outputs), not what the cache hierarchy adds.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import sfv_amd as sfv  # noqa: E402
from run_scores import device_ms  # noqa: E402


def planted_codes(N, Ld, K, flip=0.25, stay=0.98, seed=1):
    r = np.random.RandomState(seed)
    proto = r.rand(K, Ld) < 0.5
    lab = np.zeros(N, dtype=np.int64)
    moves = r.rand(N) >= stay
    jump = r.randint(K, size=N)
    for t in range(1, N):
        lab[t] = jump[t] if moves[t] else lab[t - 1]
    return (proto[lab] ^ (r.rand(N, Ld) < flip)).astype(np.float32), lab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shape", nargs="*", type=int, default=[12298, 50, 17], help="N L K")
    ap.add_argument("--launches-only", action="store_true", help="only the device times of the entries")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    N, Ld, K = a.shape
    out = open(a.out, "w") if a.out else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()

    def line(name, ms, nbytes, extra=""):
        say(f"  {name:<44s}{ms:9.3f} ms   {nbytes / 1e6:9.2f} MB   {nbytes / (ms * 1e-3) / 1e9:8.1f} GB/s{extra}")

    Xh, lab = planted_codes(N, Ld, K)
    start = lab.copy()
    start[::10] = (start[::10] + 1) % K
    X = torch.from_numpy(Xh).cuda()
    call, query = sfv._lib.call, sfv._lib.query
    B, M = sfv.bernoulli, sfv.hmm_model
    R = query("rbvae_hmm_block_rows")
    say(f"{N} x {Ld} hard codes along a planted chain over {K} states ({int((lab[1:] != lab[:-1]).sum())} changes, flip 0.25), "
        f"K = {K}; {query('rbvae_bern_chunk_components', Ld)} components per LDS chunk (Gaussian: "
        f"{query('rbvae_gmm_chunk_components', Ld)})")

    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device="cuda")     # noqa: E731
    bits = torch.empty((N, 4), dtype=torch.int32, device="cuda")
    t_pack = device_ms(lambda: call("rbvae_bern_pack", X, N, Ld, bits))
    buf = M._Buffers(N, K, R, X.device)
    buf.gamma.zero_()
    buf.gamma.scatter_(0, torch.from_numpy(start).cuda().view(1, N), 1.0)
    m = B.MStep(bits, N, Ld, K, 1.0)
    m.run(buf.gamma)
    resp, lognorm, label = f64(K, N), f64(N), torch.empty(N, dtype=torch.int32, device="cuda")
    A = M._initial_transitions(torch.from_numpy(start).cuda(), K)
    pi = torch.full((K,), 1.0 / K, dtype=torch.float64, device="cuda")
    A2, pi2 = torch.empty_like(A), torch.empty_like(pi)

    tab = 2 * K * Ld * 8
    t_e = device_ms(lambda: call("rbvae_bern_emit", bits, N, Ld, m.logt, m.logf, K, buf.logb, buf.rowmax, buf.e, None))
    t_es = device_ms(lambda: call("rbvae_bern_estep", bits, N, Ld, m.logt, m.logf, m.logw, K, resp, lognorm, None, None))
    t_el = device_ms(lambda: call("rbvae_bern_estep", bits, N, Ld, m.logt, m.logf, m.logw, K, None, lognorm, label, None))
    t_m = device_ms(lambda: m.run(buf.gamma))
    # the Gaussian entries at the same shape, on the same 0 / 1 matrix
    gw, gc, gmu, gvar, gprec = f64(K), f64(K), f64(K, Ld), f64(K, Ld), f64(K, Ld)
    gws = f64(query("rbvae_gmm_ws_bytes", N, Ld, K) // 8)
    gm = lambda: call("rbvae_gmm_mstep", X, N, Ld, buf.gamma, K, 1e-6, gw, gmu, gvar, gprec, gc, gws, None)     # noqa: E731
    gm()
    logb2, rowmax2, e2 = f64(K, N), f64(N), f64(N, K)
    t_ge = device_ms(lambda: call("rbvae_hmm_emit", X, N, Ld, gmu, gprec, K, logb2, rowmax2, e2, None))
    t_gm = device_ms(gm)
    t_f = device_ms(lambda: call("rbvae_hmm_forward", buf.e, buf.rowmax, N, K, pi, A, R, buf.alpha, buf.ll, buf.status, buf.ws,
                                 buf.ws_bytes, None))
    t_b = device_ms(lambda: call("rbvae_hmm_backward", buf.e, N, K, A, R, buf.beta, buf.status, buf.ws, buf.ws_bytes, None))
    t_p = device_ms(lambda: buf.posterior(A, A2, pi2))
    nk8 = N * K * 8
    say("launch                                          device time       bytes moved   bytes / time")
    line("pack (f32 codes -> 16 bytes a row)", t_pack, N * Ld * 4 + N * 16)
    line("Bernoulli emissions (logb, rowmax, e)", t_e, N * 16 + tab + 3 * nk8 + N * 8,
         f"   {float(N) * K * Ld / (t_e * 1e-3) / 1e9:8.2f} G (row, k, l) / s")
    line("Gaussian emissions, rbvae_hmm_emit", t_ge, N * Ld * 4 + tab + 3 * nk8 + N * 8,
         f"   {float(N) * K * Ld / (t_ge * 1e-3) / 1e9:8.2f} G (row, k, l) / s; Bernoulli / Gaussian = {t_e / t_ge:.2f}")
    line("Bernoulli E-step with resp", t_es, N * 16 + tab + 4 * nk8 + N * 8)
    line("Bernoulli E-step, labels only", t_el, N * 16 + tab + N * 12)
    line("Bernoulli M-step (two launches)", t_m, N * 16 + nk8 + 2 * len(m.ws) * 8 + 3 * K * Ld * 8)
    line("Gaussian M-step, rbvae_gmm_mstep (three)", t_gm, 2 * (N * Ld * 4 + nk8) + 2 * len(gws) * 8 + 3 * K * Ld * 8,
         f"   Bernoulli / Gaussian = {t_m / t_gm:.2f}")
    say(f"  forward {t_f:.3f} ms, backward {t_b:.3f} ms, posterior {t_p:.3f} ms (hmm.hip's, unchanged)")
    say(f"  an iteration of the mixture (E, M, decision)        {t_es + t_m:9.3f} ms of device time without the decision")
    say(f"  an iteration of the hidden Markov model             {t_e + t_f + t_b + t_p + t_m:9.3f} ms of device time without the decision")
    if a.launches_only:
        if out:
            out.close()
        return

    for name, fit_fn, score, bic, labels in (("mixture", sfv.bmm, sfv.bmm_score, sfv.bmm_bic, lambda f: f.labels),
                                             ("hidden Markov model", sfv.bhmm, sfv.bhmm_score, sfv.bhmm_bic, lambda f: f.path)):
        fit_fn(X, K, init=start, max_iter=2)                # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fit = fit_fn(X, K, init=start)
        torch.cuda.synchronize()
        t_fit = time.perf_counter() - t0
        agree = sfv.clustering_agreement(lab, labels(fit), K, K)
        say(f"whole fit of the {name} from the perturbed states (wall): {t_fit:.4f} s, {fit.n_iter} iterations "
            f"({'converged' if fit.converged else 'not converged'}), {t_fit / fit.n_iter * 1e3:.3f} ms per iteration, score "
            f"{score(fit, X):.6f}, BIC {bic(fit, X):.1f}; ARI against the states {agree['ari']:.4f} (the start "
            f"{sfv.clustering_agreement(lab, start, K, K)['ari']:.4f})")
    g = sfv.hmm(X, K, init=start)
    say(f"  the Gaussian hmm.hmm on the same 0 / 1 matrix: {g.n_iter} iterations ({g.why}), Viterbi ARI "
        f"{sfv.clustering_agreement(lab, g.path, K, K)['ari']:.4f}, BIC {sfv.hmm_bic(g, X):.1f} with "
        f"{M.n_parameters(K, Ld)} parameters (Bernoulli: {B.bhmm_n_parameters(K, Ld)})")
    sym = sfv.code_symbols(X)[1].shape[0]
    say(f"  code_symbols on the same codes: {sym} distinct patterns in {N} rows")
    if out:
        out.close()


if __name__ == "__main__":
    main()
