"""Hidden Markov model of a synthetic sequence of soft latents (hmm.py, csrc/hmm.hip): the device time of every entry of an
iteration (device events, the fastest of three runs after a warm-up), the forward pass as the plain recursion against the
blocked default, Viterbi, the wall time of a whole fit from a perturbed labelling, and -- with --host -- the numpy
restatement of tests/_hmm_ref.py on the host for the same iterations.

    python tools/run_hmm.py [N L K] [--host] [--host-iters 2] [--launches-only] [--sequences S [S ...]] [--out FILE]

Default size: 12298 x 50 in 17 states (tools/run_mixture.py's shape).  The states follow a sticky chain (stay 0.98); the start
is the states' own labelling with every tenth row moved to the next state.  The three launches of a blocked pass are one
entry point: their split comes from a kernel trace of this tool run with --launches-only (profiles/hmm_times.txt).
--sequences S cuts the same chain into S pieces of (nearly) equal length and times the rbvae_hmm_seq_ entries on them, next to
the single-sequence entries of the same run (profiles/hmm_sequences_times.txt); without it the report is unchanged.
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


def sticky_latents(N, Ld, K, stay=0.98, seed=1):
    """run_scores.soft_latents' emission model, sigmoid(0.7 centre + 1.5 noise), along a sticky chain over the K states"""
    r = np.random.RandomState(seed)
    cent = r.randn(K, Ld)
    lab = np.zeros(N, dtype=np.int64)
    lab[0] = r.randint(K)
    moves = r.rand(N) >= stay
    jump = 1 + r.randint(max(K - 1, 1), size=N)
    for t in range(1, N):
        lab[t] = (lab[t - 1] + jump[t]) % K if moves[t] and K > 1 else lab[t - 1]
    return (1.0 / (1.0 + np.exp(-(0.7 * cent[lab] + 1.5 * r.randn(N, Ld))))).astype(np.float32), lab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shape", nargs="*", type=int, default=[12298, 50, 17], help="N L K")
    ap.add_argument("--host", action="store_true", help="also run the numpy restatement of tests/_hmm_ref.py on the host")
    ap.add_argument("--host-iters", type=int, default=2, help="iterations of the host run")
    ap.add_argument("--launches-only", action="store_true", help="only the device times of the entries")
    ap.add_argument("--sequences", type=int, nargs="+", default=[], metavar="S",
                    help="also time the chain cut into S sequences (the rbvae_hmm_seq_ entries), for every S given")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    N, Ld, K = a.shape
    out = open(a.out, "w") if a.out else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()

    Xh, lab = sticky_latents(N, Ld, K)
    start = lab.copy()
    start[::10] = (start[::10] + 1) % K
    X = torch.from_numpy(Xh).cuda()
    call, query = sfv._lib.call, sfv._lib.query
    M = sfv.hmm_model
    R = query("rbvae_hmm_block_rows")
    say(f"{N} x {Ld} soft latents along a sticky chain over {K} states ({int((lab[1:] != lab[:-1]).sum())} changes), K = {K}, "
        f"block_rows = {R}: {-(-N // R)} blocks")

    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device="cuda")     # noqa: E731
    buf = M._Buffers(N, K, R, X.device)
    plain = M._Buffers(N, K, N, X.device)
    buf.gamma.zero_()
    buf.gamma.scatter_(0, torch.from_numpy(start).cuda().view(1, N), 1.0)
    weights, logc, means, covars, prec = f64(K), f64(K), f64(K, Ld), f64(K, Ld), f64(K, Ld)
    mws = f64(query("rbvae_gmm_ws_bytes", N, Ld, K) // 8)
    call("rbvae_gmm_mstep", X, N, Ld, buf.gamma, K, 1e-6, weights, means, covars, prec, logc, mws, None)
    A = M._initial_transitions(torch.from_numpy(start).cuda(), K)
    pi = torch.full((K,), 1.0 / K, dtype=torch.float64, device="cuda")
    A2, pi2 = torch.empty_like(A), torch.empty_like(pi)
    lb, hist = f64(1), f64(4)
    state, undecided = torch.zeros(4, dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")

    def fwd(b):
        call("rbvae_hmm_forward", buf.e, buf.rowmax, N, K, pi, A, b.R, b.alpha, b.ll, b.status, b.ws, b.ws_bytes, None)

    def bwd(b):
        call("rbvae_hmm_backward", buf.e, N, K, A, b.R, b.beta, b.status, b.ws, b.ws_bytes, None)

    def decide():                                           # tol = 0 and max_iter out of reach: no rule fires
        state.copy_(undecided)
        call("rbvae_gmm_decide", buf.ll, N, 0.0, 4, lb, hist, state)

    t_e = device_ms(lambda: call("rbvae_hmm_emit", X, N, Ld, means, prec, K, buf.logb, buf.rowmax, buf.e, None))
    t_f, t_b = device_ms(lambda: fwd(buf)), device_ms(lambda: bwd(buf))
    t_f1, t_b1 = device_ms(lambda: fwd(plain)), device_ms(lambda: bwd(plain))
    t_p = device_ms(lambda: buf.posterior(A, A2, pi2))
    m2, v2, p2, w2, c2 = f64(K, Ld), f64(K, Ld), f64(K, Ld), f64(K), f64(K)
    t_m = device_ms(lambda: call("rbvae_gmm_mstep", X, N, Ld, buf.gamma, K, 1e-6, w2, m2, v2, p2, c2, mws, None))
    t_re = device_ms(lambda: state.copy_(undecided))
    t_d = device_ms(decide) - t_re
    lpi, lA = torch.log(pi), torch.log(A)
    back, path, score = torch.empty((N, K), dtype=torch.uint8, device="cuda"), torch.empty(N, dtype=torch.int32, device="cuda"), f64(1)
    t_v = device_ms(lambda: call("rbvae_hmm_viterbi", buf.logb, N, K, lpi, lA, back, path, score, None))
    say(f"  emissions                               {t_e:9.3f} ms   {float(N) * K * Ld / (t_e * 1e-3) / 1e9:8.2f} G coordinate pairs/s")
    say(f"  forward, blocked (three launches)       {t_f:9.3f} ms   as the plain recursion (one launch) {t_f1:9.3f} ms: "
        f"{t_f1 / t_f:.2f} x")
    say(f"  backward, blocked (three launches)      {t_b:9.3f} ms   as the plain recursion (one launch) {t_b1:9.3f} ms: "
        f"{t_b1 / t_b:.2f} x")
    say(f"  posterior (three launches)              {t_p:9.3f} ms")
    say(f"  M-step (three launches)                 {t_m:9.3f} ms")
    say(f"  decision                                {t_d:9.3f} ms")
    say(f"  an iteration's fourteen launches        {t_e + t_f + t_b + t_p + t_m + t_d:9.3f} ms of device time")
    say(f"  Viterbi (one wave, once per fit)        {t_v:9.3f} ms   {t_v / N * 1e3:.3f} us per row")
    for S in a.sequences:
        lengths = [N // S + (1 if s < N % S else 0) for s in range(S)]
        sb = M._Buffers(N, K, R, X.device, M._Plan(tuple(lengths), N, R, X.device))
        sb.e, sb.rowmax, sb.logb = buf.e, buf.rowmax, buf.logb
        p = sb.plan
        scores = f64(S)
        t_sf = device_ms(lambda: call("rbvae_hmm_seq_forward", sb.e, sb.rowmax, N, K, pi, A, R, p.dev, S, sb.alpha, sb.ll, sb.status,
                                      sb.ws, sb.ws_bytes, None))
        t_sb = device_ms(lambda: call("rbvae_hmm_seq_backward", sb.e, N, K, A, R, p.dev, S, sb.beta, sb.status, sb.ws, sb.ws_bytes, None))
        t_sp = device_ms(lambda: sb.posterior(A, A2, pi2))
        t_sv = device_ms(lambda: call("rbvae_hmm_seq_viterbi", sb.logb, N, K, p.dev, S, lpi, lA, back, path, scores, None))
        blocks = sum(-(-n // R) for n in lengths)
        say(f"{S} sequences of {min(lengths)} to {max(lengths)} rows: {blocks} blocks, the longest walk {-(-max(lengths) // R)}")
        say(f"  forward (three launches)                {t_sf:9.3f} ms   one sequence, the existing entry {t_f:9.3f} ms: {t_f / t_sf:.2f} x")
        say(f"  backward (three launches)               {t_sb:9.3f} ms   one sequence, the existing entry {t_b:9.3f} ms: {t_b / t_sb:.2f} x")
        say(f"  posterior (three launches)              {t_sp:9.3f} ms   one sequence, the existing entry {t_p:9.3f} ms")
        say(f"  Viterbi (a wave per sequence)           {t_sv:9.3f} ms   one sequence, the existing entry {t_v:9.3f} ms: {t_v / t_sv:.2f} x")
        say(f"  forward + backward + Viterbi            {t_sf + t_sb + t_sv:9.3f} ms   one sequence, the existing entries "
            f"{t_f + t_b + t_v:9.3f} ms")
        if not a.launches_only:
            sfv.hmm(X, K, init=start, max_iter=2, lengths=lengths)      # warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sfit = sfv.hmm(X, K, init=start, lengths=lengths)
            torch.cuda.synchronize()
            t_sfit = time.perf_counter() - t0
            say(f"  whole fit (wall): {t_sfit:.4f} s, {sfit.n_iter} iterations ({sfit.why}), {t_sfit / sfit.n_iter * 1e3:.3f} ms per "
                f"iteration, mean log-likelihood {sfit.log_likelihood:.6f}, Viterbi ARI "
                f"{sfv.clustering_agreement(lab, sfit.path, K, K)['ari']:.4f}")
    if a.launches_only:
        if out:
            out.close()
        return

    sfv.hmm(X, K, init=start, max_iter=2)                   # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fit = sfv.hmm(X, K, init=start)
    torch.cuda.synchronize()
    t_fit = time.perf_counter() - t0
    say(f"whole fit from the perturbed states (wall): {t_fit:.4f} s, {fit.n_iter} iterations ({fit.why}), "
        f"{t_fit / fit.n_iter * 1e3:.3f} ms per iteration, mean log-likelihood {fit.log_likelihood:.6f}, score "
        f"{sfv.hmm_score(fit, X):.6f}, BIC {sfv.hmm_bic(fit, X):.1f}, AIC {sfv.hmm_aic(fit, X):.1f}")
    agree = sfv.clustering_agreement(lab, fit.path, K, K)
    before = sfv.clustering_agreement(lab, start, K, K)
    mix = sfv.gmm(X, K, init=start)
    say(f"  against the states: Viterbi ARI {agree['ari']:.4f} (the start {before['ari']:.4f}, the mixture's labels from the same "
        f"start {sfv.clustering_agreement(lab, mix.labels, K, K)['ari']:.4f}); mean largest posterior "
        f"{float(fit.posterior.max(dim=1).values.mean()):.4f}; {len(M.change_points(fit.path))} change points; mixture BIC "
        f"{sfv.gmm_bic(mix, X):.1f}")
    if a.host:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import _hmm_ref as ref
        n = max(1, min(a.host_iters, fit.n_iter))
        t0 = time.perf_counter()
        host = ref.fit(Xh, start, K, max_iter=n)
        t_host = time.perf_counter() - t0
        d = np.abs(host["log_likelihoods"] - fit.log_likelihoods[:n]).max()
        say(f"numpy restatement on the host: {n} iterations and the final pass {t_host:.2f} s, {t_host / (n + 1):.2f} s per pass; "
            f"its log-likelihood history within {d:.2e} of the device's; device iteration / host pass = "
            f"{t_fit / fit.n_iter / (t_host / (n + 1)):.2e}")
    if out:
        out.close()


if __name__ == "__main__":
    main()
