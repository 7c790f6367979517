"""Every launching entry point of csrc/losses.hip alone, us per launch (events around ITERS launches), at the shapes of the largest
case of each table of tests/_loss_cases.py: pair 1000 x 65, cosine 1000 x 32, triplet 1000 x 65 (swap), the trainers' terms
B = 16, T = 17, L = 32, binarise 1000 x 50, KL 1000 x 16, MSE 2^23 + 1.  RBVAE_LIB selects the library: run it alternating
between two builds to compare them (a kernel byte-identical in both still moves by ~0.2 us: code placement)."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, sfv_amd as sfv
Lb = sfv._lib
ITERS = 300
def timeit(fn, iters=ITERS):
    for _ in range(10): fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); a.record()
    for _ in range(iters): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3
def dev(*shape): return torch.randn(*shape, device="cuda")
out, gs = torch.empty(1, device="cuda"), torch.full((1,), 0.5, device="cuda")
runs = []
def entry(name, *args): runs.append((name, lambda: Lb.call("rbvae_" + name, *args)))

R, L = 1000, 65
x1, x2, x3 = dev(R, L), dev(R, L), dev(R, L)
d1, d2, d3 = (torch.empty(R, L, device="cuda") for _ in range(3))
entry("pairdist_fwd", x1, x2, L, L, R, L, 1, 1.0, 1e-6, out)
entry("pairdist_bwd", x1, x2, L, L, R, L, 1, 1.0, 1e-6, 3.0, gs, d1, d2, L, L, 0)
entry("triplet_fwd", x1, x2, x3, L, L, L, R, L, 1.0, 1e-8, 1, out)
entry("triplet_bwd", x1, x2, x3, L, L, L, R, L, 1.0, 1e-8, 1, 3.0, gs, d1, d2, d3, L, L, L, 0)
Lc = 32
c1, c2, e1, e2 = dev(R, Lc), dev(R, Lc), torch.empty(R, Lc, device="cuda"), torch.empty(R, Lc, device="cuda")
entry("paircos_fwd", c1, c2, Lc, Lc, R, Lc, 0, 0.8, 1e-8, out)
entry("paircos_bwd", c1, c2, Lc, Lc, R, Lc, 0, 0.8, 1e-8, 1.0, gs, e1, e2, Lc, Lc)
B, T, Lt = 16, 17, 32
h0 = dev(B, T, Lt) * 0.1
h1 = h0 + dev(B, T, Lt) * 0.05
g0, g1 = torch.empty_like(h0), torch.empty_like(h1)
parts = torch.empty(2 * Lb.query("rbvae_contrast_term_nparts", B, T), device="cuda")
entry("contrast_term_fwd", h0, h1, B, T, Lt, out)
entry("contrast_term_bwd", h0, h1, B, T, Lt, 1.0, gs, g0, g1)
entry("contrast_term_fused", h0, h1, B, T, Lt, 1.0, gs, parts, g0, g1)
entry("triplet_term_fwd", h0, h1, B, T, Lt, 0.2, out)
entry("triplet_term_bwd", h0, h1, B, T, Lt, 0.2, 1.0, gs, g0, g1)
Rb, Lbn = 1000, 50
h, U = dev(Rb, Lbn) * 2, torch.rand(Rb, Lbn, device="cuda")
y, z, dh, gz = (torch.empty(Rb, Lbn, device="cuda") for _ in range(4))
gz.normal_()
klp = torch.empty(Lb.query("rbvae_binarize_kl_nparts", Rb, Lbn), device="cuda")
entry("binarize_kl_fwd", h, U, y, z, out, Rb, Lbn, 0.7, 0.3, 1e-8, 0, 0.5, 1e-8, 1, 0, None)
entry("binarize_kl_fwd_parts", h, U, y, z, klp, Rb, Lbn, 0.7, None, 0.3, 1e-8, 0, 0.5, 1e-8, 1, 0, None)
entry("binarize_kl_fwd_parts", h, None, y, z, klp, Rb, Lbn, 0.7, None, 0.3, 1e-8, 0, 0.5, 1e-8, 1, 7, None)
entry("binarize_kl_bwd", gz, y, z, dh, 0, Rb, Lbn, 0.7, None, 0.3, gs, 0.5, 1e-8, 1)
Rk, Lk = 1000, 16
q, dq = dev(Rk, Lk) * 2, torch.empty(Rk, Lk, device="cuda")
entry("kl_fwd", q, out, Rk, Lk, 0.1, 1e-10, 0)
entry("kl_bwd", q, dq, Rk, Lk, 0.1, 1e-10, 0, 1.0, gs)
n = (1 << 23) + 1
ma, mb, mda = torch.rand(n, device="cuda"), torch.rand(n, device="cuda"), torch.empty(n, device="cuda")
ws = torch.empty(Lb.query("rbvae_mse_ws_floats", n), device="cuda")
entry("mse_fwd", ma, mb, n, out, ws)
entry("mse_bwd", ma, mb, n, 1.0, gs, mda)

Lb.call("rbvae_binarize_kl_fwd", h, U, y, z, out, Rb, Lbn, 0.7, 0.3, 1e-8, 0, 0.5, 1e-8, 1, 0, None)   # y, z of the backward
for name, fn in runs:
    print(f"{name:24s} {timeit(fn):8.2f} us", flush=True)
