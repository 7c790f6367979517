"""References, error model, f32 emulations and case tables for the loss and optimiser kernel bounds tests: the 20 kernels
of csrc/losses.hip, combine_losses_k / adam_k / adam_hyper_k (csrc/layout.hip) and the Adam branches of run_jobs_k (kinds
3-with-context, 6 and 7, csrc/jobs.hip).  Plain torch / numpy on the CPU: importing this module needs no GPU.

Error model (u = 2^-24; derived, not tuned)
    Assumptions, the ones on record in tests/_lstm_cases.py: library expf and logf at 1 ulp (2u relative), sqrtf and the
    division correctly rounded (u), every other f32 operation one rounding (u); hipcc may contract a product and a sum into
    one fma, which removes a rounding and never adds one.  A result whose exact value lies below 2^-126 may be flushed
    (TINY_DEN); expf past its range gives inf or 0 where the exact sigmoid is within TINY_F32 of 0 or 1.
    gamma(h) = h u / (1 - h u) bounds a summation tree of height h (additions any one term passes through), per unit of
    sum |terms|.  Heights are read off the kernels:
        wave row sum (row_sqdist, row_cos)   ceil(L/64) lane-strided chain + 6 wave_sum levels
        one-workgroup row losses             ceil(rows/16) rows per wave (only lane 0 is non-zero, so wave_sum adds zeros:
                                             exact) + the 16-wave loop of block_sum
        kl_fwd_k, binarize_kl_fwd_k          ceil(n/1024) per thread + 6 + 16
        binarize_kl_fwd_parts_k              per 256-element block: tests/_lstm_cases.check_kl_parts
        mse_partial_k + mse_final_k          c = ceil(ceil((n/4)/256)/blocks) float4 steps of 4 additions each + 1 (tail)
                                             + 6 + 4 (block) + 6 + 8 (final, 512 threads)
        contrast_term_fused_k parts          the 4 rows of a block: 3
        combine_losses_k                     ceil(n/1024) + 6 + 16 per sum
    Constants are taken as the f32 values the kernel forms: eps, margin, scale / (float)rows (* gscale_dev), 2 w /
    (float)(B T), w / ((float)B (float)(T-1)), tau, logf(p), logf(1 - p).

    Row distance d = sqrt(sum_k t_k^2), t_k = fl(fl(a_k - b_k) + eps).  Both roundings of t_k are determined by the operands
        (nothing can be contracted), so the model uses the actual dt_k = |t_k(f32) - t_k| (<= u(|a_k - b_k| + |t_k|)); the
        square adds u t_k^2:   E_s = sum_k (2|t_k| dt_k + dt_k^2 + u t_k^2) + gamma(ceil(L/64) + 6) s,
        E_d = min(E_s / (sqrt(s) + sqrt(max(s - E_s, 0))), sqrt(E_s)) + u d   (sqrtf correctly rounded).  s = 0 has E_s = 0:
        a row built with a - b + eps == 0 is exactly zero on the device too.
    Downstream of d (analytic): d^2: 2 d E_d + E_d^2 + u d^2;  m = margin - d: E_m = E_d + u|m|;  max(m, 0)^2:
        2|m| E_m + E_m^2 + u m^2 (max is 1-Lipschitz, so the VALUE needs no branch rule);  coefficient -2 w m / d (two
        roundings; 2 w is exact): (2|w| / d)(E_m + |m|(E_d / (d - E_d) + 2u));  w / d: |w / d|(E_d / (d - E_d) + u);
        a gradient element c t_k: |c| dt_k + E_c |t_k| + u|c t_k|;  sums of n such contributions: + (n - 1) u sum |.|;
        accumulate = 1: + u |prev + g|.
    Scalar losses: sum of the per-row bounds + gamma(h) sum |terms|, then the division (u) -- contrast_term_fwd: two
        divisions and one addition.  Triplet rows: |dq| <= E_dap + max(E_dan, E_dpn) + 2u(|margin + dap| + |q|).
    Cosine: dot, |a|^2, |b|^2 share the row tree: E_dot = (u + gamma) sum |a_k b_k|, norms relative (u + gamma)/2 + u; the
        clamps fmaxf(., eps) are exact and 1-Lipschitz; cs = dot / (ca cb): E_dot / (ca cb) + |cs|(r_a + r_b + 2u);
        d = 1 - cs: + u|d|; g = 2 w max(margin - d, 0) or -2 w d (continuous in d: no branch rule): 2|w|(E_d + u|m|) + u|g|;
        inv = 1 / (ca cb): r_a + r_b + 2u; ia = cs / na^2: E_cs / na^2 + |ia|(2 r_a + 2u); an element g (b inv - ia a):
        E_g |x| + |g|(|b inv|(r_inv + 2u) + |a|(E_ia + 2u|ia|)) + u|g x|.
    KL (kl_fwd_k on logits v): q = sigmoid(v) carries c_sig_lib(v); with f(q) = q(log(q + e) - lp) + (1 - q)(log(1 - q + e)
        - l1p):  |f'(q)| c_sig + per product [q(2u|log| + 2u) + u|log - lp| q + u|term|] + u|f|; the clamp is 1-Lipschitz;
        1 - eps is the f32 value (1.0f for eps <= 2^-25).  On the stored codes (binarize_kl_fwd_k) the same function, from the
        kernel's own z.  mean = tree sum / (float)rows.
    kl_bwd_k: w kl_elem_grad: tests/_lstm_cases.kl_grad64's bound times |w|, + u|result|.  binarize_kl_bwd_k: gtop_bin
        (same module) with g_hs = the preloaded dh under accumulate = 1; gscale_dev adds 2u of the KL part (the reference
        forms klw * gs / rows with one rounding fewer than the kernel).  mse_bwd_k: w (a - b): 2u|result|.
    MSE: per element 3u d^2 (the difference, the square), the tree above, the division.
    combine_losses_k: recon = tree(sse) * inv_n, kl = tree * kl_scale (u each); pair = w_sim s0 + w_dis s1 (3u of the
        absolute terms); out4[0] against the kernel's own out4[1..3]: 2u(|beta k| + |alpha pr|) + u(|recon + beta k| +
        |total|); with 0 parts out4[1..3] are the inputs bit for bit.
    Hyper terms: float64 on the device.  Against numpy longdouble: one f32 rounding u|x| plus the device pow: at most
        K_POW = 16 double ulps (the OpenCL bound for pow; the HIP device library states less), i.e. a relative
        16 * 2^-53 b^t / (1 - b^t) <= 1.8e-12 of hyper[0] at b2 = 0.999, t = 1, half of it through the square root, + 3
        double roundings: 2e-12 |x| in all -- invisible after the cast except within 2e-12 |x| of an f32 rounding tie.
    Adam (adam_update of csrc/common.h; reference in float64 from the f32 inputs and the f32 hyper values the kernel read):
        gi = fl(g gscale): u|gi|.   m' = fma(1 - b1, fl(gi - m), m): E_m = (1 - b1) u(|gi| + |gi - m|) + u|m'|.
        v' = fma(fl((1 - b2) gi), gi, fl(v b2)): E_v = 3u (1 - b2) gi^2 + u|v b2| + u|v'|.   (+ TINY_DEN each)
        sq = sqrtf(v'): E_sq = min(E_v / (sqrt(v') + sqrt(max(v' - E_v, 0))), sqrt(E_v)) + u sq;  den = sq / bc2 + eps:
        E_den = E_sq / bc2 + u sq / bc2 + u den;  r = m' / den: E_r = E_m / (den - E_den) + |m'| E_den / (den (den -
        E_den)) + u|r|;  w' = fma(-step, r, w): E_w = step E_r + u|w'|.  E_den / den is the term that grows where
        sqrt(v') / bc2 ~ eps.
    Packed copies of the update jobs: no tolerance.  Each equals the storage rounding (f32 / bf16 round-to-nearest-even) of
        the master element the job stored, through the job's index map.

Decisions on a threshold
    m > 0 and d > 0 (hinges), margin + dap - dneg > 0, dpn < dan (swap), na > eps, the KL clamp mask.  A row is ambiguous
    when the float64 quantity lies within its own bound of the threshold; an ambiguous row passes if it is within the bound
    of EITHER branch's reference (check_slots enumerates the branch combinations an output row depends on).  The random
    tables hold no ambiguous row even with 100 x the bound (asserted on the CPU); rows built on a threshold are those where
    the f32 outcome is determined: a - b + eps == 0 (s = 0 exactly) and bitwise equal rows a == p (dan and dpn are the same
    f32 operations on the same operands: an exact tie whatever the rounding, so only the tie branch is allowed).
    Conventions recorded here: at a swap tie the gradient is split evenly (torch.minimum); clamp(min = 0) at exactly 0
    passes gradient 1 in torch and 0 in the kernels (m > 0) -- a measure-zero point, which the either-branch rule covers.
    Hard codes need no rule: z == (y > 0.5) of the kernel's own y (check_binarize)."""
import itertools
import math

import numpy as np
import torch

from _bounds import U32
from _lstm_cases import TINY_F32, _exact, _worst, c_sig, check_binarize, check_kl_parts, gtop_bin, kl_grad64

U = U32
D, F = torch.float64, torch.float32
BF = torch.bfloat16
TINY_DEN = 2.0 ** -126
K_POW = 16
GOLD = 0x9E3779B97F4A7C15
MIX = 0xD6E8FEB86659FD93
M64 = (1 << 64) - 1


def f32(x):
    """The f32 value of a host float argument."""
    return float(torch.tensor(float(x), dtype=F))


def f32t(x):
    return torch.tensor(float(x), dtype=F)


def gamma(h):
    return h * U / (1 - h * U)


def cdiv(a, b):
    return -(-a // b)


def row_height(L):
    return cdiv(L, 64) + 6


def rows_height(rows):
    return cdiv(rows, 16) + 16


def flat_height(n):
    return cdiv(n, 1024) + 6 + 16


def mse_blocks(n):
    return max(1, min(512, cdiv(n >> 2, 1024)))


def mse_height(n):
    return 4 * cdiv(cdiv(n >> 2, 256), mse_blocks(n)) + 1 + 6 + 4 + 6 + 8


# ---- the counter hash of csrc/common.h -------------------------------------------------------------------------------

def hash_u32(seed, idx):
    """hash_u32(seed, idx) of csrc/common.h on numpy uint64 (wrapping arithmetic).  idx: array of element indices."""
    with np.errstate(over="ignore"):
        x = (np.asarray(idx, dtype=np.uint64) + np.uint64(1)) * np.uint64(GOLD) + np.uint64(seed & M64)
        x ^= x >> np.uint64(32)
        x *= np.uint64(MIX)
        x ^= x >> np.uint64(32)
        x *= np.uint64(MIX)
        x ^= x >> np.uint64(32)
    return (x & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def hash_u32_by_hand(seed, idx):
    """The same definition on Python integers, one step per line (the literal values of the CPU test come from here)."""
    x = ((idx + 1) * GOLD + seed) & M64
    x ^= x >> 32
    x = (x * MIX) & M64
    x ^= x >> 32
    x = (x * MIX) & M64
    x ^= x >> 32
    return x & 0xFFFFFFFF


def device_uniform(n, seed, seed_dev=None):
    """The U == NULL draw of both binarise kernels: (hash >> 8) * 2^-24 of seed + seed_dev * GOLD, exact in f32."""
    s = (seed + (seed_dev * GOLD if seed_dev is not None else 0)) & M64
    h = hash_u32(s, np.arange(n, dtype=np.uint64)) >> np.uint32(8)
    return torch.from_numpy(h.astype(np.float32) * np.float32(2.0 ** -24))


# ---- f32 emulation primitives (the kernels' summation orders) ----------------------------------------------------------

_XOR = [torch.arange(64) ^ o for o in (32, 16, 8, 4, 2, 1)]


def wave_sum32(x):
    """wave_sum over the last axis (64 lanes): the xor butterfly, 32 first."""
    for idx in _XOR:
        x = x + x[..., idx]
    return x[..., 0]


def strided32(vals, nthreads):
    """Per-thread chains acc += vals[tid + k * nthreads], k ascending -> [nthreads]."""
    n = vals.numel()
    k = cdiv(n, nthreads)
    p = torch.zeros(k * nthreads, dtype=F)
    p[:n] = vals.reshape(-1)
    p = p.view(k, nthreads)
    acc = torch.zeros(nthreads, dtype=F)
    for i in range(k):
        acc = acc + p[i]
    return acc


def block_sum32(x):
    """block_sum: wave_sum per wave, then the waves in order."""
    w = wave_sum32(x.view(-1, 64))
    t = torch.zeros((), dtype=F)
    for i in range(w.numel()):
        t = t + w[i]
    return t


def rows_sum32(terms):
    """One wave per row, rows wid, wid + 16, ... chained per wave (lane 0), then block_sum."""
    acc = strided32(terms, 16)
    t = torch.zeros((), dtype=F)
    for i in range(16):
        t = t + acc[i]
    return t


def lane_rows32(x):
    """Row sums of x [R][L] as a wave computes them: the lane-strided chain, then wave_sum."""
    R, L = x.shape
    k = cdiv(L, 64)
    p = torch.zeros(R, k * 64, dtype=F)
    p[:, :L] = x
    p = p.view(R, k, 64)
    acc = torch.zeros(R, 64, dtype=F)
    for i in range(k):
        acc = acc + p[:, i]
    return wave_sum32(acc)


def t32(a, b, eps, defect=None):
    """t_k = fl(fl(a - b) + eps) in f32."""
    d = a.to(F) - b.to(F)
    return d if defect == "no_eps" else d + f32t(eps)


def rowdist32(a, b, eps, defect=None):
    """(t [R][L], d [R]) of row_sqdist + sqrtf in f32."""
    t = t32(a, b, eps, defect)
    return t, torch.sqrt(lane_rows32(t * t))


def sig32(x):
    return 1.0 / (1.0 + torch.exp(-x))


# ---- row distance: float64 reference and bound -------------------------------------------------------------------------

class Dist:
    """Row distances of a [R][L] against b [R][L] in float64 with the model's bounds (module docstring)."""

    def __init__(self, a, b, eps):
        a64, b64, e = a.to(D), b.to(D), f32(eps)
        self.L = a.shape[-1]
        self.t = a64 - b64 + e
        self.dt = (t32(a, b, eps).to(D) - self.t).abs()
        t, dt = self.t, self.dt
        self.s = (t * t).sum(-1)
        self.E_s = ((2 * t.abs() * dt + dt * dt + U * t * t).sum(-1) + gamma(row_height(self.L)) * self.s) * (1 + 2.0 ** -20)
        self.d = self.s.sqrt()
        lo = (self.s - self.E_s).clamp(min=0).sqrt()
        first = self.E_s / (self.d + lo).clamp(min=1e-300)
        self.E_d = (torch.where(self.s > 0, torch.minimum(first, self.E_s.sqrt()), self.E_s.sqrt()) + U * self.d) * (1 + U)
        self.same = (a == b).all(-1)          # bitwise equal operands

    def sq(self):
        """(d^2, bound)."""
        return self.d ** 2, 2 * self.d * self.E_d + self.E_d ** 2 + U * self.d ** 2

    def hinge(self, margin, K=1.0):
        """m = margin - d: (max(m, 0)^2, its bound, m, E_m, active, ambiguous)."""
        m = f32(margin) - self.d
        E_m = self.E_d + U * m.abs()
        val = m.clamp(min=0) ** 2
        return val, 2 * m.abs() * E_m + E_m ** 2 + U * m * m, m, E_m, m > 0, m.abs() <= K * E_m

    def _inv_rel(self):
        return self.E_d / (self.d - self.E_d).clamp(min=1e-300)

    def hinge_options(self, margin, w, sign=1.0, valid=None, K=1.0):
        """The two branches of coef = (m > 0 && d > 0) ? -2 w m / d : 0 as options of a gradient slot: the contribution
        sign * coef * t_k with its bound and the rows it is allowed on."""
        _, _, m, E_m, act, amb = self.hinge(margin, K)
        pos = self.d > 0
        valid = torch.ones_like(pos) if valid is None else valid
        dd = self.d.clamp(min=1e-300)
        c = torch.where(pos, -2 * w * m / dd, torch.zeros_like(m))
        E_c = torch.where(pos, 2 * abs(w) / dd * (E_m + m.abs() * (self._inv_rel() + 2 * U)) * (1 + 1e-6), torch.zeros_like(m))
        g = c[:, None] * self.t
        bnd = c.abs()[:, None] * self.dt + E_c[:, None] * self.t.abs() + U * g.abs()
        zero = torch.zeros_like(g)
        on = (sign * g, bnd, valid & pos & (act | amb))
        off = (zero, zero, ~valid | ~pos | ~act | amb)
        return [on, off], amb & valid & pos

    def linear(self, c):
        """(c * t_k, bound) for an exactly formed f32 coefficient c."""
        g = c * self.t
        return g, abs(c) * self.dt + U * g.abs()

    def over_d(self, w):
        """(w / d * t_k, bound): one division."""
        pos = self.d > 0
        dd = self.d.clamp(min=1e-300)
        c = torch.where(pos, w / dd, torch.zeros_like(dd))
        E_c = c.abs() * (self._inv_rel() + U) * (1 + 1e-6)
        g = c[:, None] * self.t
        return g, c.abs()[:, None] * self.dt + E_c[:, None] * self.t.abs() + U * g.abs()


def check_slots(got, base, slots, n_add, what, dims=("row", "unit"), prev=None):
    """got [R][L] against base + one option per slot.  base: (ref, bnd) or None; a slot is a list of options (ref, bnd,
    allowed [R]); the additions that join the contributions cost n_add u sum |contributions|; prev: accumulate = 1 onto it.
    A row passes if ANY combination of options allowed on it holds the bound.  Returns the worst |err| / bound."""
    got = got.to(D)
    best = torch.full(got.shape, float("inf"), dtype=D)
    slots = [[o for o in s if bool(o[2].any())] for s in slots]
    for combo in itertools.product(*slots):
        ref = torch.zeros_like(got) if base is None else base[0].clone()
        bnd = torch.zeros_like(got) if base is None else base[1].clone()
        mag = ref.abs()
        ok = torch.ones(got.shape[0], dtype=torch.bool)
        for r, b, a in combo:
            ref, bnd, mag, ok = ref + r, bnd + b, mag + r.abs(), ok & a
        bnd = bnd + n_add * U * mag
        if prev is not None:
            ref = prev.to(D) + ref
            bnd = bnd + U * ref.abs()
        bnd = bnd + TINY_DEN
        err = (got - ref).abs()
        ratio = torch.where(torch.isnan(err) | ~ok[:, None], torch.full_like(err, float("inf")), err / bnd)
        best = torch.minimum(best, ratio)
    return _worst(best, torch.ones_like(best), what, dims)


def tree_scalar(terms, E_terms, h):
    """(sum, bound) of a summation tree of height h over terms with their own bounds."""
    return terms.sum(), E_terms.sum() + gamma(h) * terms.abs().sum()


def check_scalar(got, ref, bnd, what):
    got, ref, bnd = float(got), float(ref), float(bnd) + TINY_DEN
    err = abs(got - ref)
    assert err <= bnd, f"{what}: got {got!r}, ref {ref!r}, |err| {err:.3g} > bound {bnd:.3g} (ratio {err / bnd:.3g})"
    return err / bnd


# ---- pairwise distance loss (pairdist_fwd_k / pairdist_bwd_k) ----------------------------------------------------------

def w_rows(scale, rows, gs=None):
    """scale / (float)rows (* gscale_dev[0]) as the kernels form it in f32."""
    w = f32t(scale) / f32t(rows)
    return w * f32t(gs) if gs is not None else w


def check_pairdist_fwd(x1, x2, label, margin, eps, got, what="pairdist_fwd"):
    P = Dist(x1, x2, eps)
    terms, E = P.hinge(margin)[:2] if label else P.sq()
    R = x1.shape[0]
    s, b = tree_scalar(terms, E, rows_height(R))
    return check_scalar(got, s / R, b / R + U * abs(float(s)) / R, what)


def pairdist_options(x1, x2, label, margin, eps, w, K=1.0):
    """(base, slots, ambiguous rows) of dx1; dx2 is its negative."""
    P = Dist(x1, x2, eps)
    if not label:
        return P.linear(2 * w), [], torch.zeros(x1.shape[0], dtype=torch.bool)
    opts, amb = P.hinge_options(margin, w, K=K)
    return None, [opts], amb


def neg_opts(base, slots):
    nb = None if base is None else (-base[0], base[1])
    return nb, [[(-r, b, a) for r, b, a in s] for s in slots]


def check_pairdist_bwd(x1, x2, label, margin, eps, scale, gs, dx1, dx2, prev1=None, prev2=None, what="pairdist_bwd"):
    """dx1 / dx2 (either may be None: a null pointer); prev: the preloaded gradients of accumulate = 1."""
    base, slots, _ = pairdist_options(x1, x2, label, margin, eps, float(w_rows(scale, x1.shape[0], gs)))
    out = {}
    if dx1 is not None:
        out["dx1"] = check_slots(dx1, base, slots, 0, f"{what}: dx1", prev=prev1)
    if dx2 is not None:
        out["dx2"] = check_slots(dx2, *neg_opts(base, slots), 0, f"{what}: dx2", prev=prev2)
    return out


def emu_pairdist_fwd(x1, x2, label, margin, eps, defect=None):
    _, d = rowdist32(x1, x2, eps, defect)
    m = torch.clamp(f32t(margin) - d, min=0)
    return rows_sum32(m * m if label else d * d) / f32t(x1.shape[0])


def emu_pairdist_bwd(x1, x2, label, margin, eps, scale, gs, prev1=None, prev2=None, defect=None):
    t, d = rowdist32(x1, x2, eps, defect)
    w = w_rows(scale, x1.shape[0], gs)
    if label:
        m = f32t(margin) - d if defect == "hinge_not_zeroed" else torch.clamp(f32t(margin) - d, min=0)
        live = (d > 0) if defect == "hinge_not_zeroed" else (m > 0) & (d > 0)
        coef = torch.where(live, (-2.0 * w) * m / d, torch.zeros_like(d))[:, None]
    else:
        coef = 2.0 * w
    g = coef * t
    acc = prev1 is not None and defect != "accumulate_ignored"
    g2 = g if defect == "dx2_plus" else -g
    return (prev1 + g if acc else g), (prev2 + g2 if acc else g2)


# ---- cosine form (paircos_fwd_k / paircos_bwd_k) -------------------------------------------------------------------------

class Cos:
    def __init__(self, a, b, eps):
        a, b, e = a.to(D), b.to(D), f32(eps)
        L = a.shape[-1]
        r = (U + gamma(row_height(L))) * (1 + 2.0 ** -20)
        self.a, self.b, self.e = a, b, e
        self.dot, self.E_dot = (a * b).sum(-1), r * (a * b).abs().sum(-1)
        self.na, self.nb = (a * a).sum(-1).sqrt(), (b * b).sum(-1).sqrt()
        self.r_n = r / 2 * (1 + r) + U                                   # relative bound of either norm
        self.ca, self.cb = self.na.clamp(min=e), self.nb.clamp(min=e)
        den = self.ca * self.cb
        self.cs = self.dot / den
        self.E_cs = (self.E_dot / den + self.cs.abs() * (2 * self.r_n + 2 * U)) * (1 + 1e-6)
        self.d = 1 - self.cs
        self.E_d = self.E_cs + U * self.d.abs()

    def terms(self, label, margin):
        if not label:
            return self.d ** 2, 2 * self.d.abs() * self.E_d + self.E_d ** 2 + U * self.d ** 2
        m = f32(margin) - self.d
        E_m = self.E_d + U * m.abs()
        return m.clamp(min=0) ** 2, 2 * m.abs() * E_m + E_m ** 2 + U * m * m

    def grad_options(self, label, margin, w, K=1.0):
        """dx1 and dx2 slots: the branch na > eps (resp. nb > eps) per row."""
        m = f32(margin) - self.d
        if label:
            g, E_g = 2 * w * m.clamp(min=0), 2 * abs(w) * (self.E_d + U * m.abs())
        else:
            g, E_g = -2 * w * self.d, 2 * abs(w) * self.E_d
        E_g = E_g + U * g.abs()
        den = self.ca * self.cb
        inv, r_inv = 1 / den, 2 * self.r_n + 2 * U
        out, ambs = [], []
        for x, y, nx in ((self.a, self.b, self.na), (self.b, self.a, self.nb)):
            amb = (nx - self.e).abs() <= K * self.r_n * nx
            big = nx > self.e
            n2 = (nx * nx).clamp(min=1e-300)
            ia = self.cs / n2
            E_ia = (self.E_cs / n2 + ia.abs() * (2 * self.r_n + 2 * U)) * (1 + 1e-6)
            opts = []
            for on, allowed in ((True, big | amb), (False, ~big | amb)):
                i_, E_i = (ia, E_ia) if on else (torch.zeros_like(ia), torch.zeros_like(ia))
                p1, p2 = y * inv[:, None], i_[:, None] * x
                xx = p1 - p2
                ref = g[:, None] * xx
                bnd = (E_g[:, None] * xx.abs() + g.abs()[:, None] * (p1.abs() * (r_inv + 2 * U) + x.abs() * (E_i + 2 * U * i_.abs())[:, None])
                       + U * ref.abs())
                opts.append((ref, bnd, allowed))
            out.append([opts])
            ambs.append(amb)
        return out[0], out[1], ambs[0] | ambs[1]


def check_paircos_fwd(x1, x2, label, margin, eps, got, what="paircos_fwd"):
    terms, E = Cos(x1, x2, eps).terms(label, margin)
    R = x1.shape[0]
    s, b = tree_scalar(terms, E, rows_height(R))
    return check_scalar(got, s / R, b / R + U * abs(float(s)) / R, what)


def check_paircos_bwd(x1, x2, label, margin, eps, scale, gs, dx1, dx2, what="paircos_bwd"):
    s1, s2, _ = Cos(x1, x2, eps).grad_options(label, margin, float(w_rows(scale, x1.shape[0], gs)))
    out = {}
    if dx1 is not None:
        out["dx1"] = check_slots(dx1, None, s1, 0, f"{what}: dx1")
    if dx2 is not None:
        out["dx2"] = check_slots(dx2, None, s2, 0, f"{what}: dx2")
    return out


def _cos32(a, b, eps):
    a, b, e = a.to(F), b.to(F), f32t(eps)
    dot, na, nb = lane_rows32(a * b), torch.sqrt(lane_rows32(a * a)), torch.sqrt(lane_rows32(b * b))
    return a, b, e, dot, na, nb


def emu_paircos_fwd(x1, x2, label, margin, eps, defect=None):
    a, b, e, dot, na, nb = _cos32(x1, x2, eps)
    d = 1.0 - dot / (torch.clamp(na, min=e) * torch.clamp(nb, min=e))
    m = torch.clamp(f32t(margin) - d, min=0)
    return rows_sum32(m * m if label else d * d) / f32t(x1.shape[0])


def emu_paircos_bwd(x1, x2, label, margin, eps, scale, gs, defect=None):
    a, b, e, dot, na, nb = _cos32(x1, x2, eps)
    ca, cb = torch.clamp(na, min=e), torch.clamp(nb, min=e)
    cs = dot / (ca * cb)
    d = 1.0 - cs
    w = w_rows(scale, x1.shape[0], gs)
    g = (2.0 * w) * torch.clamp(f32t(margin) - d, min=0) if label else (-2.0 * w) * d
    zero = torch.zeros_like(cs)
    ia, ib = torch.where(na > e, cs / (na * na), zero), torch.where(nb > e, cs / (nb * nb), zero)
    if defect == "cos_no_ia":
        ia, ib = zero, zero
    inv = 1.0 / (ca * cb)
    return g[:, None] * (b * inv[:, None] - ia[:, None] * a), g[:, None] * (a * inv[:, None] - ib[:, None] * b)


# ---- the trainer's contrastive term (contrast_term_fwd_k / _bwd_k / _fused_k) ---------------------------------------------

C_EPS = 1e-6


def _next_rows(h0):
    """Row r + 1 of every row (the wrap at the end is masked by `valid`), and valid = t < T - 1."""
    B, T, L = h0.shape
    rows = h0.reshape(B * T, L)
    valid = (torch.arange(B * T) % T) < T - 1
    return rows, torch.roll(rows, -1, 0), valid


def contrast_weights(B, T, scale, gs):
    """(wsim, wdis, (float)(B T), (float)B (float)(T - 1)) as f32 tensors."""
    w = f32t(scale) * f32t(gs) if gs is not None else f32t(scale)
    nbt, nb1 = f32t(B * T), f32t(B) * f32t(T - 1)
    return (2.0 * w) / nbt, w / nb1, nbt, nb1


def check_contrast_fwd(h0, h1, got, what="contrast_term_fwd"):
    B, T, L = h0.shape
    rows, nxt, valid = _next_rows(h0)
    sim, E_sim = Dist(rows, h1.reshape(B * T, L), C_EPS).sq()
    dis, E_dis = Dist(rows[valid], nxt[valid], C_EPS).hinge(1.0)[:2]
    h = rows_height(B * T)
    (s1, b1), (s2, b2) = tree_scalar(sim, E_sim, h), tree_scalar(dis, E_dis, h)
    _, _, nbt, nb1 = contrast_weights(B, T, 1.0, None)
    q1, q2 = float(s1) / float(nbt), float(s2) / float(nb1)
    return check_scalar(got, q1 + q2, float(b1) / float(nbt) + float(b2) / float(nb1) + U * (abs(q1) + abs(q2) + abs(q1 + q2)), what)


def _shift_opts(opts, first_row):
    """Options of pair (r, r + 1) moved to row r + 1 with the opposite sign (the second operand of the pair)."""
    out = []
    for k, (r, b, a) in enumerate(opts):
        a2 = torch.roll(a, 1, 0)
        a2 = (a2 & ~first_row) if k == 0 else (a2 | first_row)
        out.append((-torch.roll(r, 1, 0), torch.roll(b, 1, 0), a2))
    return out


def contrast_options(h0, h1, scale, gs, K=1.0):
    B, T, L = h0.shape
    wsim, wdis, _, _ = contrast_weights(B, T, scale, gs)
    rows, nxt, valid = _next_rows(h0)
    base = Dist(rows, h1.reshape(B * T, L), C_EPS).linear(float(wsim))
    me, amb = Dist(rows, nxt, C_EPS).hinge_options(1.0, float(wdis), valid=valid, K=K)
    first = (torch.arange(B * T) % T) == 0
    return base, [me, _shift_opts(me, first)], amb


def check_contrast_bwd(h0, h1, scale, gs, dh0, dh1, what="contrast_term_bwd"):
    base, slots, _ = contrast_options(h0, h1, scale, gs)
    return {"dh0": check_slots(dh0.reshape(base[0].shape), base, slots, 2, f"{what}: dh0"),
            "dh1": check_slots(dh1.reshape(base[0].shape), (-base[0], base[1]), [], 0, f"{what}: dh1")}


def check_contrast_parts(h0, h1, parts, what="contrast_term_fused"):
    """parts[2 blk] / parts[2 blk + 1]: the sums over the block's four rows (((r0 + r1) + r2) + r3)."""
    B, T, L = h0.shape
    rows, nxt, valid = _next_rows(h0)
    sim, E_sim = Dist(rows, h1.reshape(B * T, L), C_EPS).sq()
    dis, E_dis = Dist(rows, nxt, C_EPS).hinge(1.0)[:2]
    z = torch.zeros_like(dis)
    dis, E_dis = torch.where(valid, dis, z), torch.where(valid, E_dis, z)
    nblk = cdiv(B * T, 4)

    def blocks(v):
        p = torch.zeros(nblk * 4, dtype=D)
        p[:B * T] = v
        return p.view(nblk, 4).sum(1)
    ref = torch.stack([blocks(sim), blocks(dis)], 1)
    bnd = torch.stack([blocks(E_sim) + gamma(3) * blocks(sim), blocks(E_dis) + gamma(3) * blocks(dis)], 1) + TINY_DEN
    return _worst((parts.to(D).view(nblk, 2) - ref).abs(), bnd, f"{what}: parts", ("block", "sum"))


def emu_contrast(h0, h1, scale, gs, defect=None):
    """dict(out, dh0, dh1, parts) of the contrastive term in f32, in the kernels' order."""
    B, T, L = h0.shape
    wsim, wdis, nbt, nb1 = contrast_weights(B, T, scale, gs)
    if defect == "dis_over_BT":
        wdis, nb1 = (f32t(scale) * f32t(gs) if gs is not None else f32t(scale)) / nbt, nbt
    rows, nxt, valid = _next_rows(h0)
    rows, nxt = rows.to(F), nxt.to(F)
    tab, dab = rowdist32(rows, h1.reshape(B * T, L), C_EPS, defect)
    tn, dn = rowdist32(rows, nxt, C_EPS, defect)
    m = torch.clamp(1.0 - dn, min=0)
    sim, dis = dab * dab, torch.where(valid, m * m, torch.zeros_like(m))
    c = torch.where(valid & (m > 0) & (dn > 0), (-2.0 * wdis) * m / dn, torch.zeros_like(m))
    out = rows_sum32(sim) / nbt + rows_sum32(dis) / nb1
    gsim = wsim * tab
    cp, tp = torch.roll(c, 1, 0), torch.roll(tn, 1, 0)
    if defect == "last_pair_missing":
        cp = torch.where((torch.arange(B * T) % T) == T - 1, torch.zeros_like(cp), cp)
    g0 = gsim + c[:, None] * tn
    g0 = g0 + cp[:, None] * tp if defect == "cp_added" else g0 - cp[:, None] * tp
    nblk = cdiv(B * T, 4)
    parts = torch.zeros(nblk * 4, 2)
    parts[:B * T, 0], parts[:B * T, 1] = sim, dis
    parts = parts.view(nblk, 4, 2)
    parts = ((parts[:, 0] + parts[:, 1]) + parts[:, 2]) + parts[:, 3]
    return dict(out=out, dh0=g0.view(B, T, L), dh1=(-gsim).view(B, T, L), parts=parts.reshape(-1))


# ---- triplet (triplet_fwd_k / triplet_bwd_k / triplet_term_fwd_k / triplet_term_bwd_k) ---------------------------------------

class Triplet:
    def __init__(self, a, p, n, margin, eps, swap, K=1.0):
        self.ap, self.an = Dist(a, p, eps), Dist(a, n, eps)
        self.pn = Dist(p, n, eps) if swap else None
        self.margin, self.swap, self.K = f32(margin), bool(swap), K
        R = a.shape[0]
        no, yes = torch.zeros(R, dtype=torch.bool), torch.ones(R, dtype=torch.bool)
        if swap:
            same = self.ap.same                               # a == p bitwise: dan and dpn are the same f32 value
            diff, E = self.pn.d - self.an.d, self.pn.E_d + self.an.E_d
            self.amb_swap = (diff.abs() <= K * E) & ~same
            self.paths = {"an": ((diff > 0) | self.amb_swap) & ~same, "pn": ((diff < 0) | self.amb_swap) & ~same,
                          "tie": same | (diff == 0) | self.amb_swap}
        else:
            self.amb_swap, self.paths = no, {"an": yes}

    def _q(self, path):
        dn = self.pn if path == "pn" else self.an
        q = self.margin + self.ap.d - dn.d
        E_n = torch.maximum(self.an.E_d, self.pn.E_d) if path == "tie" else dn.E_d
        E_q = self.ap.E_d + E_n + 2 * U * ((self.margin + self.ap.d).abs() + q.abs())
        return q, E_q

    def terms(self):
        """(max(margin + dap - min(dan, dpn), 0), bound) per row."""
        dneg = torch.minimum(self.an.d, self.pn.d) if self.swap else self.an.d
        E_n = torch.maximum(self.an.E_d, self.pn.E_d) if self.swap else self.an.E_d
        q = self.margin + self.ap.d - dneg
        return q.clamp(min=0), self.ap.E_d + E_n + 2 * U * ((self.margin + self.ap.d).abs() + q.abs())

    def ambiguous(self):
        amb = self.amb_swap.clone()
        for path, allowed in self.paths.items():
            q, E_q = self._q(path)
            amb |= allowed & (q.abs() <= self.K * E_q)
        return amb

    def options(self, w):
        """{role: options} for roles a, p, n: one option per allowed (swap path, active) branch, the inactive one last."""
        gap, b_ap = self.ap.over_d(w)
        g_an, b_an = self.an.over_d(-w)
        g_pn, b_pn = self.pn.over_d(-w) if self.swap else (None, None)
        z = torch.zeros_like(gap)
        roles = {"a": [], "p": [], "n": []}
        off = torch.zeros(gap.shape[0], dtype=torch.bool)
        for path, allowed in self.paths.items():
            q, E_q = self._q(path)
            amb = q.abs() <= self.K * E_q
            on, off = allowed & ((q > 0) | amb), off | (allowed & (~(q > 0) | amb))
            if path == "an":
                parts = {"a": [(gap, b_ap), (g_an, b_an)], "p": [(-gap, b_ap)], "n": [(-g_an, b_an)]}
            elif path == "pn":
                parts = {"a": [(gap, b_ap)], "p": [(-gap, b_ap), (g_pn, b_pn)], "n": [(-g_pn, b_pn)]}
            else:
                parts = {"a": [(gap, b_ap), (0.5 * g_an, 0.5 * b_an)], "p": [(-gap, b_ap), (0.5 * g_pn, 0.5 * b_pn)],
                         "n": [(-0.5 * g_an, 0.5 * b_an), (-0.5 * g_pn, 0.5 * b_pn)]}
            for role, ps in parts.items():
                ref, mag = sum(r for r, _ in ps), sum(r.abs() for r, _ in ps)
                roles[role].append((ref, sum(b for _, b in ps) + 2 * U * mag, on))
        for role in roles:
            roles[role].append((z, z, off))
        return roles


def check_triplet_fwd(a, p, n, margin, eps, swap, got, what="triplet_fwd"):
    terms, E = Triplet(a, p, n, margin, eps, swap).terms()
    R = a.shape[0]
    s, b = tree_scalar(terms, E, rows_height(R))
    return check_scalar(got, s / R, b / R + U * abs(float(s)) / R, what)


def check_triplet_bwd(a, p, n, margin, eps, swap, scale, gs, got, prev=None, what="triplet_bwd"):
    """got / prev: {role: tensor or None}."""
    roles = Triplet(a, p, n, margin, eps, swap).options(float(w_rows(scale, a.shape[0], gs)))
    out = {}
    for role in "apn":
        if got.get(role) is not None:
            out["d" + role] = check_slots(got[role], None, [roles[role]], 0, f"{what}: d{role}",
                                          prev=None if prev is None else prev.get(role))
    return out


def _term_rows(h0, h1):
    B, T, L = h0.shape
    f = lambda x: x.reshape(B * (T - 1), L)
    return f(h0[:, :-1]), f(h1[:, :-1]), f(h0[:, 1:])


def term_weight(B, T, scale, gs):
    w = f32t(scale) / (f32t(B) * f32t(T - 1))
    return w * f32t(gs) if gs is not None else w


def check_triplet_term_fwd(h0, h1, margin, got, what="triplet_term_fwd"):
    B, T, L = h0.shape
    terms, E = Triplet(*_term_rows(h0, h1), margin, 1e-8, 1).terms()
    s, b = tree_scalar(terms, E, rows_height(B * T))
    nb1 = float(f32t(B) * f32t(T - 1))
    return check_scalar(got, s / nb1, b / nb1 + U * abs(float(s)) / nb1, what)


def _place(opts, B, T, shift):
    """Options over the B (T - 1) triplets -> over the B T rows, at t + shift; the other rows take only the last (zero)
    option."""
    out = []
    for k, (r, b, a) in enumerate(opts):
        L = r.shape[-1]
        R, Bn, A = torch.zeros(B, T, L, dtype=D), torch.zeros(B, T, L, dtype=D), torch.zeros(B, T, dtype=torch.bool)
        if k == len(opts) - 1:
            A[:] = True
        sl = slice(shift, shift + T - 1)
        R[:, sl], Bn[:, sl], A[:, sl] = r.view(B, T - 1, L), b.view(B, T - 1, L), a.view(B, T - 1)
        out.append((R.view(B * T, L), Bn.view(B * T, L), A.view(B * T)))
    return out


def check_triplet_term_bwd(h0, h1, margin, scale, gs, dh0, dh1, what="triplet_term_bwd"):
    B, T, L = h0.shape
    roles = Triplet(*_term_rows(h0, h1), margin, 1e-8, 1).options(float(term_weight(B, T, scale, gs)))
    s0 = [_place(roles["a"], B, T, 0), _place(roles["n"], B, T, 1)]
    return {"dh0": check_slots(dh0.reshape(B * T, L), None, s0, 1, f"{what}: dh0"),
            "dh1": check_slots(dh1.reshape(B * T, L), None, [_place(roles["p"], B, T, 0)], 0, f"{what}: dh1")}


def _triplet32(a, p, n, margin, eps, swap, w, defect=None):
    """(term, ga, gp, gn) per row in f32: triplet_row_bwd with the even split at dpn == dan."""
    tap, dap = rowdist32(a, p, eps)
    tan, dan = rowdist32(a, n, eps)
    zero = torch.zeros_like(dap)
    lam = zero                                        # share of the p - n path
    dneg = dan
    if swap:
        tpn, dpn = rowdist32(p, n, eps)
        lam = torch.where(dpn < dan, zero + 1, torch.where(dpn == dan, zero + 0.5, zero))
        if defect == "tie_to_an":
            lam = torch.where(dpn < dan, zero + 1, zero)
        if defect == "swap_to_larger":
            lam = 1 - lam
        dneg = torch.where(lam == 1, dpn, dan)
    else:
        tpn = torch.zeros_like(tan)
    q = f32t(margin) + dap - dneg
    active = torch.ones_like(q, dtype=torch.bool) if defect == "hinge_not_zeroed" else q > 0
    cap = torch.where(active & (dap > 0), w / dap, zero)[:, None]
    cng = torch.where(active & (dneg > 0), -w / dneg, zero)[:, None]
    gap = cap * tap
    g_an, g_pn = (1 - lam)[:, None] * (cng * tan), lam[:, None] * (cng * tpn)
    term = torch.clamp(f32t(margin) + dap - (torch.minimum(dan, dpn) if swap else dan), min=0)
    return term, gap + g_an, -gap + g_pn, (-g_an) - g_pn


def emu_triplet(a, p, n, margin, eps, swap, scale, gs, prev=None, defect=None):
    """dict(out, a, p, n)."""
    R = a.shape[0]
    term, ga, gp, gn = _triplet32(a, p, n, margin, eps, swap, w_rows(scale, R, gs), defect)
    acc = prev is not None and defect != "accumulate_ignored"
    g = {k: (prev[k] + v if acc else v) for k, v in zip("apn", (ga, gp, gn))}
    return dict(out=rows_sum32(term) / f32t(R), **g)


def emu_triplet_term(h0, h1, margin, scale, gs, defect=None):
    B, T, L = h0.shape
    term, ga, gp, gn = _triplet32(*_term_rows(h0, h1), margin, 1e-8, 1, term_weight(B, T, scale, gs), defect)
    full = torch.zeros(B, T)
    full[:, :-1] = term.view(B, T - 1)
    dh0, dh1 = torch.zeros(B, T, L), torch.zeros(B, T, L)
    for s in range(T - 1):
        dh0[:, s] = dh0[:, s] + ga.view(B, T - 1, L)[:, s]
        dh1[:, s] = dh1[:, s] + gp.view(B, T - 1, L)[:, s]
        dh0[:, s + 1] = dh0[:, s + 1] + gn.view(B, T - 1, L)[:, s]
    return dict(out=rows_sum32(full.reshape(-1)) / (f32t(B) * f32t(T - 1)), dh0=dh0, dh1=dh1)


# ---- KL on logits / codes (kl_fwd_k, kl_bwd_k, binarize_kl_*) ----------------------------------------------------------------

def log_p(p):
    """(log p, log(1 - p)) of the f32 p; the host's logf rounds them once more (2u, in the bounds)."""
    p32 = f32t(p)
    return math.log(float(p32)), math.log(float(f32t(1.0) - p32))


def _xlog_bound(x, dx, e, lc):
    """Bound of the f32 x (log(x + e) - lc) for an operand known to dx (docstring: f' dq, logf, the sum, the products)."""
    lmax = torch.maximum(torch.log((x - dx).clamp(min=0) + e).abs(), torch.log(x + dx + e).abs())
    val = x * (torch.log(x + e) - lc)
    return (dx * (lmax + abs(lc) + 1) + (x + dx) * (2 * U * lmax + U + U * (lmax + abs(lc)) + 2 * U * abs(lc))
            + U * (val.abs() + dx * (lmax + abs(lc))))


def kl_value64(v, p, eps, clamp):
    """(kl_elem(v) in float64, bound) per element."""
    v = v.to(D)
    e, hi = f32(eps), float(f32t(1.0) - f32t(eps))
    lp, l1p = log_p(p)
    q = torch.sigmoid(v)
    dq = c_sig(v, lib=True)
    if clamp:
        q = q.clamp(e, hi)
    om = 1 - q
    f = q * (torch.log(q + e) - lp) + om * (torch.log(om + e) - l1p)
    return f, _xlog_bound(q, dq, e, lp) + _xlog_bound(om, dq + U * om, e, l1p) + U * f.abs()


def check_kl_mean(v, rows, p, eps, clamp, got, what="kl mean"):
    f, E = kl_value64(v.reshape(-1), p, eps, clamp)
    s, b = tree_scalar(f, E, flat_height(f.numel()))
    return check_scalar(got, s / rows, b / rows + U * abs(float(s)) / rows, what)


def check_elementwise(got, alts, what, dims=("element",)):
    """got against alternatives (ref, bnd, allowed mask or None): an element passes within ANY allowed one."""
    got = got.to(D).reshape(-1)
    best = torch.full(got.shape, float("inf"), dtype=D)
    for ref, bnd, allowed in alts:
        err = (got - ref.reshape(-1)).abs()
        r = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err / bnd.reshape(-1))
        if allowed is not None:
            r = torch.where(allowed.reshape(-1), r, torch.full_like(r, float("inf")))
        best = torch.minimum(best, r)
    return _worst(best, torch.ones_like(best), what, dims)


def kl_clamp_ambiguous(v, eps, clamp, K=1.0):
    """Elements whose sigmoid lies within its own error of the clamp mask's lower edge (the upper edge 1 - eps is 1.0f in
    f32 for both eps in use: never active; the results agree there because 1 - s is 0 in f32)."""
    if not clamp:
        return torch.zeros(v.shape, dtype=torch.bool)
    s = torch.sigmoid(v.to(D))
    return (s - f32(eps)).abs() <= K * c_sig(v.to(D), lib=True)


def check_kl_bwd(v, rows, p, eps, clamp, scale, gs, got, what="kl_bwd"):
    w = float(w_rows(scale, rows, gs))
    gr, E = kl_grad64(v.to(D), f32(p), f32(eps), clamp)
    ref = w * gr
    bnd = abs(w) * (E + TINY_F32) + U * ref.abs() + TINY_DEN
    amb = kl_clamp_ambiguous(v, eps, clamp)
    gr2, E2 = kl_grad64(v.to(D), f32(p), f32(eps), 0)
    other = torch.where(gr == 0, w * gr2, torch.zeros_like(gr))              # the other side of the mask
    b2 = torch.where(gr == 0, abs(w) * (E2 + TINY_F32) + U * other.abs(), torch.zeros_like(gr)) + TINY_DEN
    return check_elementwise(got, [(ref, bnd, None), (other, b2, amb)], what)


def kl_elem32(v, p, eps, clamp, defect=None):
    p32, e = f32t(p), f32t(eps)
    lp, l1p = torch.log(p32), torch.log(1.0 - p32)
    if defect == "lp_swapped":
        lp, l1p = l1p, lp
    q = sig32(v.to(F))
    if clamp:
        q = torch.minimum(torch.maximum(q, e), 1.0 - e)
    return q * (torch.log(q + e) - lp) + (1.0 - q) * (torch.log((1.0 - q) + e) - l1p)


def kl_grad32(v, p, eps, clamp, defect=None):
    p32, e = f32t(p), f32t(eps)
    lp, l1p = torch.log(p32), torch.log(1.0 - p32)
    s = sig32(v.to(F))
    q = torch.minimum(torch.maximum(s, e), 1.0 - e) if clamp else s
    ok = (s >= e) & (s <= 1.0 - e) if (clamp and defect != "clamp_mask_ignored") else torch.ones_like(s, dtype=torch.bool)
    om = 1.0 - q
    dq = (torch.log(q + e) - lp) + q / (q + e) - (torch.log(om + e) - l1p) - om / (om + e)
    return torch.where(ok, dq * s * (1.0 - s), torch.zeros_like(s))


def emu_kl_mean(v, rows, p, eps, clamp, defect=None):
    tot = block_sum32(strided32(kl_elem32(v.reshape(-1), p, eps, clamp, defect), 1024))
    return tot / f32t(v.numel() if defect == "kl_mean_over_all" else rows)


def emu_kl_bwd(v, rows, p, eps, clamp, scale, gs, defect=None):
    return w_rows(scale, rows, gs) * kl_grad32(v, p, eps, clamp, defect)


def emu_binarize(h, u, tau, ratio, neps, hard, defect=None):
    """(y_soft, z) in f32."""
    u, ne = u.to(F), (f32t(0.0) if defect == "no_neps" else f32t(neps))
    noise = f32t(ratio) * (torch.log(u + ne) - torch.log(1.0 - u + ne))
    y = sig32((h.to(F) + noise) / f32t(tau))
    return y, ((y > 0.5).float() if hard else y)


def check_binarize_bwd(gz, y, z, prev, rows, tau, klw, gs, p, eps, clamp, got, what="binarize_kl_bwd"):
    """dh of binarize_kl_bwd_k through gtop_bin; prev: the preloaded dh of accumulate = 1 (or None)."""
    gz64 = torch.zeros(y.shape, dtype=D) if gz is None else gz.to(D)
    kw = klw * gs if gs is not None else klw
    ref, bnd = gtop_bin(gz64, torch.zeros_like(gz64), y, z, prev, tau, kw, rows, p, f32(eps), clamp)
    if gs is not None and klw != 0.0:
        kg, _ = kl_grad64(z.to(D), f32(p), f32(eps), clamp)
        bnd = bnd + 2 * U * (kw / rows * kg * y.to(D) * (1 - y.to(D)) / f32(tau)).abs()
    return _worst((got.to(D) - ref).abs(), bnd, what, ("row", "unit"))


def emu_binarize_bwd(gz, y, z, prev, rows, tau, klw, gs, p, eps, clamp, defect=None):
    w = w_rows(klw, rows, gs)
    g = torch.zeros_like(y) if gz is None else gz.to(F)
    if float(w) != 0.0:
        g = g + w * kl_grad32(z, p, eps, clamp, defect)
    val = g * y * (1.0 - y) / f32t(tau)
    return prev + val if (prev is not None and defect != "accumulate_ignored") else val


# ---- MSE ---------------------------------------------------------------------------------------------------------------------

def check_mse_fwd(a, b, got, what="mse_fwd"):
    n = a.numel()
    d2 = ((a.to(D) - b.to(D)) ** 2).sum()
    ref = float(d2) / f32(n)
    return check_scalar(got, ref, (3 * U * (1 + 2.0 ** -20) + gamma(mse_height(n))) * ref + U * ref, what)


def mse_weight(n, scale, gs):
    w = (2.0 * f32t(scale)) / f32t(n)
    return w * f32t(gs) if gs is not None else w


def check_mse_bwd(a, b, scale, gs, got, what="mse_bwd"):
    ref = float(mse_weight(a.numel(), scale, gs)) * (a.to(D) - b.to(D))
    return _worst((got.to(D) - ref).abs(), 2 * U * ref.abs() + TINY_DEN, what, ("element",))


def emu_mse_fwd(a, b, defect=None):
    n = a.numel()
    n4, nb = n >> 2, mse_blocks(n)
    d = a.to(F) - b.to(F)
    sq = d * d
    q = sq[:4 * n4].view(n4, 4)
    acc = strided32(((q[:, 0] + q[:, 1]) + q[:, 2]) + q[:, 3], nb * 256)
    if defect != "mse_tail_dropped":
        for k, i in enumerate(range(4 * n4, n)):
            acc[k] = acc[k] + sq[i]
    w = wave_sum32(acc.view(nb, 4, 64))
    ws = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    v = torch.zeros(512, dtype=F)
    v[:nb] = ws
    return block_sum32(v) / f32t(n)


def emu_mse_bwd(a, b, scale, gs):
    return mse_weight(a.numel(), scale, gs) * (a.to(F) - b.to(F))


# ---- combine_losses_k and the hyper terms -------------------------------------------------------------------------------------

def _flat_tree(vals):
    vals = vals.to(D)
    return float(vals.sum()), float(gamma(flat_height(vals.numel())) * vals.abs().sum())


def check_combine(c, out4, what="combine_losses"):
    """c: the arguments (sse_ws / recon / kl / pair tensors, counts, scales).  out4[1..3] against float64 of the partial
    sums (bit for bit where the count is 0), out4[0] against the kernel's own out4[1..3]."""
    o = [float(x) for x in out4.to(D)]
    res = {}
    if c["sse_ws"] is not None:
        s, b = _flat_tree(c["sse_ws"][:c["nparts"]])
        inv = f32(c["inv_n"])
        res["recon"] = check_scalar(o[1], s * inv, b * abs(inv) + U * abs(s * inv), f"{what}: recon")
    else:
        assert bool(out4[1] == c["recon"][0]), f"{what}: recon is not passed through bit for bit"
    if c["kl_parts"] > 0:
        s, b = _flat_tree(c["kl"][:c["kl_parts"]])
        ks = f32(c["kl_scale"])
        res["kl"] = check_scalar(o[2], s * ks, b * abs(ks) + U * abs(s * ks), f"{what}: kl")
    else:
        assert bool(out4[2] == c["kl"][0]), f"{what}: kl is not passed through bit for bit"
    if c["pair_parts"] > 0:
        pr = c["pair"][:2 * c["pair_parts"]].view(-1, 2)
        (s0, b0), (s1, b1) = _flat_tree(pr[:, 0]), _flat_tree(pr[:, 1])
        ws, wd = f32(c["w_sim"]), f32(c["w_dis"])
        ref = ws * s0 + wd * s1
        res["pair"] = check_scalar(o[3], ref, abs(ws) * b0 + abs(wd) * b1 + U * (abs(ws * s0) + abs(wd * s1) + abs(ref)),
                                   f"{what}: pair")
    else:
        assert bool(out4[3] == c["pair"][0]), f"{what}: pair is not passed through bit for bit"
    beta, alpha = f32(c["beta"]), f32(c["alpha"])
    ref = o[1] + beta * o[2] + alpha * o[3]
    bnd = 2 * U * (abs(beta * o[2]) + abs(alpha * o[3])) + U * (abs(o[1] + beta * o[2]) + abs(ref))
    res["total"] = check_scalar(o[0], ref, bnd, f"{what}: total")
    return res


def emu_combine(c, defect=None):
    def tree(v, n):
        v = v[:min(n, 1024)] if defect == "combine_drops_1024" else v[:n]
        return block_sum32(strided32(v.to(F), 1024))
    recon = tree(c["sse_ws"], c["nparts"]) * f32t(c["inv_n"]) if c["sse_ws"] is not None else c["recon"][0]
    k = tree(c["kl"], c["kl_parts"]) * f32t(c["kl_scale"]) if c["kl_parts"] > 0 else c["kl"][0]
    if c["pair_parts"] > 0:
        pr = c["pair"][:2 * c["pair_parts"]].view(-1, 2)
        p = f32t(c["w_sim"]) * tree(pr[:, 0].contiguous(), c["pair_parts"]) + f32t(c["w_dis"]) * tree(pr[:, 1].contiguous(), c["pair_parts"])
    else:
        p = c["pair"][0]
    beta, alpha = f32t(c["beta"]), f32t(c["alpha"])
    if defect == "alpha_beta_exchanged":
        beta, alpha = alpha, beta
    return torch.stack([recon + beta * k + alpha * p, recon, k, p]).to(F)


def hyper_ref(lr, b1, b2, t):
    """[(hyper[0], bound), (hyper[1], bound)] for step t in numpy longdouble (module docstring: the device pow)."""
    ld = np.longdouble
    p1, p2 = ld(b1) ** ld(t), ld(b2) ** ld(t)
    h0, h1 = ld(lr) / (1 - p1), np.sqrt(1 - p2)
    r0 = K_POW * 2.0 ** -53 * float(p1 / (1 - p1)) + 3 * 2.0 ** -53
    r1 = K_POW * 2.0 ** -53 * float(p2 / (1 - p2)) / 2 + 3 * 2.0 ** -53
    return [(float(h0), (U * (1 + 1e-6) + r0) * abs(float(h0))), (float(h1), (U * (1 + 1e-6) + r1) * abs(float(h1)))]


def check_hyper(hyper, lr, b1, b2, t, what="hyper"):
    ref = hyper_ref(lr, b1, b2, t)
    return {f"hyper{k}": check_scalar(hyper[k], ref[k][0], ref[k][1], f"{what}[{k}] at step {t}") for k in (0, 1)}


def emu_hyper(lr, b1, b2, step_before, defect=None):
    """The device's double arithmetic for the step that follows step_before."""
    t = np.float64(step_before if defect == "hyper_for_t" else step_before + 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return torch.tensor([np.float32(np.float64(lr) / (1.0 - np.float64(b1) ** t)),
                             np.float32(np.sqrt(1.0 - np.float64(b2) ** t))], dtype=F)


def host_hyper(lr, b1, b2, step):
    """rbvae_adam_step's `step` form: (float)(lr / (1 - b1^step)), (float)sqrt(1 - b2^step) on the host."""
    return f32(lr / (1.0 - b1 ** float(step))), f32(math.sqrt(1.0 - b2 ** float(step)))


# ---- Adam -----------------------------------------------------------------------------------------------------------------------

def adam_consts(b1, b2, eps, gscale):
    """The f32 constants adam_k / AdamCtx receive."""
    return dict(omb1=f32(1.0 - b1), b2=f32(b2), omb2=f32(1.0 - b2), eps=f32(eps), gscale=f32(gscale))


def adam_ref(w, g, m, v, k, step, bc2):
    """{name: (ref, bound)} of one adam_update per element; k = adam_consts, step / bc2 the f32 hyper values."""
    w, g, m, v = (x.to(D) for x in (w, g, m, v))
    gi = g * k["gscale"]
    m1 = k["omb1"] * (gi - m) + m
    E_m = k["omb1"] * U * (gi.abs() + (gi - m).abs()) + U * m1.abs() + TINY_DEN
    v1 = k["omb2"] * gi * gi + v * k["b2"]
    E_v = (3 * U * k["omb2"] * gi * gi + U * (v * k["b2"]).abs() + U * v1.abs()) * (1 + 1e-6) + TINY_DEN
    sq = v1.sqrt()
    E_sq = torch.minimum(E_v / (sq + (v1 - E_v).clamp(min=0).sqrt()).clamp(min=1e-300), E_v.sqrt()) + U * sq
    den = sq / bc2 + k["eps"]
    E_den = E_sq / bc2 + U * sq / bc2 + U * den
    lo = (den - E_den).clamp(min=1e-300)
    r = m1 / den
    E_r = (E_m / lo + m1.abs() * E_den / (den * lo) + U * r.abs()) * (1 + 1e-6)
    w1 = w - step * r
    E_w = step * E_r + U * w1.abs() + TINY_DEN
    return {"w": (w1, E_w), "m": (m1, E_m), "v": (v1, E_v)}


def check_adam(ref, w1, m1, v1, what="adam", dims=("element",)):
    return {n: _worst((x.to(D).reshape(-1) - ref[n][0].reshape(-1)).abs(), ref[n][1].reshape(-1), f"{what}: {n}", dims)
            for n, x in (("w", w1), ("m", m1), ("v", v1))}


def _fma32(a, b, c):
    return (a.to(D) * b.to(D) + c.to(D)).to(F)


def emu_adam(w, g, m, v, k, step, bc2, defect=None):
    """adam_update in f32 with its fma placement -> (w', m', v')."""
    w, g, m, v = (x.to(F) for x in (w, g, m, v))
    c = {n: f32t(x) for n, x in k.items()}
    gi = g * c["gscale"]
    m1 = _fma32(c["omb1"], gi - m, m)
    gv = g if defect == "gscale_missing_in_v" else gi
    v1 = _fma32(c["omb2"] * gv, gv, v * c["b2"])
    if defect == "eps_inside_sqrt":
        den = torch.sqrt(v1 + c["eps"]) / f32t(bc2)
    elif defect == "bc2_on_v":
        den = torch.sqrt(v1 / f32t(bc2)) + c["eps"]
    else:
        den = torch.sqrt(v1) / f32t(bc2) + c["eps"]
    return _fma32(-f32t(step), m1 / den, w), m1, v1


# ---- the fused update jobs (run_jobs_k kinds 3-with-context, 6, 7) ----------------------------------------------------------------

F32_T, BF16_T = 0, 1                       # RBVAE_F32 / RBVAE_BF16
TDT = {F32_T: F, BF16_T: BF}
CPK_MAXROW, CPK_CIB = 2304, 64


def job(id, kind, dims, dtype=F32_T, copies=()):
    """kind 7: dims (n, 1, 1).  kind 3: dims (Co, Ci, kk), both GEMM orders in `dtype`.  kind 6: copies = one or two
    (dtype, (s0, s1, s2)) scatter maps of the [d0][d1][d2] tensor."""
    return dict(id=id, kind=kind, dims=tuple(dims), dtype=dtype, copies=tuple(copies))


def job_numel(j):
    return j["dims"][0] * j["dims"][1] * j["dims"][2]


def copy_maps(j):
    """[(dtype, destination offset of every master element in master order)] of a job's packed copies."""
    d0, d1, d2 = j["dims"]
    i0, i1, i2 = torch.meshgrid(torch.arange(d0), torch.arange(d1), torch.arange(d2), indexing="ij")
    if j["kind"] == 3:
        return [(j["dtype"], ((i0 * d2 + i2) * d1 + i1).reshape(-1)), (j["dtype"], ((i1 * d2 + i2) * d0 + i0).reshape(-1))]
    return [(dt, (i0 * s[0] + i1 * s[1] + i2 * s[2]).reshape(-1)) for dt, s in j["copies"]]


def conv_pack_path(j):
    """Which input path conv_pack_rows takes: ('vec' | 'elem', ci pieces per row)."""
    Co, Ci, kk = j["dims"]
    nv = 4 if j["dtype"] == F32_T else 8
    cib = min((CPK_MAXROW // kk) // nv * nv, Ci)
    if cib > CPK_CIB and Ci % CPK_CIB == 0:
        cib = CPK_CIB
    vec = Ci % nv == 0 and Co % nv == 0 and (cib * kk) % 4 == 0 and (Ci * kk) % 4 == 0
    return ("vec" if vec else "elem"), cdiv(Ci, cib)


def tile_shape(j):
    """(T0, T1, T2, fA, fB) of the tiled kind-6 path, or None where the flat loop runs (restates run_jobs_k)."""
    if j["kind"] != 6 or job_numel(j) < (1 << 20):
        return None
    a = j["copies"][0][1]
    fA = 0 if a[0] == 1 else (1 if a[1] == 1 else 2)
    fB = fA
    if len(j["copies"]) == 2:
        c = j["copies"][1][1]
        fB = 0 if c[0] == 1 else (1 if c[1] == 1 else 2)
    if fA == 2 and fB == 2:
        return None
    if fA != 2 and fB != 2 and fA != fB:
        T2, T0, T1 = 16, (32 if fB == 0 else 16), (32 if fB == 1 else 16)
    else:
        f = fA if fA != 2 else fB
        T2, T0, T1 = 32, (32 if f == 0 else 8), (32 if f == 1 else 8)
    d0, d1, d2 = j["dims"]
    return min(T0, d0), min(T1, d1), min(T2, d2), fA, fB


def job_kernel(j):
    """The branch of run_jobs_k a job takes (for the coverage table)."""
    if j["kind"] == 7:
        return "run_jobs_k[7]"
    if j["kind"] == 3:
        path, pieces = conv_pack_path(j)
        return f"run_jobs_k[3,ctx,{path},{'f32' if j['dtype'] == F32_T else 'bf16'}{',split' if pieces > 1 else ''}]"
    ts = tile_shape(j)
    if ts is None:
        return f"run_jobs_k[6,flat,{len(j['copies'])}]"
    fA, fB = ts[3], ts[4]
    cls = "one" if len(j["copies"]) == 1 else ("same" if fA == fB else ("mixed" if 2 in (fA, fB) else "different"))
    return f"run_jobs_k[6,tiled,{cls}]"


def emu_job(j, w, g, m, v, k, step, bc2, defect=None):
    """(w', m', v', [packed copies]) of one job on its slice of the flat buffers."""
    w1, m1, v1 = emu_adam(w, g, m, v, k, step, bc2)
    ts = tile_shape(j)
    if defect == "ragged_tile_skipped" and ts is not None:
        d = j["dims"]
        i = torch.meshgrid(*[torch.arange(x) for x in d], indexing="ij")
        skip = torch.zeros(d, dtype=torch.bool)
        for ax in range(3):
            if d[ax] % ts[ax]:
                skip |= i[ax] >= d[ax] // ts[ax] * ts[ax]
        skip = skip.reshape(-1)
        w1, m1, v1 = torch.where(skip, w, w1), torch.where(skip, m, m1), torch.where(skip, v, v1)
    copies = []
    for dt, idx in copy_maps(j):
        c = torch.zeros(job_numel(j), dtype=TDT[dt])
        c[idx] = (w if defect == "pack_from_old_weight" else w1).to(TDT[dt])
        copies.append(c)
    return w1, m1, v1, copies


def check_job(j, w, g, m, v, k, step, bc2, w1, m1, v1, copies, what=None):
    """Master elements against the float64 Adam reference; every packed copy bit for bit the storage rounding of the
    stored master element at the job's index."""
    what = what or j["id"]
    res = check_adam(adam_ref(w, g, m, v, k, step, bc2), w1, m1, v1, what=what)
    for q, ((dt, idx), c) in enumerate(zip(copy_maps(j), copies)):
        assert idx.unique().numel() == idx.numel() == c.numel(), f"{what}: copy {q} is not a permutation"
        _exact(c.reshape(-1)[idx], w1.reshape(-1).to(TDT[dt]), f"{what}: packed copy {q}", ("master element",))
    return res


# ---- case tables ------------------------------------------------------------------------------------------------------------------
# L in {1, 16, 25, 32, 50, 63, 64, 65, 100, 128, 200}; rows in {1, 3, 15, 16, 17, 64, 1000} (fewer than, equal to and more
# than the 16 waves of the one-workgroup forwards; rows % 4 != 0 is the tail of the 4-rows-per-block backwards); T in
# {2, 3, 8, 17}; B in {1, 2, 5, 16}.  Regimes: "spread" (distances alternate between 0.3 and 2.5 times the unit, so both
# hinge branches hold at least MIN_SHARE of the rows of every case with at least 4 rows), "close" (second operand = first
# + 1e-3 noise: eps = 1e-6 is visible against the difference), "offset" (spread, + 50: cancellation in a - b).
# special: rows built on a threshold (module docstring).

MIN_SHARE = 0.25
C_LO, C_HI = 0.3, 2.5


def ru4(n):
    return (n + 3) // 4 * 4


def gen_of(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def unit_rows(gen, R, L):
    x = torch.randn(R, L, generator=gen, dtype=D)
    return x / x.norm(dim=-1, keepdim=True)


def alternating(gen, R, unit, phase=0):
    c = torch.where((torch.arange(R) + phase) % 2 == 0, torch.tensor(C_LO, dtype=D), torch.tensor(C_HI, dtype=D))
    return (c * unit * (0.9 + 0.2 * torch.rand(R, generator=gen, dtype=D)))[:, None]


def second_operand(x, regime, gen, unit=1.0, phase=0):
    R, L = x.shape
    if regime == "close":
        return x + 1e-3 * torch.randn(R, L, generator=gen, dtype=D)
    return x + unit_rows(gen, R, L) * alternating(gen, R, unit, phase)


def first_operand(gen, R, L, regime):
    return torch.randn(R, L, generator=gen, dtype=D) * 0.5 + (50.0 if regime == "offset" else 0.0)


def pc(rows, L, label, regime, margin=1.0, eps=1e-6, pad=(0, 0), dpad=(0, 0), acc=0, nulls=(), gs=None, scale=1.0, special=False):
    c = dict(rows=rows, L=L, label=label, regime=regime, margin=margin, eps=eps, s1=ru4(L) + 4 * pad[0], s2=ru4(L) + 4 * pad[1],
             ds1=ru4(L) + 4 * dpad[0], ds2=ru4(L) + 4 * dpad[1], acc=acc, nulls=tuple(nulls), gs=gs, scale=scale, special=special)
    c["id"] = f"rows{rows}-L{L}-label{label}-{regime}" + ("-special" if special else "")
    return c


PAIR_CASES = [
    pc(1, 1, 1, "spread", margin=5.0),
    pc(3, 16, 0, "close", acc=1, gs=0.5, pad=(1, 0), dpad=(0, 2)),
    pc(15, 25, 1, "spread", pad=(1, 2), dpad=(3, 0), nulls=("dx2",)),
    pc(16, 32, 1, "offset", scale=0.7),
    pc(17, 50, 0, "spread", nulls=("dx1",), acc=1, pad=(0, 1), dpad=(2, 1)),
    pc(64, 63, 1, "close", gs=1.0 / 1024, pad=(2, 0), dpad=(0, 1)),
    pc(64, 64, 1, "spread", special=True, acc=1, pad=(1, 1), dpad=(2, 3)),
    pc(1000, 65, 1, "spread", scale=3.0),
    pc(3, 100, 0, "offset", pad=(1, 3), dpad=(0, 0)),
    pc(17, 128, 1, "spread", gs=0.5, margin=0.8, pad=(0, 2), dpad=(1, 0)),
    pc(15, 200, 1, "spread", special=True, pad=(1, 0), dpad=(0, 1)),
]


def pair_data(c):
    g = gen_of(c["rows"], c["L"], c["label"], len(c["regime"]))
    x1 = first_operand(g, c["rows"], c["L"], c["regime"])
    x2 = second_operand(x1, c["regime"], g, unit=c["margin"])
    x1, x2 = x1.float(), x2.float()
    if c["special"]:
        x1[0], x2[0] = 0.0, f32(c["eps"])          # a - b + eps == 0 exactly: d = 0, gradient 0, no NaN
        x2[1] = x1[1]                               # a == b: d = eps sqrt(L), coefficient m / d ~ 1e6 / sqrt(L)
        x2[2] = x1[2] + 100.0                       # d far above the margin
    return x1, x2


def prev_of(c, name, shape):
    """The preloaded gradient of accumulate = 1."""
    return torch.randn(*shape, generator=gen_of(c["rows"], c["L"], len(name), 17)) if c["acc"] else None


COS_CASES = [
    pc(1, 1, 0, "cos", margin=0.8, eps=1e-8),
    pc(3, 16, 1, "cos", margin=0.8, eps=1e-8, gs=0.5, pad=(1, 0), dpad=(0, 2)),
    pc(16, 25, 0, "cos", margin=0.8, eps=1e-8, pad=(1, 2), dpad=(3, 0), nulls=("dx2",)),
    pc(17, 64, 1, "cos", margin=0.8, eps=1e-8, special=True, scale=1.5),
    pc(64, 65, 1, "cos", margin=0.8, eps=1e-8, nulls=("dx1",), pad=(0, 1), dpad=(1, 1)),
    pc(1000, 32, 0, "cos", margin=0.8, eps=1e-8),
    pc(15, 200, 1, "cos", margin=0.8, eps=1e-8, special=True, pad=(1, 0), dpad=(0, 1)),
]


def cos_data(c):
    g = gen_of(c["rows"], c["L"], c["label"], 5)
    x1 = torch.randn(c["rows"], c["L"], generator=g)
    x2 = torch.randn(c["rows"], c["L"], generator=g) + 0.3
    if c["special"]:
        x1[0] = 0.0                                 # na <= eps: the clamped norm is a constant
        x1[1], x2[1] = 0.0, 0.0
        x2[2] = 0.0
    return x1, x2


def tc(rows, L, swap, margin, regime, pad=(0, 0, 0), dpad=(0, 0, 0), acc=0, nulls=(), gs=None, scale=1.0, special=False):
    c = dict(rows=rows, L=L, swap=swap, margin=margin, regime=regime, eps=1e-8, acc=acc, nulls=tuple(nulls), gs=gs, scale=scale,
             special=special, s=tuple(ru4(L) + 4 * p for p in pad), ds=tuple(ru4(L) + 4 * p for p in dpad))
    c["id"] = f"rows{rows}-L{L}-swap{swap}-m{margin}-{regime}" + ("-special" if special else "")
    return c


TRIPLET_CASES = [
    tc(1, 1, 1, 0.2, "spread"),
    tc(3, 16, 0, 1.0, "close", acc=1, gs=0.5, pad=(1, 0, 2), dpad=(0, 2, 1)),
    tc(15, 25, 1, 1.0, "spread", pad=(1, 2, 0), dpad=(3, 0, 1), nulls=("p",)),
    tc(16, 32, 1, 0.2, "offset", scale=0.7),
    tc(17, 50, 1, 0.2, "spread", nulls=("a", "n"), acc=1, pad=(0, 1, 1), dpad=(2, 1, 0)),
    tc(64, 63, 0, 0.2, "spread", gs=1.0 / 1024),
    tc(64, 64, 1, 1.0, "spread", special=True, acc=1, pad=(1, 1, 0), dpad=(2, 3, 1)),
    tc(1000, 65, 1, 1.0, "spread", scale=3.0),
    tc(3, 100, 1, 0.2, "close", pad=(1, 3, 0)),
    tc(17, 128, 1, 1.0, "spread", gs=0.5, pad=(0, 2, 1), dpad=(1, 0, 2)),
    tc(15, 200, 1, 10.0, "spread", special=True),
]


def beside(gen, dirs, size, R):
    """Rows of length `size` at a fixed angle to the unit rows `dirs`: +-0.6 along them (the sign alternates every two rows)
    and 0.8 across, so |p - n| and |a - n| differ by a margin no rounding reaches and both swap choices occur."""
    L = dirs.shape[-1]
    sgn = torch.where((torch.arange(R) // 2) % 2 == 0, 1.0, -1.0).to(D)[:, None]
    if L == 1:
        return sgn * dirs * size
    o = torch.randn(R, L, generator=gen, dtype=D)
    o = o - (o * dirs).sum(-1, keepdim=True) * dirs
    return (0.6 * sgn * dirs + 0.8 * o / o.norm(dim=-1, keepdim=True)) * size


def close_size(gen, R, L):
    """|h1 - h0| of the "close" regime: 1e-3 per component."""
    return (1e-3 * L ** 0.5 * (0.5 + torch.rand(R, generator=gen, dtype=D)))[:, None]


def triplet_rows_data(g, R, L, regime, phase=0):
    a = first_operand(g, R, L, regime)
    dn = unit_rows(g, R, L)
    p = a + beside(g, dn, close_size(g, R, L) if regime == "close" else C_LO, R)
    n = a + dn * alternating(g, R, 1.0, phase)
    return a.float(), p.float(), n.float()


def triplet_data(c):
    g = gen_of(c["rows"], c["L"], c["swap"], 3)
    a, p, n = triplet_rows_data(g, c["rows"], c["L"], c["regime"])
    if c["special"]:
        p[0] = a[0]                                 # bitwise equal views: dpn == dan exactly (the swap tie)
        a[1], p[1] = 0.0, f32(c["eps"])             # a - p + eps == 0: dap = 0
        n[2] = a[2] + 100.0                         # far above the margin: inactive
        p[3] = a[3]
    return a, p, n


def sc(B, T, L, regime, scale=1.0, gs=None, margin=0.2, special=None):
    c = dict(B=B, T=T, L=L, regime=regime, scale=scale, gs=gs, margin=margin, special=special)
    c["id"] = f"B{B}-T{T}-L{L}-{regime}" + (f"-{special}" if special else "")
    return c


TERM_CASES = [
    sc(1, 2, 1, "spread"),
    sc(2, 3, 16, "close", scale=0.5, gs=0.5),
    sc(5, 8, 25, "spread", margin=1.0),
    sc(16, 17, 32, "offset", gs=1.0 / 1024),
    sc(2, 2, 50, "spread", scale=2.0),
    sc(5, 3, 63, "close"),
    sc(16, 8, 64, "spread", margin=1.0, gs=0.5),
    sc(1, 17, 65, "spread"),
    sc(2, 8, 100, "offset", scale=0.7),
    sc(5, 2, 128, "spread"),
    sc(16, 3, 200, "spread", margin=1.0),
    sc(2, 3, 32, "spread", special="equal-views", margin=10.0),
    sc(5, 17, 25, "spread", special="equal-views", margin=1.0),
    sc(2, 3, 25, "spread", special="zero-distance"),
    sc(3, 2, 64, "spread", special="far"),
]


def term_data(c):
    """h0, h1 [B][T][L]: consecutive states of h0 alternate between C_LO and C_HI apart; h1 is h0 + C_LO (or + 1e-3 per component) at a fixed angle to the step."""
    B, T, L = c["B"], c["T"], c["L"]
    g = gen_of(B, T, L, len(c["regime"]))
    h0, h1 = torch.zeros(B, T, L, dtype=D), torch.zeros(B, T, L, dtype=D)
    h0[:, 0] = first_operand(g, B, L, c["regime"])
    for t in range(T):
        dn = unit_rows(g, B, L)                     # towards the next state
        if t + 1 < T:
            h0[:, t + 1] = h0[:, t] + dn * alternating(g, B, 1.0, phase=t)
        h1[:, t] = h0[:, t] + beside(g, dn, close_size(g, B, L) if c["regime"] == "close" else C_LO, B)
    h0, h1 = h0.float(), h1.float().view(B, T, L)
    if c["special"] == "equal-views":
        h1 = h0.clone()                             # two identical views: every triplet is an exact swap tie
        if T > 2:
            h1[:, 1] = h0[:, 1] + 0.25              # ... except at t = 1
    elif c["special"] == "zero-distance":
        h0[0, 0], h0[0, 1] = 0.0, f32(C_EPS)        # contrast: a - a' + 1e-6 == 0
        h1[1, 0] = h0[1, 0]                         # a == b: d = eps sqrt(L)
        h0[1, 1], h1[1, 1] = 0.0, f32(1e-8)         # triplet: a - p + 1e-8 == 0
    elif c["special"] == "far":
        h0[:, 1] = h0[:, 0] + 100.0
    return h0.contiguous(), h1.contiguous()


def bc(rows, L, U, logits="randn", tau=0.7, ratio=0.3, neps=1e-8, hard=0, p=0.1, keps=1e-8, clamp=1, seed=0, seed_dev=None,
       tau_dev=False, klw=0.3, gs=None, acc=0, gz=True):
    c = dict(rows=rows, L=L, U=U, logits=logits, tau=tau, ratio=ratio, neps=neps, hard=hard, p=p, keps=keps, clamp=clamp, seed=seed,
             seed_dev=seed_dev, tau_dev=tau_dev, klw=klw, gs=gs, acc=acc, gz=gz)
    c["id"] = f"rows{rows}-L{L}-U{U}-{logits}-hard{hard}-p{p}-clamp{clamp}" + ("-taudev" if tau_dev else "") + ("-seeddev" if seed_dev else "")
    return c


# n = rows * L on both sides of binarize_kl_fwd_k's batch of 8 * 1024 elements; n % 256 != 0 for the parts kernel
BIN_CASES = [
    bc(1, 1, "rand"),
    bc(3, 25, "edges", logits="edges", hard=1, acc=1, gs=0.5),
    bc(7, 16, "edges", logits="edges", hard=0, p=0.5, clamp=0, keps=1e-10, tau=0.5, tau_dev=True),
    bc(255, 32, "rand", hard=1, p=0.5, tau_dev=True, klw=0.0),
    bc(256, 32, "rand", hard=0, clamp=0, keps=1e-10, gz=False),
    bc(257, 32, "rand", hard=1, tau=1.3, ratio=1.0, gs=1.0 / 1024),
    bc(1000, 50, "rand", hard=0, p=0.5, acc=1),
    bc(17, 100, None, seed=12345, hard=0),
    bc(64, 63, None, seed=(1 << 63) + 77, seed_dev=3, hard=1, clamp=0, keps=1e-10),
    bc(300, 32, None, seed=7, seed_dev=(1 << 40) + 1, hard=0, p=0.5, tau_dev=True),
]

EDGE_LOGITS = (0.0, 20.0, -20.0, 90.0, -90.0, 104.0, -104.0)
EDGE_U = (0.0, 2.0 ** -24, 0.5, 1.0 - 2.0 ** -24)


def cycle(vals, n):
    return torch.tensor(vals, dtype=F).repeat(cdiv(n, len(vals)))[:n]


def bin_data(c):
    """h, U (None: the device-side hash), g_z, preloaded dh."""
    n = c["rows"] * c["L"]
    g = gen_of(c["rows"], c["L"], c["hard"], 11)
    h = cycle(EDGE_LOGITS, n) if c["logits"] == "edges" else torch.randn(n, generator=g) * 2
    Un = None if c["U"] is None else (cycle(EDGE_U, n) if c["U"] == "edges" else torch.rand(n, generator=g))
    gz = torch.randn(n, generator=g) if c["gz"] else None
    prev = torch.randn(n, generator=g) if c["acc"] else None
    sh = (c["rows"], c["L"])
    return h.view(sh), None if Un is None else Un.view(sh), None if gz is None else gz.view(sh), None if prev is None else prev.view(sh)


def kc(rows, L, p, eps, clamp, logits, scale=1.0, gs=None):
    c = dict(rows=rows, L=L, p=p, eps=eps, clamp=clamp, logits=logits, scale=scale, gs=gs)
    c["id"] = f"rows{rows}-L{L}-p{p}-eps{eps}-clamp{clamp}-{logits}"
    return c


KL_CASES = [kc(1, 1, 0.1, 1e-8, 1, "randn"), kc(3, 25, 0.1, 1e-8, 1, "edges", scale=0.3, gs=0.5),
            kc(7, 16, 0.5, 1e-10, 0, "edges"), kc(64, 100, 0.5, 1e-8, 1, "randn", scale=2.0),
            kc(1000, 16, 0.1, 1e-10, 0, "randn", gs=1.0 / 1024), kc(17, 63, 0.1, 1e-8, 1, "wide")]


def kl_data(c):
    n = c["rows"] * c["L"]
    g = gen_of(c["rows"], c["L"], c["clamp"], 13)
    if c["logits"] == "edges":
        v = cycle(EDGE_LOGITS, n)
    else:
        v = torch.randn(n, generator=g) * (6.0 if c["logits"] == "wide" else 2.0)
    return v.view(c["rows"], c["L"])


# n = 2^23 + 1 reaches mse_partial_k's 512-block cap: the GPU file only
MSE_CASES = [dict(id=f"n{n}", n=n, scale=s, gs=gs, gpu_only=n > (1 << 21))
             for n, s, gs in ((1, 1.0, None), (3, 0.5, 0.5), (4, 1.0, None), (1027, 2.0, None), ((1 << 20) + 3, 0.5, 1.0 / 1024),
                              ((1 << 23) + 1, 1.0, None))]


def mse_data(c):
    g = gen_of(c["n"], 19)
    return torch.rand(c["n"], generator=g), torch.rand(c["n"], generator=g)


COUNTS = (0, 1, 1023, 1024, 1025, 4096)


def cc(k, step=None, lr_dev=None):
    """nparts / kl_parts / pair_parts rotate through COUNTS; nparts == 0 hands recon in instead of sse_ws."""
    n, kp, pp = COUNTS[k % 6], COUNTS[(k + 1) % 6], COUNTS[(k + 2) % 6]
    return dict(id=f"n{n}-kl{kp}-pair{pp}-step{step}" + ("-lrdev" if lr_dev else ""), nparts=n, kl_parts=kp, pair_parts=pp, step=step,
                lr_dev=lr_dev, inv_n=1.0 / 12288, kl_scale=1.0 / 24, w_sim=1.0 / 48, w_dis=1.0 / 40, beta=0.7, alpha=1.3, lr=2e-3,
                b1=0.9, b2=0.999)


# step: the optimiser step the launch prepares (step_dev holds step - 1 before it)
COMBINE_CASES = [cc(0, step=1), cc(1, step=2, lr_dev=5e-4), cc(2, step=1000), cc(3, step=10 ** 6, lr_dev=1e-3), cc(4), cc(5, step=7)]


def combine_data(c):
    g = gen_of(c["nparts"], c["kl_parts"], c["pair_parts"], 23)
    d = dict(c)
    d["sse_ws"] = torch.rand(c["nparts"], generator=g) * 30 if c["nparts"] else None
    d["recon"] = torch.rand(1, generator=g)
    d["kl"] = torch.rand(max(c["kl_parts"], 1), generator=g) * 5
    d["pair"] = torch.rand(2 * max(c["pair_parts"], 1), generator=g) * 3
    return d


def ac(n, mode, eps=1e-8, gscale=1.0, steps=1, t0=0, lr=1e-3):
    return dict(id=f"n{n}-{mode}-eps{eps}-gs{gscale}-steps{steps}-t{t0}", n=n, mode=mode, eps=eps, gscale=gscale, steps=steps, t0=t0,
                lr=lr, b1=0.9, b2=0.999)


# mode: how the step is stated ("step", "step_dev" + hyper_ws, "prepared" hyper_ws); t0: steps already taken
ADAM_CASES = [ac(1, "step", t0=3), ac(255, "step_dev", eps=1e-3, gscale=0.5, t0=6), ac(10007, "prepared", gscale=1.0 / 1024, t0=999),
              ac(2048 * 256 + 1, "step", eps=1e-3, gscale=0.5, t0=1), ac(10007, "step", steps=5), ac(255, "step_dev", steps=5, gscale=0.5),
              ac(10007, "prepared", steps=5, eps=1e-3, gscale=1.0 / 1024)]


def adam_data(n, gen, fresh):
    """w, m, v (zero moments when fresh) with the elements where sqrt(v') / bc2 ~ eps or below in front."""
    w = torch.randn(n, generator=gen)
    m = torch.zeros(n) if fresh else torch.randn(n, generator=gen) * 0.01
    v = torch.zeros(n) if fresh else torch.rand(n, generator=gen) * 1e-4
    if not fresh and n >= 8:
        v[:8] = torch.tensor([0.0, 1e-40, 1e-16, 1e-16, 0.0, 1e-6, 1e-40, 1e-30])
        m[:8] = torch.tensor([0.0, 0.0, 1e-9, -1e-9, 1e-12, 1e-3, 1e-20, 0.0])
    return w, m, v


def adam_grad(n, gen, step=0):
    g = torch.randn(n, generator=gen) * 10.0 ** float(torch.randint(-6, 1, (1,), generator=gen))
    if n >= 8:
        g[:8] = torch.tensor([0.0, 0.0, 1e-12, -1e-12, 1e-12, 1e-3, 0.0, 1e-20])
    return g


def perm_strides(dims, order):
    """Strides (per logical index) of the copy laid out in `order` (slowest first)."""
    s, acc = [0, 0, 0], 1
    for ax in reversed(order):
        s[ax] = acc
        acc *= dims[ax]
    return tuple(s)


def j6(id, dims, *copies):
    return job(id, 6, dims, copies=[(dt, perm_strides(dims, order)) for dt, order in copies])


BIG_A, BIG_B = (1031, 37, 29), (33, 1000, 33)                   # >= 2^20 elements, ragged against every tile shape

JOB_TABLES = {
    "small": [job("bias1", 7, (1, 1, 1)), job("bias1000", 7, (1000, 1, 1)), j6("one-f32", (5, 7, 3), (F32_T, (2, 1, 0))),
              j6("two-bf16-f32", (33, 20, 1), (BF16_T, (0, 1, 2)), (F32_T, (1, 0, 2))), j6("one-bf16", (64, 9, 16), (BF16_T, (2, 0, 1))),
              j6("two-f32-bf16", (7, 11, 13), (F32_T, (1, 2, 0)), (BF16_T, (2, 1, 0)))],
    "conv": [job("vec-f32", 3, (8, 8, 9), F32_T), job("vec-bf16", 3, (16, 16, 9), BF16_T), job("elem-f32", 3, (6, 5, 4), F32_T),
             job("elem-bf16", 3, (9, 20, 4), BF16_T), job("split-256", 3, (8, 256, 9), BF16_T), job("144x16", 3, (16, 144, 16), BF16_T),
             job("split-f32", 3, (4, 128, 9), F32_T)],
    "tiled-one": [j6("one", BIG_A, (BF16_T, (2, 1, 0)))],
    "tiled-same": [j6("same", BIG_B, (BF16_T, (0, 2, 1)), (F32_T, (2, 0, 1)))],
    "tiled-different": [j6("different", BIG_A, (BF16_T, (2, 1, 0)), (F32_T, (0, 2, 1)))],
    "tiled-mixed": [j6("mixed", BIG_B, (F32_T, (0, 1, 2)), (BF16_T, (1, 2, 0)))],
    "flat-big": [j6("both2", BIG_B, (BF16_T, (0, 1, 2)), (F32_T, (1, 0, 2))), job("bias7", 7, (7, 1, 1))],
}
JOB_GAP = 12                                                        # sentinel floats between the tensors of a table


def table_layout(jobs):
    """[(job, offset)] and the total length: tensors at 16-byte aligned offsets with JOB_GAP (or more) floats between."""
    out, off = [], JOB_GAP
    for j in jobs:
        out.append((j, off))
        off = ru4(off + job_numel(j) + JOB_GAP)
    return out, off


def table_data(name):
    jobs = JOB_TABLES[name]
    lay, total = table_layout(jobs)
    g = gen_of(len(name), total)
    w, gr = torch.randn(total, generator=g) * 0.1, torch.randn(total, generator=g) * 0.01
    m, v = torch.randn(total, generator=g) * 0.01, torch.rand(total, generator=g) * 1e-4
    return lay, total, w, gr, m, v


JOB_CONSTS = dict(b1=0.9, b2=0.999, eps=1e-8, gscale=0.5, lr=2e-3, step=7)


# ---- ambiguity of the random tables, coverage --------------------------------------------------------------------------------------

def table_ambiguity(K=100.0):
    """{case id: number of rows within K times their bound of a threshold} over every random case table, in float64 alone."""
    out = {}
    for c in PAIR_CASES:
        if not c["special"]:
            x1, x2 = pair_data(c)
            out["pair " + c["id"]] = int(pairdist_options(x1, x2, c["label"], c["margin"], c["eps"], 1.0, K=K)[2].sum())
    for c in COS_CASES:
        if not c["special"]:
            out["cos " + c["id"]] = int(Cos(*cos_data(c), c["eps"]).grad_options(c["label"], c["margin"], 1.0, K=K)[2].sum())
    for c in TRIPLET_CASES:
        if not c["special"]:
            out["triplet " + c["id"]] = int(Triplet(*triplet_data(c), c["margin"], c["eps"], c["swap"], K=K).ambiguous().sum())
    for c in TERM_CASES:
        if not c["special"]:
            h0, h1 = term_data(c)
            out["contrast " + c["id"]] = int(contrast_options(h0, h1, 1.0, None, K=K)[2].sum())
            out["triplet term " + c["id"]] = int(Triplet(*_term_rows(h0, h1), c["margin"], 1e-8, 1, K=K).ambiguous().sum())
    for c in KL_CASES:
        if c["logits"] != "edges":
            out["kl " + c["id"]] = int(kl_clamp_ambiguous(kl_data(c), c["eps"], c["clamp"], K=K).sum())
    return out


def branch_shares():
    """{case id: (share of active rows, share of inactive rows)} of the hinge in every random case with >= 4 rows / pairs."""
    out = {}
    for c in PAIR_CASES:
        if c["label"] and c["regime"] != "close" and not c["special"] and c["rows"] >= 4:
            act = Dist(*pair_data(c), c["eps"]).hinge(c["margin"])[4].double().mean()
            out["pair " + c["id"]] = (float(act), 1 - float(act))
    for c in TRIPLET_CASES:
        if c["regime"] != "close" and not c["special"] and c["rows"] >= 4:
            act = (Triplet(*triplet_data(c), c["margin"], c["eps"], c["swap"]).terms()[0] > 0).double().mean()
            out["triplet " + c["id"]] = (float(act), 1 - float(act))
    for c in TERM_CASES:
        if c["regime"] != "close" and not c["special"] and c["B"] * (c["T"] - 1) >= 4:
            h0, h1 = term_data(c)
            rows, nxt, valid = _next_rows(h0)
            act = Dist(rows[valid], nxt[valid], C_EPS).hinge(1.0)[4].double().mean()
            out["contrast " + c["id"]] = (float(act), 1 - float(act))
            act = (Triplet(*_term_rows(h0, h1), c["margin"], 1e-8, 1).terms()[0] > 0).double().mean()
            out["triplet term " + c["id"]] = (float(act), 1 - float(act))
    return out


# Which kernels an entry point launches, and which table exercises it in test_loss_bounds_gpu.py
ENTRY_KERNELS = {
    "rbvae_binarize_kl_fwd": ["binarize_kl_fwd_k"], "rbvae_binarize_kl_fwd_parts": ["binarize_kl_fwd_parts_k"],
    "rbvae_binarize_kl_bwd": ["binarize_kl_bwd_k"], "rbvae_kl_fwd": ["kl_fwd_k"], "rbvae_kl_bwd": ["kl_bwd_k"],
    "rbvae_pairdist_fwd": ["pairdist_fwd_k"], "rbvae_pairdist_bwd": ["pairdist_bwd_k"], "rbvae_paircos_fwd": ["paircos_fwd_k"],
    "rbvae_paircos_bwd": ["paircos_bwd_k"], "rbvae_contrast_term_fwd": ["contrast_term_fwd_k"],
    "rbvae_contrast_term_bwd": ["contrast_term_bwd_k"], "rbvae_contrast_term_fused": ["contrast_term_fused_k"],
    "rbvae_triplet_fwd": ["triplet_fwd_k"], "rbvae_triplet_bwd": ["triplet_bwd_k"], "rbvae_triplet_term_fwd": ["triplet_term_fwd_k"],
    "rbvae_triplet_term_bwd": ["triplet_term_bwd_k"], "rbvae_mse_fwd": ["mse_partial_k", "mse_final_k"], "rbvae_mse_bwd": ["mse_bwd_k"],
    "rbvae_combine_losses": ["combine_losses_k"], "rbvae_adam_step": ["adam_k"],
}
TABLE_ENTRIES = {
    "BIN_CASES": ["rbvae_binarize_kl_fwd", "rbvae_binarize_kl_fwd_parts", "rbvae_binarize_kl_bwd"],
    "KL_CASES": ["rbvae_kl_fwd", "rbvae_kl_bwd"], "PAIR_CASES": ["rbvae_pairdist_fwd", "rbvae_pairdist_bwd"],
    "COS_CASES": ["rbvae_paircos_fwd", "rbvae_paircos_bwd"],
    "TERM_CASES": ["rbvae_contrast_term_fwd", "rbvae_contrast_term_bwd", "rbvae_contrast_term_fused", "rbvae_triplet_term_fwd",
                   "rbvae_triplet_term_bwd"],
    "TRIPLET_CASES": ["rbvae_triplet_fwd", "rbvae_triplet_bwd"], "MSE_CASES": ["rbvae_mse_fwd", "rbvae_mse_bwd"],
    "COMBINE_CASES": ["rbvae_combine_losses"], "ADAM_CASES": ["rbvae_adam_step"],
}
LOSS_KERNELS = ["binarize_kl_fwd_k", "binarize_kl_fwd_parts_k", "binarize_kl_bwd_k", "kl_fwd_k", "kl_bwd_k", "pairdist_fwd_k",
                "pairdist_bwd_k", "paircos_fwd_k", "paircos_bwd_k", "contrast_term_fwd_k", "contrast_term_bwd_k",
                "contrast_term_fused_k", "triplet_fwd_k", "triplet_bwd_k", "triplet_term_fwd_k", "triplet_term_bwd_k",
                "mse_partial_k", "mse_final_k", "mse_bwd_k", "counter_add_k"]
JOB_BRANCHES = ["run_jobs_k[7]", "run_jobs_k[3,ctx,vec,f32]", "run_jobs_k[3,ctx,vec,bf16]", "run_jobs_k[3,ctx,elem,f32]",
                "run_jobs_k[3,ctx,elem,bf16]", "run_jobs_k[3,ctx,vec,bf16,split]", "run_jobs_k[3,ctx,vec,f32,split]",
                "run_jobs_k[6,flat,1]", "run_jobs_k[6,flat,2]", "run_jobs_k[6,tiled,one]", "run_jobs_k[6,tiled,same]",
                "run_jobs_k[6,tiled,different]", "run_jobs_k[6,tiled,mixed]"]
REACHABLE = set(LOSS_KERNELS) | {"combine_losses_k", "combine_losses_k[hyper]", "adam_k", "adam_hyper_k"} | set(JOB_BRANCHES)


def covered_instances():
    """Every kernel (and branch of run_jobs_k) the case tables launch."""
    got = set()
    tables = globals()
    for tab, entries in TABLE_ENTRIES.items():
        if tables[tab]:
            for e in entries:
                got |= set(ENTRY_KERNELS[e])
    if any(c["step"] is not None for c in COMBINE_CASES):
        got.add("combine_losses_k[hyper]")
    if any(c["mode"] == "step_dev" for c in ADAM_CASES):
        got.add("adam_hyper_k")
    if any(c["seed_dev"] is not None for c in BIN_CASES):
        got.add("counter_add_k")                                   # the device seed is advanced with rbvae_counter_add
    for jobs in JOB_TABLES.values():
        got |= {job_kernel(j) for j in jobs}
    return got
