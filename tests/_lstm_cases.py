"""References, error model and case tables for the LSTM kernel bounds tests (csrc/lstm.hip).  Plain Python and torch
float64 on the CPU: importing this module needs no GPU.

Restated dispatch
    fwd_dispatch / bwd_dispatch / pair_fwd_dispatch / pair_bwd_dispatch / wgrad_dispatch name the kernel instance an
    entry point launches for a shape, or ("refused", reason).  They restate lstm_fwd_impl, lstm_bwd_impl,
    rbvae_lstm_pair_fwd(_ok), rbvae_lstm_pair_bwd(_ok) and launch_lstm_wgrad.  The case tables below are built from them
    (the T where a dispatcher changes kernel is computed by first_change, never typed in), and REACHABLE lists every
    instance the tables have to reach.

Error model: every stored cell against its own stored neighbours
    An LSTM is a recurrence, so an end-to-end element-wise bound is either useless or loose.  But the kernels store
    everything a cell reads: each stored value is recomputed in float64 from the values THE KERNEL stored one step
    upstream, and its bound holds the rounding of that one step only.  u = 2^-24 throughout.

    fast_sigmoid(x) = v_rcp_f32(1 + v_exp_f32(-log2e * x)) (the wavefront, big, pair and unit kernels):
        the f32 constant and the product put 2u|a| into the exponent a = -log2e x, i.e. a relative 2 ln2 |a| u = 2|x|u
        into e = 2^a; v_exp_f32 is 1 ulp (2u relative); so e carries (2|x| + 2)u.  1 + e rounds once (u) and v_rcp_f32
        is 1 ulp (2u).  s = 1/(1+e) has ds/s = -(1 - s) de/e, hence
            c_sig(x) = s(1-s)(2|x| + 2)u + 3u s            (<= 3.95u: x s(1-s) <= 0.224)
        Overflow: e = inf gives 1 + inf = inf and rcp(inf) = 0 where the true value is < 2^-126; e flushed to 0 gives
        exactly 1: both inside TINY_F32.  (1 ulp for v_exp_f32 / v_rcp_f32 is the figure of the CDNA ISA manual and of
        the kernels' own comment; it is taken as given, not measured.)
    fast_tanh(x) = 2 r - 1 with r = fast_sigmoid(2x): r carries r(1-r)(4|x| + 2)u + 3u r with r(1-r) = (1-t^2)/4; the
        doubling is exact and the subtraction rounds once (u|t|; one rounding also when contracted into an fma):
            c_tanh(x) = (1-t^2)(2|x| + 1)u + 6u r + u|t|   (<= 8.9u: x(1-t^2) <= 0.448)
    lstm_fwd_k<32> / lstm_bwd_k<32> and the binarisation use the device library: 1/(1 + expf(-x)) with expf at 1 ulp (2u
        relative in e), one rounding in 1 + e and a correctly rounded division (u):  c_sig_lib = 2u s(1-s) + 2u s;
        tanhf at 2 ulp: c_tanh_lib = 4u|t|; logf at 1 ulp.  These are the accuracies the HIP device-library documentation
        states for expf / tanhf / logf; they are an ASSUMPTION of this model (the document is not part of the tree).

    Gates:   pre_ref = W_ih x + W_hh h + b_ih + b_hh from the stored hs[l] / hprev[l],  S_pre the same on absolute values,
             d_pre = c_acc(2L) S_pre (the project's accumulation constant, tests/_bounds.py);
             |acts - act(pre_ref)| <= act'(pre_ref) d_pre + max|act''|/2 d_pre^2 + c_act(pre_ref)
             (max|sigmoid''|/2 < 0.05, max|tanh''|/2 < 0.39).
    Cell:    cs == fma(f, c_prev, i g) of the stored acts and the stored cs[t-1]: two roundings, u(|i g| + |c|);
             lstm_fwd_k<32> writes fg * c + ig * gg with no explicit fma: one rounding more, + u|f c_prev|.
    Output:  hs[l+1] == o tanh(cs) of the stored values within o c_tanh(c) + u|h|.
    Structure, bit for bit: hprev[l][s][t] == hs[l+1][s][t-1] (zero at t = 0); hs[0] == the input (the slab sum in slab
             order); the cast copy == round-to-nearest-even of the top layer, zero padding; hard codes == (y > 0.5).

    Backward (acts, cs, weights, g_top are INPUTS; dG, dx, dz outputs):
        dx == W_ih[0]^T dG[0] of the kernel's own dG within c_acc(4L) S.
        dh_ref(l, t) = (top: g_top_ref, else W_ih[l+1]^T dG[l+1][t]) + W_hh[l]^T dG[l][t+1], all from the kernel's own dG,
        E_dh = c_acc(8L) S_dh (+ the bound of g_top_ref).  Only the scalar chain dc(t) = f(t+1) dc(t+1) + dh o (1-tc^2)
        is propagated, in float64, with the running bound
            E_dc(t) = f(t+1) E_dc(t+1) + u|f(t+1) dc(t+1)| + o(1-tc^2) E_dh
                      + |dh o| (2|tc| c_tanh + c_tanh^2 + 2u) + 3u|dh o (1-tc^2)| + u|dc|
        (the product dc f; the absolute error u of 1 - tc tc plus that of the recomputed tc; the products and the sum).
        Gate gradients, 4 roundings of their own products each (5u allowed):
            d_o: E_dh |tc o(1-o)| + |dh o(1-o)| c_tanh + 5u|d_o|        d_i: E_dc |g i(1-i)| + 5u|d_i|
            d_f: E_dc |c_prev f(1-f)| + 5u|d_f|                        d_g: E_dc |i(1-g^2)| + u|dc i| + 5u|d_g|
    Weight gradient: gblk == dG^T [hs | hprev | 1] of the tensors handed to the kernel within (c_acc(S T) + 4u) S (the
        four-wave merge), + u|result| with accumulate = 1.
"""
import math

import torch

from _bounds import c_acc, colsum_bound

U = 2.0 ** -24
TINY_F32 = 2.0 ** -120
LDS_BYTES = 64 * 1024
LOG2E_F32 = 1.4426950216293335          # float(1.4426950408889634f)
LOG2E2_F32 = 2.885390043258667          # float(2.8853900817779268f)


def ru(a, b):
    return (a + b - 1) // b * b


# ---- restated dispatch ---------------------------------------------------------------------------------------------

BIG_NCH = (10, 13, 16, 19, 22, 25, 28, 32)


def _big(L):
    nch = (L + 3) // 4
    return next(n for n in BIG_NCH if nch <= n)


def fwd_wave_ok(T, L, layers):
    wlds = ((layers + 1) * T * L + layers * 4 * L) * 4
    return L <= 32 and layers * ru(4 * L, 64) <= 1024 and wlds <= LDS_BYTES


def bwd_wave_ok(T, L, layers):
    wlds = (T * L + layers * T * 5 * L + layers * 12 * L) * 4
    return L <= 32 and layers * ru(4 * L, 64) <= 1024 and wlds <= LDS_BYTES


def fwd_dispatch(T, L, layers, in_parts=False, cast=False, S=1, use_wT=False):
    """lstm_fwd_impl (rbvae_lstm_fwd: in_parts = cast = False; rbvae_lstm_fwd_ex)."""
    if L > 128:
        return ("refused", "latent_dim > 128")
    if (2 * T * L + 5 * L) * 4 > LDS_BYTES:
        return ("refused", "T*L too large")
    if fwd_wave_ok(T, L, layers):
        if L == 32:
            return "lstm_fwd_wave_k<32,true,true>"
        return "lstm_fwd_wave_k<32,true,false>" if L % 4 == 0 else "lstm_fwd_wave_k<32,false,false>"
    if in_parts or cast:
        return ("refused", "only the wavefront kernel sums slabs / casts")
    if L > 32:
        RP = ru(4 * L, 64)
        if ((2 * T + 1) * 128 + RP + T * RP) * 4 > LDS_BYTES:
            return ("refused", "T too long")
        return f"lstm_fwd_big_k<{_big(L)}>"
    return "lstm_fwd_k<32>"


def bwd_dispatch(T, L, layers, nparts=1, cast=False, dx_colsum=False, bin=False, S=1, use_wT=False):
    """lstm_bwd_impl (rbvae_lstm_bwd, rbvae_lstm_bwd_ex, rbvae_lstm_bwd_bin)."""
    if L > 128:
        return ("refused", "latent_dim > 128")
    if (2 * T * L + 13 * L) * 4 > LDS_BYTES:
        return ("refused", "T*L too large")
    if bwd_wave_ok(T, L, layers):
        return "lstm_bwd_wave_k<32,true>" if L == 32 else "lstm_bwd_wave_k<32,false>"
    if nparts != 1 or cast or dx_colsum or bin:
        return ("refused", "only the wavefront kernel sums slabs / casts / binarises")
    if L > 32:
        if ((2 * T + 1) * 128 + T * 4 * 132) * 4 > LDS_BYTES:
            return ("refused", "T too long")
        return f"lstm_bwd_big_k<{_big(L)}>"
    return "lstm_bwd_k<32>"


def pair_fwd_ok(T, L, layers):
    LS = (L + 3) & ~3
    lds = (2 * (layers + 1) * T * LS + 2 * layers * 4 * L + T * LS + 16) * 4
    return L <= 32 and 2 * layers * ru(4 * L, 64) <= 1024 and lds <= LDS_BYTES


def pair_fwd_dispatch(T, L, layers, unit_threads=1):
    """rbvae_lstm_pair_fwd; unit_threads: the rbvae_dbg_lstm_unit_threads switch (1 = shipped)."""
    if not pair_fwd_ok(T, L, layers):
        return ("refused", "outside rbvae_lstm_pair_fwd_ok")
    if L == 32 and 2 * layers * 64 <= 512 and unit_threads:
        return "lstm_pair_fwd_unit_k"
    if L == 32:
        return "lstm_pair_fwd_k<32,true>"
    return "lstm_pair_fwd_k<32,false,28>" if ((L + 3) & ~3) == 28 else "lstm_pair_fwd_k<32,false>"


def pair_bwd_ok(T, L, layers):
    lds = (5 * T * L + 2 * layers * (T * 5 * L + 12 * L)) * 4
    return L <= 32 and 2 * layers * ru(4 * L, 64) <= 1024 and lds <= LDS_BYTES


def pair_bwd_dispatch(T, L, layers, unit_threads=1):
    if not pair_bwd_ok(T, L, layers):
        return ("refused", "outside rbvae_lstm_pair_bwd_ok")
    if L == 32 and 2 * layers * 64 <= 512 and unit_threads:
        return "lstm_pair_bwd_unit_k"
    return "lstm_pair_bwd_k<32,true>" if L == 32 else "lstm_pair_bwd_k<32,false>"


def wgrad_dispatch(pair=False, accumulate=0):
    """launch_lstm_wgrad: one kernel, launched over one stack or a pair of stacks."""
    return f"lstm_wgrad_mfma_k[{'pair' if pair else 'single'},accumulate={int(bool(accumulate))}]"


REACHABLE = (
    ["lstm_fwd_wave_k<32,true,true>", "lstm_fwd_wave_k<32,true,false>", "lstm_fwd_wave_k<32,false,false>", "lstm_fwd_k<32>"]
    + [f"lstm_fwd_big_k<{n}>" for n in BIG_NCH]
    + ["lstm_bwd_wave_k<32,true>", "lstm_bwd_wave_k<32,false>", "lstm_bwd_k<32>"]
    + [f"lstm_bwd_big_k<{n}>" for n in BIG_NCH]
    + ["lstm_pair_fwd_unit_k", "lstm_pair_fwd_k<32,true>", "lstm_pair_fwd_k<32,false,28>", "lstm_pair_fwd_k<32,false>"]
    + ["lstm_pair_bwd_unit_k", "lstm_pair_bwd_k<32,true>", "lstm_pair_bwd_k<32,false>"]
    + [wgrad_dispatch(p, a) for p in (False, True) for a in (0, 1)])


def first_change(fn, Tmax=4096):
    """(T, fn(T)) at the first T >= 2 where fn(T) differs from fn(1); (None, fn(1)) if it never does."""
    base = fn(1)
    for T in range(2, Tmax + 1):
        if fn(T) != base:
            return T, fn(T)
    return None, base


def first_changes(L, layers):
    """The first T at which each entry point changes kernel or refuses."""
    return {
        "rbvae_lstm_fwd": first_change(lambda T: fwd_dispatch(T, L, layers)),
        "rbvae_lstm_fwd_ex": first_change(lambda T: fwd_dispatch(T, L, layers, in_parts=True, cast=True)),
        "rbvae_lstm_bwd": first_change(lambda T: bwd_dispatch(T, L, layers)),
        "rbvae_lstm_bwd_ex": first_change(lambda T: bwd_dispatch(T, L, layers, nparts=2, cast=True, dx_colsum=True)),
        "rbvae_lstm_bwd_bin": first_change(lambda T: bwd_dispatch(T, L, layers, bin=True)),
        "rbvae_lstm_pair_fwd": first_change(lambda T: pair_fwd_dispatch(T, L, layers)),
        "rbvae_lstm_pair_bwd": first_change(lambda T: pair_bwd_dispatch(T, L, layers)),
    }


def is_lib_kernel(name):
    """The layer-sequential fall-backs use expf / tanhf; every other kernel fast_sigmoid / fast_tanh."""
    return name in ("lstm_fwd_k<32>", "lstm_bwd_k<32>")


# ---- activation error model ----------------------------------------------------------------------------------------

def c_sig(x, lib=False):
    s = torch.sigmoid(x)
    if lib:
        return 2 * U * s * (1 - s) + 2 * U * s + TINY_F32
    return s * (1 - s) * (2 * x.abs() + 2) * U + 3 * U * s + TINY_F32


def c_tanh(x, lib=False):
    t = torch.tanh(x)
    if lib:
        return 4 * U * t.abs() + TINY_F32
    r = torch.sigmoid(2 * x)
    return (1 - t * t) * (2 * x.abs() + 1) * U + 6 * U * r + U * t.abs() + TINY_F32


# ---- data ----------------------------------------------------------------------------------------------------------

def layer_floats(L):
    return 8 * L * L + 8 * L


def split_w(wblk, L, layers):
    """[(W_ih [4L][L], W_hh [4L][L], b_ih [4L], b_hh [4L])] views of a flat weight block."""
    out = []
    for l in range(layers):
        b = wblk[l * layer_floats(L):(l + 1) * layer_floats(L)]
        out.append((b[:4 * L * L].view(4 * L, L), b[4 * L * L:8 * L * L].view(4 * L, L), b[8 * L * L:8 * L * L + 4 * L],
                    b[8 * L * L + 4 * L:]))
    return out


def make_wT(wblk, L, layers):
    """[layers][ih | hh][L][4L] transposed copies."""
    return torch.stack([torch.stack([wi.t().contiguous(), wh.t().contiguous()]) for wi, wh, _, _ in split_w(wblk, L, layers)])


REGIMES = ("small", "wide", "saturated")


def make_weights(L, layers, regime, gen):
    """small: U(-1,1)/sqrt(L), the suite's present weights.  wide: scaled so that pre-activations spread over about
    +-10 (gates near 0 and 1, 1 - tc^2 small).  saturated: small weights with a handful of bias entries at +-100, where
    exp2 overflows to inf or flushes to zero."""
    w = (torch.rand(layers * layer_floats(L), generator=gen) * 2 - 1) / L ** 0.5
    if regime == "wide":
        w = w * 8.0
    elif regime == "saturated":
        for l, (_, _, bi, bh) in enumerate(split_w(w, L, layers)):
            for q in range(min(6, 4 * L)):
                j = (q * 2654435761 + l * 97) % (4 * L)
                (bi if q % 2 else bh)[j] = 100.0 if (q // 2) % 2 else -100.0
    else:
        assert regime == "small", regime
    return w.float().contiguous()


# ---- forward: reference pass / f32 emulation (with injectable defects), and the checks -------------------------------

def _sig32(x):
    """fast_sigmoid in torch f32: exp2 and the reciprocal round as separate f32 operations."""
    return 1.0 / (1.0 + torch.exp2(-torch.tensor(LOG2E_F32, dtype=torch.float32) * x))


def _tanh32(x):
    return 2.0 * (1.0 / (1.0 + torch.exp2(-torch.tensor(LOG2E2_F32, dtype=torch.float32) * x))) - 1.0


def forward_pass(wblk, x, L, layers, f32=False, defect=None):
    """The stack in float64 (results rounded to f32 where stored), or with f32=True an f32 emulation of the wavefront
    kernel's cell (f32 dot products, exp2 / rcp activations, the fused multiply-add of the cell state).  x [S][T][L].
    Returns f32 hs_all [layers+1][S][T][L], hprev, acts [layers][S][T][4L], cs.  defect: one of the single faults of
    tests/test_lstm_bounds_cpu.py."""
    S, T, _ = x.shape
    dt = torch.float32 if f32 else torch.float64
    sig, tanh = (_sig32, _tanh32) if f32 else (torch.sigmoid, torch.tanh)
    hs = torch.zeros(layers + 1, S, T, L)
    hp, cs, acts = torch.zeros(layers, S, T, L), torch.zeros(layers, S, T, L), torch.zeros(layers, S, T, 4 * L)
    hs[0] = x.float()
    c = torch.zeros(S, L, dtype=dt)
    clean = forward_pass(wblk, x, L, layers, f32)[0] if defect == "h_from_prev_seq" else None
    for l, (wi, wh, bi, bh) in enumerate(split_w(wblk, L, layers)):
        wi, wh, bi, bh = wi.to(dt), wh.to(dt), bi.to(dt), bh.clone().to(dt)
        if defect == "drop_bhh" and l == layers - 1:
            bh[L + 1 if L > 1 else 0] = 0
        wi_d = wi
        if defect == "skip_last_k" and l == 0:
            wi_d = wi.clone()
            wi_d[2 * L, L - 1] = 0
        h = torch.zeros(S, L, dtype=dt)
        if defect != "c_not_reset":
            c = torch.zeros(S, L, dtype=dt)
        for t in range(T):
            if t == 0 and defect == "h_from_prev_seq":
                h = torch.cat([torch.zeros(1, L, dtype=dt), clean[l + 1][:-1, T - 1].to(dt)])
            xin = hs[l][:, t].to(dt)
            pre = xin @ wi_d.t() + h @ wh.t() + (bi + bh)
            i, f, o = sig(pre[:, :L]), sig(pre[:, L:2 * L]), sig(pre[:, 3 * L:])
            g = sig(pre[:, 2 * L:3 * L]) if (defect == "sigmoid_g" and l == 0) else tanh(pre[:, 2 * L:3 * L])
            a = torch.cat([i, f, g, o], 1).float()             # as stored
            i, f, g, o = (a[:, k * L:(k + 1) * L] for k in range(4))
            if f32:
                c = (f.double() * c.double() + (i * g).double()).float()        # fmaf(f, c, i * g)
                hn = o * tanh(c)
            else:
                c = (f.double() * c + i.double() * g.double()).float().double()
                hn = (o.double() * torch.tanh(c)).float().double()
            acts[l][:, t] = torch.cat([i, f, o, g], 1) if (defect == "gate_order" and l == 0) else a
            cs[l][:, t], hp[l][:, t], hs[l + 1][:, t] = c.float(), h.float(), hn.float()
            h = hn.to(dt)
    return hs, hp, acts, cs


def _worst(err, bnd, what, dims):
    """Assert err <= bnd element-wise (NaN fails); returns the worst ratio.  dims names the axes for the message."""
    ratio = torch.where(torch.isnan(err) | torch.isnan(bnd), torch.full_like(err, float("inf")), err / bnd)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    bad = ~(err <= bnd)
    if bool(bad.any()):
        flat = int(torch.argmax(ratio.reshape(-1)))
        idx = []
        for n in reversed(err.shape):
            idx.append(flat % n)
            flat //= n
        where = ", ".join(f"{d} {i}" for d, i in zip(dims, reversed(idx)))
        k = tuple(reversed(idx))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound; worst |err|/bound = "
                             f"{worst:.3g} at ({where}): |err| {float(err[k]):.3g}, bound {float(bnd[k]):.3g}")
    return worst


def _exact(got, ref, what, dims):
    """Bit for bit (f32 / bf16 payloads compared as integers, so NaN patterns count too)."""
    it = torch.int16 if got.dtype == torch.bfloat16 else torch.int32
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    bad = got.contiguous().view(it) != ref.contiguous().view(it)
    if bool(bad.any()):
        k = tuple(int(v) for v in bad.nonzero()[0])
        where = ", ".join(f"{d} {i}" for d, i in zip(dims, k))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ bit for bit; first at ({where}): "
                             f"got {float(got[k])!r}, want {float(ref[k])!r}")
    return 0.0


def check_forward(wblk, hs, hprev, acts, cs, L, layers, lib=False, what="lstm fwd"):
    """Every stored cell of a forward pass against its stored neighbours (module docstring).  All tensors f32 on the
    CPU.  Returns {"hprev": 0, "gates": r, "cell": r, "h": r} (worst |err| / bound per check)."""
    S, T = hs.shape[1], hs.shape[2]
    out = {}
    want_hp = torch.zeros_like(hprev)
    want_hp[:, :, 1:] = hs[1:, :, :-1]
    out["hprev"] = _exact(hprev, want_hp, f"{what}: hprev == hs[l+1][t-1]", ("layer", "sequence", "time", "unit"))
    d = torch.float64
    g_r, c_r, h_r = 0.0, 0.0, 0.0
    for l, (wi, wh, bi, bh) in enumerate(split_w(wblk.double(), L, layers)):
        x, h = hs[l].to(d), hprev[l].to(d)
        pre = x @ wi.t() + h @ wh.t() + bi + bh
        S_pre = x.abs() @ wi.abs().t() + h.abs() @ wh.abs().t() + bi.abs() + bh.abs()
        d_pre = c_acc(2 * L) * S_pre
        is_g = torch.zeros(4 * L, dtype=torch.bool)
        is_g[2 * L:3 * L] = True
        sg, th = torch.sigmoid(pre), torch.tanh(pre)
        ref = torch.where(is_g, th, sg)
        slope = torch.where(is_g, 1 - th * th, sg * (1 - sg))
        curv = torch.where(is_g, torch.tensor(0.39, dtype=d), torch.tensor(0.05, dtype=d))
        c_act = torch.where(is_g, c_tanh(pre, lib), c_sig(pre, lib))
        a = acts[l].to(d)
        g_r = max(g_r, _worst((a - ref).abs(), slope * d_pre + curv * d_pre * d_pre + c_act,
                              f"{what}: gates of layer {l}", ("sequence", "time", "gate row")))
        i, f, g, o = (a[..., k * L:(k + 1) * L] for k in range(4))
        c = cs[l].to(d)
        cp = torch.zeros_like(c)
        cp[:, 1:] = c[:, :-1]
        cref = f * cp + i * g
        bc = U * ((i * g).abs() + cref.abs()) + (U * (f * cp).abs() if lib else 0.0) + TINY_F32
        c_r = max(c_r, _worst((c - cref).abs(), bc, f"{what}: cell state of layer {l}", ("sequence", "time", "unit")))
        href = o * torch.tanh(c)
        bh_ = o * c_tanh(c, lib) + U * href.abs() + TINY_F32
        h_r = max(h_r, _worst((hs[l + 1].to(d) - href).abs(), bh_, f"{what}: output of layer {l}", ("sequence", "time", "unit")))
    out.update(gates=g_r, cell=c_r, h=h_r)
    return out


def slab_sum_fwd(parts):
    """The forward kernels' slab sum, exactly: v = p0; v += p1; ... in slab order, in f32."""
    v = parts[0].clone()
    for q in range(1, parts.shape[0]):
        v = v + parts[q]
    return v


def slab_sum_bwd(parts):
    """lstm_bwd_wave_k's order: groups of three ((g + a) + b) + c, then the tail one by one -- the same left-to-right
    f32 sum, restated as the kernel writes it."""
    gt, q, n = parts[0].clone(), 1, parts.shape[0]
    while q + 3 <= n:
        gt = ((gt + parts[q]) + parts[q + 1]) + parts[q + 2]
        q += 3
    while q < n:
        gt = gt + parts[q]
        q += 1
    return gt


def check_cast(cast, src, L, what="cast"):
    """cast [rows][ld] (f32 or bf16) == round-to-nearest-even of src [rows][L], padding columns exactly zero."""
    want = torch.zeros_like(cast)
    want[:, :L] = src.reshape(-1, L).to(cast.dtype)           # torch rounds to nearest even
    return _exact(cast, want, what, ("row", "column"))


def check_colsum(sums, dx, what="dx_colsum"):
    """sums [S][L] == sum over t of the kernel's own dx [S][T][L] within the recursive-summation bound."""
    d = dx.double()
    ref = d.sum(1)
    bnd = torch.stack([colsum_bound(d[s]) for s in range(d.shape[0])]) + U * ref.abs()
    return _worst((sums.double() - ref).abs(), bnd, what, ("sequence", "unit"))


# ---- the binarisation around the stacks ------------------------------------------------------------------------------

def check_binarize(hs_top, Un, y, z, tau, ratio, neps, hard, what="pair fwd"):
    """y_soft against sigmoid((h + ratio (log(U + e) - log(1 - U + e))) / tau) from the stored top-layer h (library expf /
    logf: c_sig_lib, logf at 1 ulp, each f32 operation one rounding), and the codes: hard z == (y > 0.5) of the kernel's
    own y bit for bit, soft z == y."""
    d = torch.float64
    h, u = hs_top.reshape(y.shape).to(d), Un.reshape(y.shape).to(d)
    tau = float(torch.tensor(tau, dtype=torch.float32))
    ratio, neps = float(torch.tensor(ratio, dtype=torch.float32)), float(torch.tensor(neps, dtype=torch.float32))
    a, b = u + neps, 1.0 - u + neps
    la, lb = torch.log(a), torch.log(b)
    n = ratio * (la - lb)
    E_n = abs(ratio) * ((2 * U * la.abs() + U) + (2 * U * lb.abs() + 2 * U / b) + U * (la - lb).abs()) + U * n.abs()
    arg = (h + n) / tau
    E_arg = (E_n + U * (h + n).abs()) / tau + U * arg.abs()
    yr = torch.sigmoid(arg)
    r = _worst((y.to(d) - yr).abs(), yr * (1 - yr) * E_arg + c_sig(arg, lib=True), f"{what}: y_soft", ("row", "unit"))
    _exact(z, (y > 0.5).float() if hard else y, f"{what}: codes", ("row", "unit"))
    return r


def kl_elem64(v, p, eps, clamp):
    q = torch.sigmoid(v)
    if clamp:
        q = q.clamp(eps, 1 - eps)
    return q * (torch.log(q + eps) - math.log(p)) + (1 - q) * (torch.log(1 - q + eps) - math.log(1 - p))


def check_kl_parts(kl_parts, z, S, p, eps, clamp, what="pair fwd"):
    """kl_parts[s] against the float64 sum of kl_elem over the stored codes of sequence s: colsum_bound plus the
    per-element term (sigmoid, two logf, six f32 operations: 12u of the absolute terms)."""
    d = torch.float64
    p = float(torch.tensor(p, dtype=torch.float32))
    v = z.reshape(S, -1).to(d)
    e = kl_elem64(v, p, eps, clamp)
    q = torch.sigmoid(v)
    per = 12 * U * (q * (torch.log(q + eps).abs() + abs(math.log(p))) + (1 - q) * (torch.log(1 - q + eps).abs() + abs(math.log(1 - p))))
    bnd = torch.stack([colsum_bound(e[s].reshape(-1, 1))[0] for s in range(S)]) + per.sum(1)
    return _worst((kl_parts.to(d) - e.sum(1)).abs(), bnd, f"{what}: kl_parts", ("sequence",))


def kl_grad64(v, p, eps, clamp):
    """(kl_elem_grad in float64, its f32 error bound): the clamp rule of csrc/common.h; sigmoid at c_sig_lib, logf at
    1 ulp, the arguments q + eps / 1 - q + eps carry the sigmoid's error."""
    s = torch.sigmoid(v)
    q = s.clamp(eps, 1 - eps) if clamp else s
    omq = 1 - q
    lp, l1p = math.log(p), math.log(1 - p)
    terms = [torch.log(q + eps) - lp, q / (q + eps), torch.log(omq + eps) - l1p, omq / (omq + eps)]
    dq = terms[0] + terms[1] - terms[2] - terms[3]
    E_dq = 3.5 * U * (1 / (q + eps) + 1 / (omq + eps)) + 12 * U * (torch.log(q + eps).abs() + abs(lp) + torch.log(omq + eps).abs()
                                                                 + abs(l1p) + 2)
    gr = dq * s * (1 - s)
    E = E_dq * s * (1 - s) + dq.abs() * (3.5 * U + 3 * U * s * (1 - s))
    if clamp:
        ok = (s >= eps) & (s <= 1 - eps)
        gr, E = torch.where(ok, gr, torch.zeros_like(gr)), torch.where(ok, E, torch.zeros_like(E))
    return gr, E


def gtop_bin(gz, E_gz, y, z, g_hs, tau, kl_weight, N, p, eps, clamp):
    """(g_top_ref, bound) of the fused binarise backward: g_hs + (gz + klw dKL/dz(z)) y (1 - y) / tau, klw the f32
    kl_weight / (float)N.  gz float64 with its own bound E_gz; five f32 operations on the product."""
    d = torch.float64
    tau = float(torch.tensor(tau, dtype=torch.float32))
    klw = float(torch.tensor(kl_weight, dtype=torch.float32) / torch.tensor(float(N), dtype=torch.float32))
    p = float(torch.tensor(p, dtype=torch.float32))
    y, z = y.to(d), z.to(d)
    gg, E_gg = gz, E_gz
    if klw != 0.0:
        kg, E_kg = kl_grad64(z, p, eps, clamp)
        gg = gz + klw * kg
        E_gg = E_gz + abs(klw) * E_kg + 2 * U * (gz.abs() + (klw * kg).abs())
    fac = y * (1 - y) / tau
    prod = gg * fac
    hsv = g_hs.to(d) if g_hs is not None else torch.zeros_like(prod)
    ref = hsv + prod
    return ref, E_gg * fac.abs() + 5 * U * prod.abs() + U * ref.abs() + TINY_F32


# ---- backward ------------------------------------------------------------------------------------------------------

def backward_pass(wblk, acts, cs, g_top, L, layers, f32=False, defect=None):
    """BPTT of the stack from the saved gates / cell states in float64 (stored values rounded to f32), or with f32=True in
    f32 arithmetic with the recomputed exp2 / rcp tanh.  Returns f32 dG [layers][S][T][4L], dx [S][T][L]."""
    S, T, _ = g_top.shape
    dt = torch.float32 if f32 else torch.float64
    tanh = _tanh32 if f32 else torch.tanh
    dG = torch.zeros(layers, S, T, 4 * L)
    dh_above = g_top.to(dt)
    ws = split_w(wblk, L, layers)
    for l in range(layers - 1, -1, -1):
        wi, wh = ws[l][0].to(dt), ws[l][1].to(dt)
        a, c = acts[l].to(dt), cs[l].to(dt)
        dcn, dhrec = torch.zeros(S, L, dtype=dt), torch.zeros(S, L, dtype=dt)
        for t in range(T - 1, -1, -1):
            i, f, g, o = (a[:, t, k * L:(k + 1) * L] for k in range(4))
            cp = c[:, t - 1] if t > 0 else (c[:, 0] if defect == "cprev_t0" else torch.zeros(S, L, dtype=dt))
            tc = tanh(c[:, t])
            dh = dh_above[:, t] + dhrec
            dc = dcn + dh * o * (1 - tc * tc)
            row = torch.cat([dc * g * i * (1 - i), dc * cp * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)], 1).float()
            dG[l][:, t] = row
            dcn = dc if defect == "dc_no_f" else dc * f
            dhrec = row.to(dt) @ wh
        dh_above = (dG[l].to(dt) @ wi).float().to(dt)
    dx = dh_above.float()
    if defect == "dx_swap" and T > 1:
        dx[0, [0, 1]] = dx[0, [1, 0]]
    return dG, dx


def check_backward(wblk, acts, cs, gtop_ref, E_gtop, dG, dx, L, layers, lib=False, what="lstm bwd"):
    """Every gate gradient and input-gradient row of a backward pass against the kernel's own dG one step upstream (module
    docstring).  gtop_ref float64 [S][T][L] with its bound E_gtop (0 for a plain or exactly summed g_top).  Returns
    {"dG": r, "dx": r}."""
    d = torch.float64
    S, T = dG.shape[1], dG.shape[2]
    ws = split_w(wblk.double(), L, layers)
    dGd = dG.to(d)
    g_r = 0.0
    for l in range(layers - 1, -1, -1):
        wi, wh = ws[l][0], ws[l][1]
        if l == layers - 1:
            up, S_up, E_up = gtop_ref.to(d), gtop_ref.to(d).abs(), E_gtop
        else:
            up, S_up, E_up = dGd[l + 1] @ ws[l + 1][0], dGd[l + 1].abs() @ ws[l + 1][0].abs(), 0.0
        rec, S_rec = torch.zeros(S, T, L, dtype=d), torch.zeros(S, T, L, dtype=d)
        rec[:, :-1], S_rec[:, :-1] = dGd[l][:, 1:] @ wh, dGd[l][:, 1:].abs() @ wh.abs()
        dh = up + rec
        E_dh = c_acc(8 * L) * (S_up + S_rec) + E_up
        a, c = acts[l].to(d), cs[l].to(d)
        i, f, g, o = (a[..., k * L:(k + 1) * L] for k in range(4))
        cp = torch.zeros_like(c)
        cp[:, 1:] = c[:, :-1]
        tc, ct = torch.tanh(c), c_tanh(c, lib)
        dc, E_dc = torch.zeros(S, T, L, dtype=d), torch.zeros(S, T, L, dtype=d)
        dcn, E_n = torch.zeros(S, L, dtype=d), torch.zeros(S, L, dtype=d)
        for t in range(T - 1, -1, -1):
            dho = dh[:, t] * o[:, t]
            om = 1 - tc[:, t] * tc[:, t]
            dc[:, t] = dcn + dho * om
            E_dc[:, t] = (E_n + o[:, t] * om * E_dh[:, t] + dho.abs() * (2 * tc[:, t].abs() * ct[:, t] + ct[:, t] ** 2 + 2 * U)
                          + 3 * U * (dho * om).abs() + U * dc[:, t].abs())
            dcn = dc[:, t] * f[:, t]
            E_n = f[:, t] * E_dc[:, t] + U * dcn.abs()
        d_i, d_f = dc * g * i * (1 - i), dc * cp * f * (1 - f)
        d_g, d_o = dc * i * (1 - g * g), dh * tc * o * (1 - o)
        ref = torch.cat([d_i, d_f, d_g, d_o], -1)
        bnd = torch.cat([E_dc * (g * i * (1 - i)).abs() + 5 * U * d_i.abs(),
                         E_dc * (cp * f * (1 - f)).abs() + 5 * U * d_f.abs(),
                         E_dc * (i * (1 - g * g)).abs() + U * (dc * i).abs() + 5 * U * d_g.abs(),
                         E_dh * (tc * o * (1 - o)).abs() + (dh * o * (1 - o)).abs() * ct + 5 * U * d_o.abs()], -1) + TINY_F32
        g_r = max(g_r, _worst((dGd[l] - ref).abs(), bnd, f"{what}: dG of layer {l}", ("sequence", "time", "gate row")))
    x_r = check_input_grad(wblk, dG, dx, L, layers, what=f"{what}: dx") if dx is not None else 0.0
    return {"dG": g_r, "dx": x_r}


def check_input_grad(wblk, dG, dx, L, layers, what="dx"):
    """dx [S][T][L] == W_ih[0]^T dG[0] of the kernel's own dG within c_acc(4L) S."""
    wi = split_w(wblk.double(), L, layers)[0][0]
    g0 = dG[0].double()
    ref, Sx = g0 @ wi, g0.abs() @ wi.abs()
    return _worst((dx.double().reshape(ref.shape) - ref).abs(), c_acc(4 * L) * Sx + TINY_F32, what, ("sequence", "time", "unit"))


def input_grad_ref(wblk, dG, L, layers):
    """(W_ih[0]^T dG[0] in float64, c_acc(4L) S): the pair kernel's dz, which its seam consumes."""
    wi = split_w(wblk.double(), L, layers)[0][0]
    g0 = dG[0].double()
    return g0 @ wi, c_acc(4 * L) * (g0.abs() @ wi.abs())


# ---- weight gradient -----------------------------------------------------------------------------------------------

def wgrad_pass(dG, hs, hprev, L, layers, f32=False, prev=None, defect=None):
    """gblk (the weight block's layout) = dG^T [hs | hprev | 1] per layer, float64 rounded to f32 or f32 arithmetic;
    prev: accumulate = 1 onto it."""
    dt = torch.float32 if f32 else torch.float64
    out = []
    for l in range(layers):
        g = dG[l].reshape(-1, 4 * L).to(dt)
        x, h = hs[l].reshape(-1, L).to(dt), hprev[l].reshape(-1, L).to(dt)
        gih, ghh, b = g.t() @ x, g.t() @ h, g.sum(0)
        bh = b
        if defect == "bias_nonzero_rows":
            bh = g[(h != 0).any(1)].sum(0)
        if defect == "edge_tile" and l == layers - 1:
            ghh = ghh.clone()
            ghh[(4 * L - 1) // 16 * 16:, (L - 1) // 16 * 16:] = 0          # the last (partial) 16 x 16 tile
        out.append(torch.cat([gih.reshape(-1), ghh.reshape(-1), b, bh]))
    out = torch.cat(out)
    if prev is not None and defect != "accumulate_overwrites":
        out = prev.to(dt) + out
    return out.float()


def check_wgrad(dG, hs, hprev, gblk, L, layers, prev=None, what="lstm wgrad"):
    """Every one of the 8L^2 + 8L entries per layer against dG^T [hs | hprev | 1] in float64 from the tensors handed to
    the kernel."""
    d = torch.float64
    R = dG.shape[1] * dG.shape[2]
    worst = 0.0
    for l in range(layers):
        g = dG[l].reshape(-1, 4 * L).to(d)
        x, h = hs[l].reshape(-1, L).to(d), hprev[l].reshape(-1, L).to(d)
        ref = torch.cat([(g.t() @ x).reshape(-1), (g.t() @ h).reshape(-1), g.sum(0), g.sum(0)])
        Sx = torch.cat([(g.abs().t() @ x.abs()).reshape(-1), (g.abs().t() @ h.abs()).reshape(-1), g.abs().sum(0), g.abs().sum(0)])
        bnd = (c_acc(R) + 4 * U) * Sx + TINY_F32
        sl = slice(l * layer_floats(L), (l + 1) * layer_floats(L))
        if prev is not None:
            ref = prev[sl].to(d) + ref
            bnd = bnd + U * ref.abs()
        worst = max(worst, _worst((gblk[sl].to(d) - ref).abs(), bnd, f"{what}: layer {l}", ("entry of the layer's block",)))
    return worst


def wgrad_entry_name(e, L):
    """Name entry e of a layer's block: (matrix, gate row, column)."""
    if e < 8 * L * L:
        return ("w_ih" if e < 4 * L * L else "w_hh", (e % (4 * L * L)) // L, e % L)
    e -= 8 * L * L
    return ("b_ih" if e < 4 * L else "b_hh", e % (4 * L), None)


# ---- case tables ---------------------------------------------------------------------------------------------------
# Small S*T everywhere: the whole GPU file has to stay a small share of the suite.  Every T at a dispatch boundary
# comes from first_change.

def _T(fn):
    T, _ = first_change(fn)
    assert T is not None
    return T


T_FWD_32x4 = _T(lambda T: fwd_dispatch(T, 32, 4))              # the forward wavefront kernel's first refused T
T_BWD_32x4 = _T(lambda T: bwd_dispatch(T, 32, 4))              # the backward wavefront kernel's
T_PAIR_FWD_32x4 = _T(lambda T: pair_fwd_dispatch(T, 32, 4))
T_PAIR_BWD_32x4 = _T(lambda T: pair_bwd_dispatch(T, 32, 4))
T_BWD_25x2 = _T(lambda T: bwd_dispatch(T, 25, 2))
T_FWD_TL = _T(lambda T: fwd_dispatch(T, 32, 9))                # "T*L too large" of the fall-back kernel
T_BWD_TL = _T(lambda T: bwd_dispatch(T, 32, 9))


def _case(**kw):
    c = dict(S=2, T=3, layers=1, wT=False, nparts=1, pad=0, cast=None, regime="small", seed=0)
    c.update(kw)
    return c


# cast: (dtype name, cast_ld); pad: part_stride - S*T*L
FWD_CASES = [
    _case(L=2, layers=4, S=3, T=5, regime="wide"),
    _case(L=7, layers=2, S=2, T=2, wT=True, nparts=2, cast=("f32", 64)),
    _case(L=24, layers=4, S=2, T=3, nparts=3, pad=5, cast=("bf16", 24), regime="saturated"),
    _case(L=25, layers=2, S=3, T=7, wT=True, nparts=5, cast=("bf16", 64), regime="wide"),
    _case(L=28, layers=1, S=1, T=1, nparts=4, cast=("f32", 128)),
    _case(L=31, layers=4, S=2, T=5, regime="saturated", wT=True),
    _case(L=32, layers=4, S=2, T=9, wT=True, nparts=4, pad=64, cast=("bf16", 64), regime="wide"),
    _case(L=32, layers=1, S=1, T=1, cast=("bf16", 128), regime="saturated"),
    _case(L=32, layers=4, S=1, T=T_FWD_32x4 - 1, cast=("f32", 32)),            # the last T of the wavefront kernel
    _case(L=32, layers=4, S=1, T=T_FWD_32x4, regime="wide"),                   # lstm_fwd_k<32>: the LDS no longer fits
    _case(L=32, layers=9, S=2, T=3, regime="saturated"),                       # lstm_fwd_k<32>: more than 8 layers
    _case(L=25, layers=2, S=1, T=_T(lambda T: fwd_dispatch(T, 25, 2)), regime="small"),
    _case(L=33, layers=4, S=2, T=3, wT=True, regime="wide"),
    _case(L=40, layers=1, S=1, T=2),
    _case(L=50, layers=4, S=2, T=5, wT=True, regime="saturated"),
    _case(L=64, layers=2, S=2, T=3, regime="wide"),
    _case(L=75, layers=2, S=1, T=5, wT=True),
    _case(L=88, layers=1, S=2, T=3, regime="saturated"),
    _case(L=100, layers=4, S=2, T=_T(lambda T: fwd_dispatch(T, 100, 4)) - 1, wT=True, regime="wide"),
    _case(L=112, layers=1, S=1, T=1, regime="wide"),
    _case(L=125, layers=2, S=2, T=3, wT=True, regime="saturated"),
    _case(L=128, layers=2, S=3, T=_T(lambda T: fwd_dispatch(T, 128, 2)) - 1),
]

# refusals: an error and nothing written.  (entry, kwargs of the dispatch)
FWD_REFUSALS = [
    _case(L=50, layers=1, S=1, T=_T(lambda T: fwd_dispatch(T, 50, 1))),
    _case(L=100, layers=2, S=1, T=_T(lambda T: fwd_dispatch(T, 100, 2))),
    _case(L=128, layers=1, S=1, T=_T(lambda T: fwd_dispatch(T, 128, 1))),
    _case(L=32, layers=4, S=1, T=T_FWD_32x4, nparts=2, cast=("bf16", 64)),     # the _ex forms past the wavefront kernel
    _case(L=32, layers=9, S=1, T=T_FWD_TL),
]

# bwd cases: entry "plain" (rbvae_lstm_bwd), "ex" (slabs / cast / colsum), "bin" (fused binarise backward).
# saved: "forward" = acts / cs of a float64 forward pass rounded to f32; "random" = independent gate values
def _bcase(**kw):
    c = _case(entry="plain", saved="forward", colsum=False, hard=0, tau_dev=False, klw=0.0, clamp=1, ghs=False)
    c.update(kw)
    return c


BWD_CASES = [
    _bcase(L=1, layers=4, S=3, T=5, regime="wide"),
    _bcase(L=7, layers=2, S=2, T=2, entry="ex", nparts=2, cast=("f32", 64), colsum=True),
    _bcase(L=24, layers=4, S=2, T=3, entry="ex", nparts=4, pad=7, cast=("bf16", 24), regime="saturated"),
    _bcase(L=25, layers=2, S=3, T=7, entry="ex", nparts=5, cast=("bf16", 64), colsum=True, regime="wide"),
    _bcase(L=25, layers=2, S=1, T=T_BWD_25x2, saved="random"),                                  # lstm_bwd_k<32>
    _bcase(L=28, layers=1, S=1, T=1, entry="bin", tau_dev=True, klw=1.0, ghs=True, cast=("f32", 128), colsum=True),
    _bcase(L=31, layers=4, S=2, T=5, regime="saturated", wT=True),
    _bcase(L=32, layers=4, S=2, T=9, entry="bin", klw=0.5, clamp=0, ghs=True, hard=1, cast=("bf16", 64), colsum=True, regime="wide"),
    _bcase(L=32, layers=4, S=2, T=5, entry="bin", klw=0.0, cast=("bf16", 128), regime="saturated"),
    _bcase(L=32, layers=1, S=2, T=37, entry="ex", nparts=3, colsum=True),        # more than U staging rounds, T*L > block
    _bcase(L=32, layers=4, S=1, T=T_BWD_32x4 - 1, entry="ex", nparts=2, pad=3, cast=("f32", 32), regime="wide"),
    _bcase(L=32, layers=4, S=2, T=T_BWD_32x4, regime="wide"),                                   # lstm_bwd_k<32>
    _bcase(L=32, layers=9, S=2, T=3, regime="saturated", saved="random"),                       # lstm_bwd_k<32>
    _bcase(L=33, layers=4, S=2, T=3, wT=True, regime="wide"),
    _bcase(L=40, layers=1, S=1, T=2),
    _bcase(L=50, layers=4, S=2, T=5, wT=True, regime="saturated"),
    _bcase(L=64, layers=2, S=2, T=3, regime="wide", saved="random"),
    _bcase(L=75, layers=2, S=1, T=5, wT=True),
    _bcase(L=88, layers=1, S=2, T=3, regime="saturated"),
    _bcase(L=100, layers=4, S=2, T=_T(lambda T: bwd_dispatch(T, 100, 4)) - 1, wT=True, regime="wide"),
    _bcase(L=101, layers=1, S=1, T=1, regime="wide"),
    _bcase(L=125, layers=2, S=2, T=3, wT=True, regime="saturated"),
    _bcase(L=128, layers=2, S=3, T=7),
]

BWD_REFUSALS = [
    _bcase(L=50, layers=1, S=1, T=_T(lambda T: bwd_dispatch(T, 50, 1))),
    _bcase(L=128, layers=2, S=1, T=_T(lambda T: bwd_dispatch(T, 128, 2))),
    _bcase(L=32, layers=4, S=1, T=T_BWD_32x4, entry="ex", nparts=2),
    _bcase(L=32, layers=4, S=1, T=T_BWD_32x4, entry="bin"),
    _bcase(L=32, layers=9, S=1, T=T_BWD_TL),
]


def _pcase(**kw):
    c = _case(unit=1, hard=0, tau_dev=False, klw=1.0, clamp=1, ghs=False, extra=False, dz=True, kl=True, colsum=True,
              saved="forward")
    c.update(kw)
    return c


PAIR_FWD_CASES = [
    _pcase(L=32, layers=4, S=2, T=5, wT=True, nparts=3, cast=("bf16", 64), regime="wide"),                  # unit_k
    _pcase(L=32, layers=1, S=1, T=1, hard=1, cast=("f32", 128), regime="saturated", tau_dev=True),         # unit_k
    _pcase(L=32, layers=4, S=2, T=T_PAIR_FWD_32x4 - 1, unit=0, nparts=5, pad=9, cast=("bf16", 128)),       # <32,true>
    _pcase(L=32, layers=2, S=3, T=2, unit=0, hard=1, regime="wide", kl=False, clamp=0),                     # <32,true>
    _pcase(L=25, layers=2, S=3, T=7, wT=True, nparts=2, cast=("bf16", 64), regime="wide", tau_dev=True),   # <32,false,28>
    _pcase(L=28, layers=4, S=1, T=3, hard=1, regime="saturated", cast=("f32", 28)),                        # <32,false,28>
    _pcase(L=7, layers=2, S=2, T=3, nparts=4, cast=("f32", 64), regime="saturated"),                       # <32,false>
    _pcase(L=24, layers=4, S=2, T=5, wT=True, regime="wide", clamp=0),
    _pcase(L=31, layers=3, S=2, T=2, hard=1),
    _pcase(L=12, layers=1, S=1, T=9, regime="wide"),
]

PAIR_BWD_CASES = [
    _pcase(L=32, layers=4, S=2, T=5, nparts=4, klw=1.0, ghs=True, cast=("bf16", 64), regime="wide"),                   # unit_k
    _pcase(L=32, layers=1, S=1, T=1, klw=0.0, extra=True, cast=("f32", 128), regime="saturated", tau_dev=True, dz=False),
    _pcase(L=32, layers=4, S=2, T=T_PAIR_BWD_32x4 - 1, unit=0, nparts=5, pad=9, klw=0.5, ghs=True, extra=True, hard=1,
           cast=("bf16", 128)),                                                                                         # <32,true>
    _pcase(L=32, layers=2, S=3, T=2, unit=0, regime="wide", clamp=0, saved="random", colsum=False),
    _pcase(L=25, layers=2, S=3, T=7, nparts=2, cast=("bf16", 64), regime="wide", tau_dev=True, ghs=True),             # <32,false>
    _pcase(L=7, layers=2, S=2, T=3, nparts=3, cast=("f32", 64), regime="saturated", extra=True, hard=1),
    _pcase(L=12, layers=4, S=1, T=3, klw=0.0, regime="wide", dz=False),
    _pcase(L=31, layers=3, S=2, T=2, klw=1.0, clamp=0, ghs=True, saved="random"),
]

PAIR_REFUSALS = [("fwd", _pcase(L=32, layers=4, S=1, T=T_PAIR_FWD_32x4)), ("bwd", _pcase(L=32, layers=4, S=1, T=T_PAIR_BWD_32x4)),
                 ("fwd", _pcase(L=33, layers=1, S=1, T=2)), ("bwd", _pcase(L=32, layers=5, S=1, T=2))]

# weight gradient: R = S*T in {1, 3, 4, 5, 63, 64, 65, 257}; 4L and L + 1 not multiples of 16 at L = 7, 25, 50, 75, 125
WGRAD_CASES = [
    dict(L=7, layers=2, S=1, T=1, pair=False, acc=0, regime="small"),
    dict(L=25, layers=2, S=1, T=3, pair=True, acc=0, regime="wide"),
    dict(L=32, layers=4, S=2, T=2, pair=True, acc=1, regime="saturated"),
    dict(L=31, layers=1, S=5, T=1, pair=False, acc=1, regime="wide"),
    dict(L=50, layers=1, S=7, T=9, pair=False, acc=0, regime="saturated"),
    dict(L=75, layers=2, S=8, T=8, pair=False, acc=1, regime="small"),
    dict(L=125, layers=1, S=5, T=13, pair=True, acc=1, regime="wide"),
    dict(L=2, layers=3, S=1, T=257, pair=True, acc=0, regime="small"),
    dict(L=128, layers=1, S=1, T=5, pair=False, acc=0, regime="wide"),
]


def fwd_instance(c):
    return fwd_dispatch(c["T"], c["L"], c["layers"], in_parts=c["nparts"] > 1 or c["pad"] > 0, cast=c["cast"] is not None)


def bwd_instance(c):
    return bwd_dispatch(c["T"], c["L"], c["layers"], nparts=c["nparts"], cast=c["cast"] is not None,
                        dx_colsum=c["colsum"], bin=c["entry"] == "bin")


def covered_instances():
    """Every instance the case tables launch, from the restated dispatch."""
    got = {fwd_instance(c) for c in FWD_CASES} | {bwd_instance(c) for c in BWD_CASES}
    got |= {pair_fwd_dispatch(c["T"], c["L"], c["layers"], c["unit"]) for c in PAIR_FWD_CASES}
    got |= {pair_bwd_dispatch(c["T"], c["L"], c["layers"], c["unit"]) for c in PAIR_BWD_CASES}
    got |= {wgrad_dispatch(c["pair"], c["acc"]) for c in WGRAD_CASES}
    return got


def case_id(c):
    return "-".join(f"{k}{v}" for k, v in c.items() if k in ("L", "layers", "S", "T", "entry", "unit", "regime"))


# ---- case data -----------------------------------------------------------------------------------------------------

def gen_for(c, salt=0):
    return torch.Generator().manual_seed(1000 * c["L"] + 10 * c["T"] + c["layers"] + 7919 * salt + c.get("seed", 0))


def make_input(c, gen):
    """x [S][T][L] (distinct per sequence) as nparts slabs [nparts][S*T*L + pad] whose f32 slab-order sum is the input."""
    S, T, L, n = c["S"], c["T"], c["L"], c["nparts"]
    parts = torch.randn(n, S * T * L, generator=gen) * (1.0 if n == 1 else 0.7)
    return parts


def saved_state(c, w, gen):
    """(acts, cs, hs, hprev) for a backward case: a float64 forward pass rounded to f32 ("forward"), or independent gate
    values in (0,1) / (-1,1) with cell states of moderate size ("random")."""
    S, T, L, layers = c["S"], c["T"], c["L"], c["layers"]
    x = torch.randn(S, T, L, generator=gen)
    hs, hp, acts, cs = forward_pass(w, x, L, layers)
    if c["saved"] == "random":
        acts = torch.rand(layers, S, T, 4 * L, generator=gen)
        acts[..., 2 * L:3 * L] = acts[..., 2 * L:3 * L] * 2 - 1
        cs = torch.randn(layers, S, T, L, generator=gen)
    return acts.contiguous(), cs.contiguous(), hs, hp
