"""Launch-by-launch references for the trace of the LDM encoder / decoder (symbols-from-video_amd/ldm.py, _LDMBlocks._trace).
torch only; importable without a GPU.

A record is (prefix, op, inputs, output, geometry): the tensors a launch read and the tensor (or pair) it stored.  For
every op this module holds
  the reference     float64 from the RECORDED inputs as the kernel sees them (storage-rounded activations, weights rounded
                    to the storage type), with its condition scale S and the element-wise bound of tests/_bounds.py
                    (convolutions / GEMMs: check(K = taps Kc, pre = value before the addend, S_in / u_in for the operand
                    normalised while it is staged) or of tests/_ldm_cases.py (GroupNorm, softmax, attention) and
                    tests/_halo_cases.py (statistics out of tile partials);
  the storage model the same float64 arithmetic, rounded to the storage type wherever the device stores or stages: the
                    floor of the relative-L2 gate and the stand-in device of test_ldm_trace_cpu.py;
  the exact form    no rounding at all: composed along expected_stages it IS oracle/ldm_oracle.py / _ldm_decoder_ref.py.
GroupNorm statistics are the float64 mean / variance of the stored input per (image, group); the recorded scale / shift
(mean / rstd) are checked against them.  The storage model and the exact form take them from the recorded partials
instead (the parallel-variance merge of rbvae_gn_finish_tiles), so the composition exercises the hand-off.

walk() restates ldm.py's wiring (which launch reads which tensor, which dispatch branch runs) over an executor:
expected_stages() lists the (prefix, op) a pass must record; run() evaluates the storage model or the exact form along it
and returns records in the device's format, optionally with one named wiring defect at one record."""
import torch
import torch.nn.functional as F

import _bounds as B
import _halo_cases as HC
import _ldm_cases as LC
import _ldm_decoder_ref as DR

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
U32 = B.U32
G = 32                                  # GroupNorm(32) everywhere (model.py:33-34)
EPS = 1e-6
SCALE_FACTOR = 0.18215
TWO = ("conv_in", "conv3_halo", "gn_affine", "gn_finish")       # ops that store two tensors
L2_OPS = ("conv3", "conv1", "conv3_halo", "conv_in", "conv_in_gemm", "down", "gn", "gn_apply", "attention", "scores",
          "softmax", "pv", "up_halo", "up_gather", "up_unfolded")                 # storage-type outputs with a rounding floor
UP_DEFECTS = ("dropped_tap", "swapped_classes", "wrong_edge", "unfolded_w1")

# The smallest shapes at which each dispatch decision of ldm.py flips.  `reach`: what the case's stage list must hold
# (asserted from expected_stages, i.e. from the library's own _ok queries), so a case that stops reaching its row fails.
#   3 x 32 x 128: the maps are 32 x 128, 16 x 64, 8 x 32 and 4 x 16.  8 x 32 hangs over the 16 x 16 tile and runs the halo
#   kernel; rbvae_conv3x3_halo_ok refuses 4 x 16 (and 8 x 8), so the last level and the mid blocks of every case but
#   1 x 128 x 128 take the gather form -- the only smaller maps that hang over a tile are refused the same way.
ENC_CASES = [
    dict(id="bf16_halo_2x64x64", dtype="bf16", impl="halo", N=2, H=64, W=64,
         reach=("conv_in", "gn_finish", "gn_finish_ms", "gn_affine", "gn_apply", "conv3_halo", "attention")),
    dict(id="bf16_halo_3x32x128", dtype="bf16", impl="halo", N=3, H=32, W=128,
         reach=("conv_in", "gn_finish", "gn_finish_ms", "conv3_halo", "conv3", "attention")),
    dict(id="bf16_halo_1x128x128", dtype="bf16", impl="halo", N=1, H=128, W=128,
         reach=("conv_in", "gn_finish_ms", "gn_apply", "conv3_halo", "attention")),
    dict(id="f32_halo_2x32x64", dtype="f32", impl="halo", N=2, H=32, W=64,
         reach=("im2col", "conv_in_gemm", "gn_affine", "conv3_halo", "scores", "softmax", "transpose", "pv")),
    dict(id="f32_gather_1x64x64", dtype="f32", impl="gather", N=1, H=64, W=64, reach=("im2col", "conv_in_gemm", "gn", "conv3", "scores"),
         never=("conv3_halo", "conv_in", "gn_apply")),
    dict(id="bf16_gather_1x64x64", dtype="bf16", impl="gather", N=1, H=64, W=64, reach=("im2col", "conv_in_gemm", "gn", "conv3", "attention"),
         never=("conv3_halo", "conv_in", "gn_apply")),
]
DEC_CASES = [
    dict(id="bf16_halo_2x8x8", dtype="bf16", impl="halo", N=2, H=8, W=8, reach=("up_halo", "attention"), never=("up_gather",),
         forms=("halo", "halo", "halo")),
    dict(id="bf16_halo_1x4x12", dtype="bf16", impl="halo", N=1, H=4, W=12, reach=("up_halo", "up_gather", "scores", "softmax", "pv"),
         forms=("gather", "halo", "halo")),
    dict(id="f32_gather_1x8x8", dtype="f32", impl="gather", N=1, H=8, W=8, reach=("up_gather", "scores"), never=("up_halo",),
         forms=("gather",) * 3),
    dict(id="bf16_unfolded_1x8x8", dtype="bf16", impl="unfolded", N=1, H=8, W=8, reach=("nearest2x", "up_unfolded"),
         never=("up_halo", "up_gather"), forms=("unfolded",) * 3),
    # 16 tokens; the first upsampled map is 8 x 8, which rbvae_conv3x3_halo_ok refuses: the as-written form on the gather GEMM
    dict(id="bf16_unfolded_1x4x4", dtype="bf16", impl="unfolded", N=1, H=4, W=4, reach=("nearest2x", "up_unfolded", "scores"),
         never=("up_halo", "up_gather", "attention"), forms=("unfolded",) * 3),
]
TDT = {"f32": F32, "bf16": BF}


def make_model(sfv, c, seed=11):
    """(model on the CPU, its parameters under the reference's names) of a case: torch's default initialisation"""
    torch.manual_seed(seed)
    if "forms" in c:
        m = sfv.LDMDecoder(compute_dtype=c["dtype"], upsample_impl=c["impl"], halo_where_covered=True)
    else:
        m = sfv.LDMEncoder(compute_dtype=c["dtype"], conv_impl=c["impl"])
    return m, {k: v.detach().clone() for k, v in m.state_dict().items()}


def make_input(c):
    g = torch.Generator().manual_seed(sum(map(ord, c["id"])))
    if "forms" in c:
        return torch.randn(c["N"], 4, c["H"], c["W"], generator=g) * 0.5
    return torch.rand(c["N"], 3, c["H"], c["W"], generator=g) * 2 - 1


def assert_reach(c, stages):
    ops = {op for _, op in stages}
    assert set(c["reach"]) <= ops, f"{c['id']}: the dispatch no longer reaches {sorted(set(c['reach']) - ops)}"
    assert not ops & set(c.get("never", ())), f"{c['id']}: reached {sorted(ops & set(c.get('never', ())))}"
_ru = lambda x, m: (x + m - 1) // m * m


class Mode:
    """kind "both": the reference and the storage model; "exact": no rounding anywhere (float64 weights)."""

    def __init__(self, tdt, kind="both"):
        self.tdt, self.kind, self.exact = tdt, kind, kind == "exact"
        self.name = "f32" if tdt == F32 else "bf16"

    def w(self, t):
        """a weight or a frame as the kernel sees it"""
        return t.double() if self.exact else t.to(self.tdt).double()

    def r(self, t):
        """a value the device stores or stages in the storage type"""
        return t if self.exact else t.double().to(self.tdt).double()


def nchw(rows, N, H, W):
    return rows.double().reshape(N, H, W, -1).permute(0, 3, 1, 2)


def wb(P, name):
    if name.endswith(".qkv"):
        base = name[:-4]
        return (torch.cat([P[f"{base}.{n}.weight"] for n in "qkv"]), torch.cat([P[f"{base}.{n}.bias"] for n in "qkv"]))
    return P[f"{name}.weight"], P[f"{name}.bias"]


def tile_of_rows(N, H, W, th, tw):
    """statistics tile (n tiles_r + ty) tiles_c + tx of every NHWC row -> (tile [N H W], tiles per image)"""
    tr, tc = LC.cdiv(H, th), LC.cdiv(W, tw)
    p = torch.arange(N * H * W)
    n, y, x = p // (H * W), p // W % H, p % W
    return (n * tr + y // th) * tc + x // tw, tr * tc


def tile_stats(stored, N, H, W, th, tw, cg):
    """float64 (mean, M2) per (tile, group) of stored rows, flat in the partials' layout [(tile G + group)][2]"""
    tile, nb = tile_of_rows(N, H, W, th, tw)
    mean, m2 = HC.tile_stats_ref(stored, tile, N * nb, cg)[:2]
    return torch.stack([mean, m2], -1).reshape(-1)


def merge_tiles(part, N, H, W, C, th, tw):
    """rbvae_gn_finish_tiles' merge in float64: partials -> (mean, rstd) [N][G]"""
    cg = C // G
    tr, tc = LC.cdiv(H, th), LC.cdiv(W, tw)
    p = part.double().reshape(-1)[:N * tr * tc * G * 2].reshape(N, tr * tc, G, 2)
    hh = torch.tensor([min(th, H - r * th) for r in range(tr)], dtype=F64)
    ww = torch.tensor([min(tw, W - c * tw) for c in range(tc)], dtype=F64)
    cnt = (hh[:, None] * ww[None, :]).reshape(1, -1, 1) * cg
    total = H * W * cg
    mean = (cnt * p[..., 0]).sum(1) / total
    q = (p[..., 1] + cnt * (p[..., 0] - mean[:, None]) ** 2).sum(1)
    return mean, (q / total + EPS).rsqrt()


def scale_shift(mean, rstd, gamma, beta, b_mean=None, b_rstd=None):
    """(scale, shift) [N][C] float64 of per-group statistics, with their bounds when the statistics' are given: scale =
    rstd gamma (one rounding), shift = beta - mean scale (three), the statistics' own error carried through."""
    N, C = mean.shape[0], gamma.numel()
    ex = lambda s: s.double().reshape(N, G, 1).expand(N, G, C // G).reshape(N, C)
    ga, be = gamma.double()[None], beta.double()[None]
    sc = ex(rstd) * ga
    ms = ex(mean) * sc
    sh = be - ms
    if b_mean is None:
        return sc, sh
    b_sc = ex(b_rstd) * ga.abs() + U32 * sc.abs() + B.TINY
    b_sh = ex(b_mean) * sc.abs() + ex(mean).abs() * b_sc + 3 * U32 * (be.abs() + ms.abs()) + B.TINY
    return sc, sh, b_sc, b_sh


class Res:
    """ref / model: lists of float64 tensors shaped like the stored ones; stat: which are f32 statistics; chk(got list) ->
    worst |err| / bound (raises outside the bound); cols: the declared columns of output 0 (the rest is padding)"""

    def __init__(self, ref, model, chk, stat=(False,), cols=None):
        self.ref, self.model, self.chk, self.stat, self.cols = ref, model, chk, stat, cols


def _padded(val, ncols):
    out = torch.zeros(val.shape[0], ncols, dtype=F64)
    out[:, :val.shape[1]] = val
    return out


def _conv_res(M, ref, S, bias, addend, K, ncols, what, scale=1.0, ref_m=None, S_in=None, u_in=0.0, nhw=None, extra=None):
    """a convolution / GEMM whose float64 sum is ref (S on |operands|; ref_m: the sum over the staged-and-rounded operand)
    -> Res: bias, the store's rounding, the addend added to the rounded value and rounded again"""
    if S_in is not None:
        S_in = S.clone()
    ref_m = ref if ref_m is None else ref_m
    if bias is not None:
        ref, ref_m, S = ref + bias.double(), ref_m + bias.double(), S + bias.double().abs()
    pre, val, mval = None, ref, M.r(ref_m)
    if addend is not None:
        pre, val, mval = ref, ref + addend.double(), M.r(mval + addend.double())
    cout = ref.shape[1]

    def chk(got):
        g = got[0].detach().cpu().double()
        assert g.shape == (ref.shape[0], ncols), f"{what}: stored shape {tuple(g.shape)}"
        assert bool((g[:, cout:] == 0).all()), f"{what}: the padding columns {cout}.. are not zero"
        worst = B.check(g[:, :cout], val, S, out_dtype=M.tdt, K=K, scale=scale, pre=pre, S_in=S_in, u_in=u_in, nhw=nhw,
                        what=what)
        return max(worst, extra(got)) if extra else worst

    return Res([_padded(val, ncols)], [_padded(mval, ncols)], chk, cols=cout)


def _exact_res(M, val, what):
    def chk(got):
        g = got[0].detach().cpu().double()
        assert g.shape == val.shape and torch.equal(g, val), f"{what}: not bit-equal to the reference"
        return 0.0
    return Res([val], [val], chk)


def _bound_res(M, items, what, stat):
    """items: [(ref, model, bound)] per output"""
    def chk(got):
        worst = 0.0
        for i, (r, _, b) in enumerate(items):
            g = got[i].detach().cpu().double().reshape(-1)[:r.numel()].reshape(r.shape)
            worst = max(worst, LC.check_bound(g, r, b, f"{what} [{i}]"))
        return worst
    return Res([r for r, _, _ in items], [m for _, m, _ in items], chk, stat=stat)


# ---- the ops ---------------------------------------------------------------------------------------------------------

def evaluate(rec, P, M, defect=None):
    """Res of one record (prefix, op, inputs, output or None, geometry) under Mode M.  defect: a named defect of this op's
    own arithmetic (the wiring defects are run()'s)."""
    prefix, op, ins, stored, g = rec
    what = f"{prefix} {op}"
    c = lambda t: None if t is None else t.detach().cpu()
    ins = tuple(c(t) for t in ins)
    first = stored[0] if isinstance(stored, (tuple, list)) else stored
    ncols = g.get("ncols", first.shape[1] if first is not None and first.dim() == 2 else g.get("cout", g.get("C")))

    if op in ("conv3", "up_unfolded", "down", "conv3_halo"):
        N, H, W = g["N"], g["H"], g["W"]
        cin, cout = (g["C"], g["C"]) if op == "up_unfolded" else (g["cin"], g["cout"])
        w, bias = wb(P, prefix)
        w = M.w(w)
        if op == "down":
            pad = (1, 0, 1, 0) if defect == "pad_top_left" else (0, 1, 0, 1)
            conv = lambda a, w: F.conv2d(F.pad(a, pad), w, stride=2)
            nhw = (N, H // 2, W // 2)
        else:
            conv = lambda a, w: F.conv2d(a, w, padding=1)
            nhw = (N, H, W)
        x = ins[0]
        addend = ins[-1] if op in ("conv3", "conv3_halo") else None
        a = nchw(x, N, H, W)[:, :cin]
        kw, a_m, extra = {}, None, None
        if op == "conv3_halo" and g["fused"]:
            a, tmax = B.staged_operand(a, ins[1], ins[2], True)
            kw = dict(S_in=True, u_in=0.0 if M.exact else B.staged_u_in(M.tdt, True, tmax))
            a_m = M.r(a)
        ref, S = B.rows(conv(a, w)), B.rows(conv(a.abs(), w.abs()))
        ref_m = None if a_m is None or M.exact else B.rows(conv(a_m, w))
        if op == "conv3_halo":
            cg = cout // G
            tile, nb = tile_of_rows(N, H, W, 16, 16)
            extra = lambda got: max(HC.check_tile_stats(got[1].detach().cpu().reshape(-1)[:N * nb * G * 2], got[0].detach().cpu(),
                                                        tile, N * nb, cg, what + " statistics"))
        r = _conv_res(M, ref, S, bias, addend, 9 * x.shape[1], ncols, what, ref_m=ref_m, nhw=nhw, extra=extra, **kw)
        if op == "conv3_halo":
            r.ref.append(tile_stats(r.ref[0], N, H, W, 16, 16, cg))
            r.model.append(tile_stats(r.model[0], N, H, W, 16, 16, cg))
            r.stat = (False, True)
        return r

    if op == "conv_in":
        N, C, H, W, cout = g["N"], g["C"], g["H"], g["W"], g["cout"]
        w, bias = wb(P, prefix)
        a, w = M.w(ins[0]), M.w(w)
        cg = cout // G
        tile, nb = tile_of_rows(N, H, W, 8, 16)
        extra = lambda got: max(HC.check_tile_stats(got[1].detach().cpu().reshape(-1)[:N * nb * G * 2], got[0].detach().cpu(), tile,
                                                    N * nb, cg, what + " statistics"))
        r = _conv_res(M, B.rows(F.conv2d(a, w, padding=1)), B.rows(F.conv2d(a.abs(), w.abs(), padding=1)), bias, None, 64,
                      ncols, what, nhw=(N, H, W), extra=extra)
        r.ref.append(tile_stats(r.ref[0], N, H, W, 8, 16, cg))
        r.model.append(tile_stats(r.model[0], N, H, W, 8, 16, cg))
        r.stat = (False, True)
        return r

    if op == "im2col":
        N, C, H, W, K = g["N"], g["C"], g["H"], g["W"], g["K"]
        u = F.unfold(M.w(ins[0]), 3, padding=1).reshape(N, C, 9, H * W).permute(0, 3, 2, 1).reshape(N * H * W, 9 * C)
        return _exact_res(M, _padded(u, K), what)

    if op == "conv_in_gemm":
        C, K, cout = g["C"], g["K"], g["cout"]
        w, bias = wb(P, prefix)
        w = M.w(w).permute(0, 2, 3, 1).reshape(cout, 9 * C)
        a = ins[0].double()[:, :9 * C]
        return _conv_res(M, a @ w.t(), a.abs() @ w.abs().t(), bias, None, K, ncols, what, nhw=(g["N"], g["H"], g["W"]))

    if op == "conv1":
        cin, cout = g["cin"], g["cout"]
        w, bias = wb(P, prefix)
        w = M.w(w).reshape(cout, cin)
        a = ins[0].double()[:, :cin]
        return _conv_res(M, a @ w.t(), a.abs() @ w.abs().t(), bias, ins[1], ins[0].shape[1], ncols, what)

    if op in ("up_halo", "up_gather"):
        N, H, W, C = g["N"], g["H"], g["W"], g["C"]
        w, bias = wb(P, prefix)
        fd = defect if defect == "unfolded_w1" else None
        ud = defect if defect in UP_DEFECTS[:3] else None
        wf = DR.fold_upconv(w.double(), defect=fd) if M.exact else DR.fold_upconv(w.float(), defect=fd).to(M.tdt).double()
        a = nchw(ins[0], N, H, W)[:, :C]
        ref = B.rows(DR.upconv_folded(a, wf, ud))
        S = B.rows(DR.upconv_folded(a.abs(), DR.fold_upconv(w.double()).abs() if M.exact else
                                    DR.fold_upconv(w.float()).to(M.tdt).double().abs()))
        return _conv_res(M, ref, S, bias, None, 4 * ins[0].shape[1], ncols, what, nhw=(N, 2 * H, 2 * W))

    if op == "nearest2x":
        N, H, W = g["N"], g["H"], g["W"]
        return _exact_res(M, B.rows(F.interpolate(nchw(ins[0], N, H, W), scale_factor=2.0, mode="nearest")).contiguous(), what)

    if op == "latent_rows":
        N, Z, HW = g["N"], g["Z"], g["HW"]
        z = ins[0].reshape(N, Z, HW)
        v = (1. / SCALE_FACTOR * z.double()) if M.exact else (1. / SCALE_FACTOR * z.float()).to(M.tdt).double()     # ddpm.py:713
        return _exact_res(M, _padded(v.permute(0, 2, 1).reshape(N * HW, Z), ncols), what)

    if op in ("gn", "gn_apply", "gn_stats", "gn_affine", "gn_finish", "gn_finish_ms"):
        N, C = g["N"], g["C"]
        HW = g["HW"] if "HW" in g else g["H"] * g["W"]
        gamma, beta = wb(P, prefix)
        x3 = ins[0].double().reshape(N, HW, -1)[:, :, :C]
        swish = g.get("swish", 1)
        NG = N * G
        if op == "gn_apply":
            ms = ins[1].reshape(-1)
            y, b = LC.gn_bounds(x3, gamma, beta, G, M.tdt, 1, given=(ms[:NG], ms[NG:2 * NG]))["y"]
            return _bound_res(M, [(y, M.r(y), b)], what, (False,))
        if op in ("gn", "gn_stats", "gn_affine"):
            bd = LC.gn_bounds(x3, gamma, beta, G, M.tdt, swish, h=LC.gn_height_of(M.name, HW, C, G, True))
            (mean, b_mean), (rstd, b_rstd) = bd["mean"], bd["rstd"]
            if op == "gn":
                y, b = bd["y"]
                return _bound_res(M, [(y, M.r(y), b)], what, (False,))
            if op == "gn_stats":
                ms = torch.cat([mean, rstd])
                return _bound_res(M, [(ms, ms, torch.cat([b_mean, b_rstd]))], what, (True,))
            mean, rstd, b_mean, b_rstd = (t.reshape(N, G) for t in (mean, rstd, b_mean, b_rstd))
            ws = ins[1].double().reshape(-1)
            given = (ws[:NG].reshape(N, G), ws[NG:2 * NG].reshape(N, G))
        else:
            H, W, th, tw = g["H"], g["W"], g["th"], g["tw"]
            tile, nb = tile_of_rows(N, H, W, th, tw)
            mean, rstd, b_mean, b_rstd = HC.gn_finish_bounds(x3.reshape(N * HW, C), tile, N, HW, nb, C // G, EPS)
            given = merge_tiles(ins[1], N, H, W, C, th, tw)
        if op == "gn_finish_ms":
            ms, msm = torch.cat([mean.reshape(-1), rstd.reshape(-1)]), torch.cat([given[0].reshape(-1), given[1].reshape(-1)])
            return _bound_res(M, [(ms, msm, torch.cat([b_mean.reshape(-1), b_rstd.reshape(-1)]))], what, (True,))
        sc, sh, b_sc, b_sh = scale_shift(mean, rstd, gamma, beta, b_mean, b_rstd)
        scm, shm = scale_shift(given[0], given[1], gamma, beta)
        return _bound_res(M, [(sc, scm, b_sc), (sh, shm, b_sh)], what, (True, True))

    if op == "attention":
        N, hw, C = g["N"], g["hw"], g["C"]
        q, k, v = (ins[0][:, i * C:(i + 1) * C].reshape(N, hw, C) for i in range(3))
        scale = float(int(C) ** (-0.5))
        if M.exact:
            o = torch.softmax(q.double() @ k.double().transpose(1, 2) * scale, 2) @ v.double()
            return Res([o.reshape(N * hw, C)], [o.reshape(N * hw, C)], None)
        ref, bnd = LC.at_bounds(q, k, v, scale)
        s = q.double() @ k.double().transpose(1, 2) * scale
        p = M.r(torch.exp(s - s.max(2, keepdim=True).values))        # the probabilities are staged in the storage type
        model = M.r((p @ v.double()) / p.sum(2, keepdim=True)).reshape(N * hw, C)
        return _bound_res(M, [(ref, model, bnd)], what, (False,))

    if op == "scores":
        n, hw, C, ld = g["n"], g["hw"], g["C"], g["ld"]
        q, k = (t.double()[n * hw:(n + 1) * hw] for t in ins)
        if defect == "q_k_exchanged":
            q, k = k, q
        scale = float(int(C) ** (-0.5)) if M.exact else float(torch.tensor(float(int(C) ** (-0.5)), dtype=F32))
        return _conv_res(M, q @ k.t() * scale, q.abs() @ k.abs().t(), None, None, C, ld, what, scale=scale)

    if op == "softmax":
        hw, ld = g["hw"], g["ld"]
        x = ins[0][:, :hw]
        p, b = LC.sm_bounds(x, M.tdt)

        def chk(got):
            gt = got[0].detach().cpu().double()
            assert gt.shape == (hw, ld) and bool((gt[:, hw:] == 0).all()), f"{what}: the padding columns are not zero"
            return LC.check_bound(gt[:, :hw], p, b, what)
        return Res([_padded(p, ld)], [_padded(M.r(p), ld)], chk, cols=hw)

    if op == "transpose":
        n, hw, C, ld = g["n"], g["hw"], g["C"], g["ld"]
        return _exact_res(M, _padded(ins[0].double()[n * hw:(n + 1) * hw].t(), ld), what)

    if op == "pv":
        hw, C, ld = g["hw"], g["C"], g["ld"]
        p, vt = ins[0].double(), ins[1].double()
        return _conv_res(M, p @ vt.t(), p.abs() @ vt.abs().t(), None, None, ld, C, what)

    raise KeyError(op)


# ---- the wiring --------------------------------------------------------------------------------------------------------

class Dispatch:
    """The dispatch queries of a model, restated: `query(name, *args)` is the library's (sfv_amd._lib.query) or a stub."""

    def __init__(self, model, query):
        self.m, self.query = model, query
        self.dt = 0 if model.compute_dtype == "f32" else 1
        self.ke = 32 if self.dt == 0 else 64

    def halo_ok(self, N, H, W, cin, cout):
        tiles = N * ((H + 15) // 16) * ((W + 15) // 16) * (cout // 128)
        return (self.m.conv_impl == "halo" and cout % 32 == 0 and tiles >= self.m._halo_min_tiles and
                bool(self.query("rbvae_conv3x3_halo_ok", self.dt, H, W, H, W, cin, cout)))

    def attention_ok(self, hw, C):
        return bool(self.query("rbvae_attention_ok", self.dt, hw, C))

    def conv_in_ok(self, C, H, W, cout, N):
        return (self.m.conv_impl == "halo" and cout % 32 == 0 and _ru(9 * C, self.ke) == 64 and
                bool(self.query("rbvae_conv_in_ok", self.dt, C, H, W, cout, N, cout // 32)))

    def upconv_halo_ok(self, N, H, W, C):
        if self.m.upsample_impl != "halo" or not (self.m.halo_where_covered or self.m._upconv_halo_rule(N, H, W, C)):
            return False
        return bool(self.query("rbvae_upconv3x3_halo_ok", self.dt, N, H, W, C, C))


def walk(model, query, N, H, W, ex, x0=None):
    """ldm.py's forward over executor ex(prefix, op, inputs, **geometry) -> output (a pair for the ops in TWO).  model: an
    LDMEncoder (N x 3 x H x W frames) or LDMDecoder (N x 4 x H x W latents); returns the last output."""
    q = Dispatch(model, query)
    ke = q.ke

    def gn_halo(norm, conv, x, xst, cin, cout, addend):
        fused = cout // 128 <= 2
        sc = sh = None
        if xst is None:
            ws = ex(norm, "gn_stats", (x,), N=N, HW=H * W, C=cin)
        if fused:
            if xst is None:
                sc, sh = ex(norm, "gn_affine", (x, ws), N=N, HW=H * W, C=cin)
            else:
                sc, sh = ex(norm, "gn_finish", (x, xst[0]), N=N, H=H, W=W, C=cin, th=xst[1], tw=xst[2])
        else:
            ms = ws if xst is None else ex(norm, "gn_finish_ms", (x, xst[0]), N=N, H=H, W=W, C=cin, th=xst[1], tw=xst[2])
            x = ex(norm, "gn_apply", (x, ms), N=N, HW=H * W, C=cin)
        out, ost = ex(conv, "conv3_halo", (x, sc, sh, addend), N=N, H=H, W=W, cin=cin, cout=cout, fused=int(fused), norm=norm)
        return out, (ost, 16, 16)

    def res(prefix, x, xst, cin, cout):
        if q.halo_ok(N, H, W, cin, cout) and q.halo_ok(N, H, W, cout, cout):
            h, hst = gn_halo(f"{prefix}.norm1", f"{prefix}.conv1", x, xst, cin, cout, None)
            skip = x if cin == cout else ex(f"{prefix}.nin_shortcut", "conv1", (x, None), rows=N * H * W, cin=cin, cout=cout)
            return gn_halo(f"{prefix}.norm2", f"{prefix}.conv2", h, hst, cout, cout, skip)
        h = ex(f"{prefix}.norm1", "gn", (x,), N=N, HW=H * W, C=cin, swish=1)
        h = ex(f"{prefix}.conv1", "conv3", (h, None), N=N, H=H, W=W, cin=cin, cout=cout)
        h = ex(f"{prefix}.norm2", "gn", (h,), N=N, HW=H * W, C=cout, swish=1)
        skip = x if cin == cout else ex(f"{prefix}.nin_shortcut", "conv1", (x, None), rows=N * H * W, cin=cin, cout=cout)
        return ex(f"{prefix}.conv2", "conv3", (h, skip), N=N, H=H, W=W, cin=cout, cout=cout), None

    def attn(prefix, x, C, decoder):
        hw = H * W
        if hw % ke and not (decoder and hw % 8 == 0):
            raise ValueError("token count")
        h = ex(f"{prefix}.norm", "gn", (x,), N=N, HW=hw, C=C, swish=0)
        rows = N * hw
        if hw % ke == 0 and q.attention_ok(hw, C):
            qkv = ex(f"{prefix}.qkv", "conv1", (h, None), rows=rows, cin=C, cout=3 * C)
            o = ex(prefix, "attention", (qkv,), N=N, hw=hw, C=C)
            return ex(f"{prefix}.proj_out", "conv1", (o, x), rows=rows, cin=C, cout=C)
        ld = _ru(hw, ke)
        qq, kk, vv = (ex(f"{prefix}.{n}", "conv1", (h, None), rows=rows, cin=C, cout=C) for n in "qkv")
        os_ = []
        for n in range(N):
            s0 = ex(prefix, "scores", (qq, kk), n=n, hw=hw, C=C, ld=ld)
            p0 = ex(prefix, "softmax", (s0,), n=n, hw=hw, ld=ld)
            vt0 = ex(prefix, "transpose", (vv,), n=n, hw=hw, C=C, ld=ld)
            os_.append(ex(prefix, "pv", (p0, vt0), n=n, hw=hw, C=C, ld=ld))
        o = None if os_[0] is None else torch.cat(os_)
        return ex(f"{prefix}.proj_out", "conv1", (o, x), rows=rows, cin=C, cout=C)

    decoder = hasattr(model, "upsample_impl")
    h, hst = x0, None
    if decoder:
        h = ex("latent", "latent_rows", (x0,), N=N, Z=model.cfg["z_channels"], HW=H * W, ncols=ke)
    for prefix, kind, cin, cout in model.plan:
        if kind == "conv_in" and not decoder:
            if q.conv_in_ok(cin, H, W, cout, N):
                h, ost = ex(prefix, "conv_in", (x0,), N=N, C=cin, H=H, W=W, cout=cout)
                hst = (ost, 8, 16)
                continue
            K = _ru(9 * cin, ke)
            col = ex(prefix, "im2col", (x0,), N=N, C=cin, H=H, W=W, K=K)
            h = ex(prefix, "conv_in_gemm", (col,), N=N, C=cin, H=H, W=W, K=K, cout=cout)
        elif kind == "res":
            h, hst = res(prefix, h, hst, cin, cout)
            continue
        elif kind == "down":
            h = ex(prefix, "down", (h,), N=N, H=H, W=W, cin=cin, cout=cout)
            H, W = H // 2, W // 2
        elif kind == "attn":
            h = attn(prefix, h, cin, decoder)
        elif kind == "norm":
            h = ex(prefix, "gn", (h,), N=N, HW=H * W, C=cin, swish=1)
        elif kind == "conv_out":
            h = ex(prefix, "conv3", (h, None), N=N, H=H, W=W, cin=cin, cout=cout,
                   ncols=_ru(cout, 8) if decoder else _ru(cout, ke))
        elif kind in ("quant", "post_quant"):
            h = ex(prefix, "conv1", (h, None), rows=N * H * W, cin=cin, cout=cout, ncols=ke if decoder else cout)
        elif kind == "conv_in":
            h = ex(prefix, "conv3", (h, None), N=N, H=H, W=W, cin=cin, cout=cout)
        elif kind == "up":
            if model.upsample_impl == "unfolded":
                up = ex(prefix, "nearest2x", (h,), N=N, H=H, W=W, C=cin)
                h = ex(prefix, "up_unfolded", (up,), N=N, H=2 * H, W=2 * W, C=cin)
            elif q.upconv_halo_ok(N, H, W, cin):
                h = ex(prefix, "up_halo", (h,), N=N, H=H, W=W, C=cin)
            else:
                h = ex(prefix, "up_gather", (h,), N=N, H=H, W=W, C=cin)
            H, W = 2 * H, 2 * W
        hst = None
    return h


def expected_stages(model, N, H, W, query=None):
    """the (prefix, op) list one traced pass of `model` over N inputs of H x W (frames / latents) must record"""
    if query is None:
        import sfv_amd
        query = sfv_amd._lib.query
    stages = []

    def ex(prefix, op, ins, **g):
        stages.append((prefix, op))
        return (None, None) if op in TWO else None
    walk(model, query, N, H, W, ex)
    return stages


# the defects inject() knows
WIRING_DEFECTS = ("dropped_skip", "skip_from_h1", "norm2_with_norm1_statistics", "statistics_2_percent",
                  "pad_top_left", "q_k_exchanged", "quant_reads_unpadded") + UP_DEFECTS


def _launch(rec, P, M, by_key, defect=None):
    """what the launch of rec = (prefix, op, inputs, None, geometry) stores under the storage model / exact form (M),
    optionally as the named defect makes it: the recorded inputs stay what ldm.py passes -> list of outputs"""
    prefix, op, ins, _, g = rec
    use, opdef = ins, None
    block = prefix.rsplit(".", 1)[0]
    if defect == "dropped_skip":
        assert ins[-1] is not None
        use = ins[:-1] + (None,)
    elif defect == "skip_from_h1":
        use = ins[:-1] + (by_key[(f"{block}.conv1", op)],)
    elif defect == "statistics_2_percent":
        part = ins[1].clone().reshape(-1, 2)
        part[:, 1] /= 1.02 ** 2                           # every M2 low by 4 %: rstd high by 2 %
        use = (ins[0], part.reshape(-1))
    elif defect == "quant_reads_unpadded":
        x = ins[0]
        bad = torch.zeros_like(x)
        bad[:, :g["cin"]] = x.reshape(-1)[:x.shape[0] * g["cin"]].reshape(x.shape[0], g["cin"])      # lda = cin
        use = (bad, None)
    elif defect not in (None, "norm2_with_norm1_statistics") and not (defect == "q_k_exchanged" and op == "conv1"):
        opdef = defect
    r = evaluate((prefix, op, use, None, g), P, M, opdef)
    outs = r.model if M.exact else [o.float() if st else o.to(M.tdt) for o, st in zip(r.model, r.stat)]
    if defect == "norm2_with_norm1_statistics":
        outs = list(by_key[(f"{block}.norm1", op)])
    elif defect == "q_k_exchanged" and op == "conv1":
        C = g["cin"]
        outs = [torch.cat([outs[0][:, C:2 * C], outs[0][:, :C], outs[0][:, 2 * C:]], 1)]
    return outs


def _key_out(op, out):
    return out[0] if op in ("conv3_halo", "conv_in") else out


def run(model, P, x0, kind="model", query=None):
    """The storage model (kind "model": outputs in the storage type / f32 statistics, as the device leaves them) or the
    exact form (kind "exact": float64, no rounding) along walk() -> (records, last output)."""
    if query is None:
        import sfv_amd
        query = sfv_amd._lib.query
    tdt = F32 if model.compute_dtype == "f32" else BF
    M = Mode(tdt, "exact" if kind == "exact" else "both")
    records, by_key = [], {}
    x0 = x0.double() if kind == "exact" else x0.float()

    def ex(prefix, op, ins, **g):
        outs = _launch((prefix, op, ins, None, g), P, M, by_key)
        out = tuple(outs) if op in TWO else outs[0]
        by_key[(prefix, op)] = _key_out(op, out)
        records.append((prefix, op, ins, out, g))
        return out

    N, _, H, W = x0.shape
    last = walk(model, query, N, H, W, ex, x0)
    return records, last


def inject(records, P, tdt, defect, at):
    """(index, record) of the first record (prefix, op) = at of a storage-model trace, its output replaced by what the
    named defect would have stored.  The records before it are untouched: they pass or fail as they did."""
    by_key = {(r[0], r[1]): _key_out(r[1], r[3]) for r in records}
    i = next(i for i, r in enumerate(records) if (r[0], r[1]) == tuple(at))
    prefix, op, ins, _, g = records[i]
    outs = _launch(records[i], P, Mode(tdt, "both"), by_key, defect)
    return i, (prefix, op, ins, tuple(outs) if op in TWO else outs[0], g)


# ---- the gates ---------------------------------------------------------------------------------------------------------

def check_record(rec, P, tdt):
    """gates (a) and (b) on one record -> dict(worst = |err| / bound, l2 = relative L2 of the stored output against the
    reference, floor = the storage model's; None where gate (b) does not apply).  Raises AssertionError outside a gate."""
    prefix, op, ins, stored, g = rec
    M = Mode(tdt, "both")
    r = evaluate(rec, P, M)
    got = list(stored) if isinstance(stored, (tuple, list)) else [stored]
    worst = r.chk(got)
    out = dict(worst=worst, l2=None, floor=None)
    if tdt == BF and op in L2_OPS:
        cols = r.cols if r.cols is not None else r.ref[0].shape[-1]
        ref, mod = r.ref[0][..., :cols], r.model[0][..., :cols]
        gg = got[0].detach().cpu().double().reshape(r.ref[0].shape)[..., :cols]
        nr = float(ref.norm())
        out["l2"], out["floor"] = float((gg - ref).norm()) / nr, float((mod - ref).norm()) / nr
        assert out["l2"] <= 2 * out["floor"], (f"{prefix} {op}: relative L2 {out['l2']:.3g} above twice the storage model's "
                                               f"{out['floor']:.3g} (|err|/bound {worst:.3g})")
    return out


def storage_ptr(t):
    return t.untyped_storage().data_ptr()


def check_chain(records, sources, last):
    """every input of a record lives in the storage of an earlier record's output (or of a source: the frame / latent);
    the last record's output is `last`"""
    seen = {storage_ptr(t) for t in sources}
    for prefix, op, ins, out, g in records:
        for t in ins:
            if t is not None:
                assert storage_ptr(t) in seen, f"{prefix} {op}: an input that no earlier record stored"
        for t in (out if isinstance(out, (tuple, list)) else (out,)):
            seen.add(storage_ptr(t))
    out = records[-1][3]
    assert out.data_ptr() == last.data_ptr() and out.shape == last.shape, "the last record is not what the pass returned"
