"""Cases, restated dispatch, float64 references, error models, f32 emulations and named defects for the frozen LDM
encoder's own kernels: csrc/attn.hip (rbvae_attention) and csrc/ldm.hip (GroupNorm, row softmax, transpose, posterior
sample), plus gn_affine_k of csrc/conv_halo.hip.  torch only; importable without a GPU.  u = 2^-24 (f32 unit roundoff),
u8 = 2^-8 (bf16), c_acc from tests/_bounds.py.

ATTENTION (attn_flash_k<D, 64>, attn_flash_db_k: the same arithmetic).  Per image, float64 from the bf16 operands:
s = q k^T scale, w = softmax(s), o = w v, D[i][c] = sum_j w_ij |v_jc - o_ic|, S[i][c] = sum_j w_ij |v_jc|,
Sqk[i][j] = scale sum_c |q_ic| |k_jc|.  The kernel divides by the sum of the SAME bf16-rounded probabilities it multiplies
with (`rs` is taken from bf16_to_f32(p0) + bf16_to_f32(p1)), so a relative perturbation e_ij of the weights moves the output
by sum_j w_ij e_ij (v_j - o_i) / (1 + sum_j w_ij e_ij): bounded with D, not S.

    |got - ref| <= (1 + u8) [ eta_i / (1 - eta_i) D + c_pv S ] + u8 |ref| + tiny

    eta_i = u8                                        p0 / p1 = f32_to_bf16(exp2f(..)): round to nearest, 8 bits
          + max_j ( c_acc(C) Sqk_ij                   sc[h]: C products accumulated in f32 by D / 32 chained MFMAs
                    + 3 u |s_ij| )                    t = sc * scale_log2e: the literal 1.4426950408889634f, the product
                                                      scale * that (launch_attn_*) and the product with sc, one rounding
                                                      each, relative to |t|; in natural-log units that is 3 u |s_ij|
          + (92 + 2 nt) u                             nt = hw / 32 key tiles.  The weight of key j of tile a is
                                                      exp2f(t - m_a) prod_{b > a} alpha_b, alpha_b = exp2f(m_{b-1} - m_b).
                                                      The subtractions round by u |t - m_a| and u (m_b - m_{b-1}) in
                                                      log2 units; the distances telescope to m_final - t <= 126 for any
                                                      weight that is a normal f32 (smaller ones are inside `tiny`):
                                                      126 ln 2 u < 88 u.  exp2f is 1 ulp = 2 u: once for p, once per
                                                      alpha (2 + 2 nt) u; 2 u spare for the flush of p below 2^-126.
    c_pv  = c_acc(hw) + (hw / 32 + 8) 2^-23           o: hw products accumulated by MFMAs (c_acc(hw)) and one rounding
                                                      per tile in o[c][r] *= alpha[r]; lrun = fma(lrun, alpha, rs): one
                                                      per tile: 2 nt u = (hw / 32) 2^-23.  The 8 * 2^-23 = 16 u: rs (one
                                                      add and four shuffle levels), inv = 1 / lrun, o * inv, and slack
                                                      for an unfused lrun update.
eta / (1 - eta) is first order in the score term (exp(x) - 1 <= x / (1 - x)).  Data kinds: see at_data.

GROUPNORM.  float64 from the storage-rounded x: mean, M2 = sum (x - mean)^2, var = M2 / n, rstd = (var + eps)^-1/2 per
(image, group), n = HW cg; t = (x - mean) rstd gamma + beta; y = t sigmoid(t) when swish.
  mean, M2: tile_stats_bounds(n, cg, sum |x|, max |x|, M2, h) with the height h of the kernels that ran (gn_height):
    tiled    GN_PASSES = 8 values per thread, rl_n = 256 / (C / V) row lanes and cg channels summed one after another in
             group_reduce, the division by rows_b cg; gn_finish_k: the product n_b mean_b, ceil(nb / 64) terms per lane
             (stride-64 loop), wave_sum's 6 levels, the division: h = 8 + rl_n + cg + ceil(nb / 64) + 9.  Two merge levels
             (block, image) <= the 4 of tile_stats_bounds.
    fallback gn_stats_k: ceil(n / 256) terms per thread (stride-256 loop), wave_sum's 6 levels, block_sum's 4 waves, the
             division: h = ceil(n / 256) + 12.  Its second pass sums (x - m)^2 about the computed m: M2 + n (m - mean)^2,
             inside the same bound (n E^2).
  rstd: b_var = b_M2 / n + u var (the division); with v = var + eps, |d rstd| <= (v - b_var)^-1/2 - v^-1/2 (first order
    rstd b_var / (2 v), and the second-order term exactly) + 4 u rstd (the addition of eps and rsqrtf, 1 ulp + spare).
  t: |dt| <= rstd |gamma| b_mean + |x - mean| |gamma| b_rstd + 4 u ((|x| + |mean|) rstd |gamma| + |beta|): sc = rs ga,
    mu sc, be - mu sc and the fma of gn_apply_vec_k, which cancels under a common offset, hence |x| + |mean|; the other
    forms round (x - mean), * rstd, * gamma, + beta: four roundings of smaller values.
  y: swish is 1.1-Lipschitz (max swish' = 1.0998); its evaluation costs c_eval |y| (staged_u_in(f32, swish, max |t|) of
    _bounds.py: covers expf / division and the hardware exp2 / rcp form of the bf16 kernel); then the output rounding:
    |dy| <= (1 + u_out) (1.1 |dt| + c_eval |y|) + u_out |y| + tiny.  Without swish: Lipschitz 1, c_eval = u.
  rbvae_groupnorm_apply: the reference takes the GIVEN f32 mean / rstd, b_mean = b_rstd = 0.
  rbvae_gn_affine: scale = rstd gamma: u |scale|; shift = beta - mean scale: 3 u (|beta| + |mean scale|) (three roundings).

SOFTMAX ROWS (softmax_rows_k).  p = exp(x - max) / sum: the maximum is exact; x - mx rounds by u |x - mx|, a relative
error of p; expf 1 ulp = 2 u; each term of the sum carries the same two errors, weighted by p_j: sum_j p_j |x_j - mx| =
H(p) - ln Z <= ln n, and 2 u; the sum itself ceil(n / 64) - 1 additions per lane and wave_sum's 6 levels; 1 / s and the
product one each: c = 2 + 2 + ln n + ceil(n / 64) + 5 + 2 = 11 + ln n + ceil(n / 64).
    |got - p| <= (1 + u_out) (c + |x - max|) u p + u_out p + tiny      (entries below 2^-100 sit inside tiny)

POSTERIOR SAMPLE (posterior_sample_k).  latent = scale (mean + exp(0.5 clamp(lv, -30, 20)) eps): 0.5 lv is exact; expf
1 ulp = 2 u, plus |0.5 lv| u for an exp2-based evaluation whose argument product rounds; the product with eps, the sum
and the product with scale one rounding each:
    |got - ref| <= u |scale| ((4 + |0.5 lv|) |e eps| + |mean|) + u |ref| + tiny

TRANSPOSE: bit equality."""
import functools
import math

import torch

import _bounds as B

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
TDT = {"f32": F32, "bf16": BF}
DT = {"f32": 0, "bf16": 1}
U32, U8, TINY = B.U32, 2.0 ** -8, B.TINY
cdiv = lambda a, b: -(-a // b)
by_id = lambda cases, i: next(c for c in cases if c["id"] == i)


def check_bound(got, ref, bnd, what, per_image=None):
    """Assert |got - ref| <= bnd element-wise ([rows][cols] or flat); returns the worst |err| / bound."""
    got = got.detach().cpu().double().reshape(ref.shape)
    err = (got - ref).abs()
    ratio = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err / bnd)
    bad = ~(err <= bnd)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if bool(bad.any()):
        flat = int(torch.argmax(ratio.reshape(-1)))
        ncol = ref.shape[-1] if ref.dim() > 1 else 1
        r, c = divmod(flat, ncol)
        where = f"(row {r}, col {c})"
        if per_image:
            where += f" = (image {r // per_image}, row {r % per_image}, channel {c})"
        raise AssertionError(f"{what} worst: {int(bad.sum())} of {bad.numel()} elements outside the bound; worst |err|/bound"
                             f" = {worst:.3g} at {where}: got {got.reshape(-1)[flat].item()!r}, ref "
                             f"{ref.reshape(-1)[flat].item()!r}, bound {bnd.reshape(-1)[flat].item():.3g}")
    return worst


# ---- attention -------------------------------------------------------------------------------------------------------

AT_BK = 32


def attn_ok(dtype, hw, C):
    return int(dtype == 1 and hw > 0 and hw % AT_BK == 0 and C in (64, 128, 256, 512))


def attn_form(C, hw):
    """The kernel rbvae_attention launches (the query tile is 64 rows: launch_attn's bq)."""
    assert attn_ok(1, hw, C)
    return "attn_flash_db_k" if C == 512 and hw >= 4 * AT_BK else f"attn_flash_k<{C},64>"


AT_REACHABLE = {f"attn_flash_k<{C},64>" for C in (64, 128, 256, 512)} | {"attn_flash_db_k"}
AT_KINDS = ("random", "peaked", "rising", "falling", "uniform", "huge")


def _at_cases():
    small = {32: ("uniform", "peaked", "huge"), 64: ("random", "rising", "falling"), 96: ("peaked", "uniform", "rising"),
             160: ("random", "falling", "huge", "peaked")}
    table = [(C, hw, kinds) for C in (64, 128, 256) for hw, kinds in small.items()]
    table += [(512, 32, ("uniform", "peaked", "random")), (512, 96, ("rising", "falling", "huge", "peaked")),
              (512, 128, AT_KINDS), (512, 160, ("peaked", "rising", "uniform")), (512, 192, ("random", "falling", "huge")),
              (512, 1024, ("rising", "peaked"))]
    cases, i = [], 0
    for C, hw, kinds in table:
        for kind in kinds:
            N = 1 if hw == 1024 else 2 if kind == "uniform" else 1 + i % 3
            layout = "fused" if i % 2 == 0 else "split"
            pad = 8 if (i // 2) % 2 == 0 else 0
            cases.append(dict(id=f"c{C}_hw{hw}_n{N}_{kind}_{layout}_ldo{pad}", C=C, hw=hw, N=N, kind=kind, layout=layout,
                              ldo=C + pad, seed=1000 + i))
            i += 1
    return cases


AT_CASES = _at_cases()


def peaked_perm(hw):
    """Row i -> the key that takes nearly all of its weight: tile edges first (keys 0, 31, 32, 63, hw - 32, hw - 1), the
    last row to key 31, every other row by a stride coprime with hw."""
    perm = [(5 * i + 3) % hw for i in range(hw)]
    for i, key in enumerate((0, 31, 32, 63, hw - 32, hw - 1)):
        perm[i % hw] = key % hw
    perm[hw - 1] = 31
    return torch.tensor(perm)


def at_data(c):
    """q, k, v [N][hw][C] as bf16 (every image its own K and V).
    random   sd 1.5: every softmax row spread over many keys
    peaked   q_i = 6 k_perm(i): one key per row carries the weight (a dropped or displaced key moves the whole output)
    rising   the score grows with the key index: the maximum moves in every tile, the rescale runs every step
    falling  the maximum never moves after the first tile: the __any(moved) branch is skipped
    uniform  q = 0, v = 3 + image + z: the output is the mean over all keys of the image's own V
    huge     q, k times 16: one-hot weights, alpha underflows to 0"""
    N, hw, C, kind = c["N"], c["hw"], c["C"], c["kind"]
    g = torch.Generator().manual_seed(c["seed"])
    rn = lambda *s: torch.randn(*s, generator=g)
    q, k, v = rn(N, hw, C) * 1.5, rn(N, hw, C) * 1.5, rn(N, hw, C) * 1.5
    if kind == "peaked":
        k = rn(N, hw, C)
        q = 6.0 * k.bfloat16().float()[:, peaked_perm(hw)]
    elif kind in ("rising", "falling"):
        j = torch.arange(hw, dtype=torch.float32) / hw
        ramp = j if kind == "rising" else 1.0 - j
        k = ramp[None, :, None] * (20.0 / math.sqrt(C)) + 0.02 * rn(N, hw, C)
        q = (0.5 + torch.rand(N, hw, 1, generator=g)).expand(N, hw, C).contiguous()
    elif kind == "uniform":
        q = torch.zeros(N, hw, C)
        v = v + 3.0 + torch.arange(N, dtype=torch.float32)[:, None, None]
    elif kind == "huge":
        q, k = q * 16.0, k * 16.0
    return dict(q=q.bfloat16(), k=k.bfloat16(), v=v.bfloat16(), scale=float(int(C) ** (-0.5)))


def at_eta_tail(hw):
    return (92 + 2 * (hw // AT_BK)) * U32


def at_c_pv(hw):
    return B.c_acc(hw) + (hw / 32 + 8) * 2.0 ** -23


def at_reference(c, d):
    """float64 (ref, bound) [N * hw][C] of the case."""
    return at_bounds(d["q"], d["k"], d["v"], d["scale"])


def at_bounds(Q, K, V, scale):
    """float64 (ref, bound) [N * hw][C] of bf16 operands q, k, v [N][hw][C]."""
    N, hw, C = Q.shape
    refs, bnds = [], []
    for n in range(N):
        q, k, v = Q[n].double(), K[n].double(), V[n].double()
        s = q @ k.t() * scale
        w = torch.softmax(s, dim=1)
        o = w @ v
        S = w @ v.abs()
        Sqk = q.abs() @ k.abs().t() * scale
        eta = U8 + (B.c_acc(C) * Sqk + 3 * U32 * s.abs()).max(1).values + at_eta_tail(hw)
        D = torch.empty_like(o)
        step = max(1, (1 << 24) // (hw * C))
        for r0 in range(0, hw, step):
            dev = (v[None, :, :] - o[r0:r0 + step, None, :]).abs()
            D[r0:r0 + step] = torch.einsum("ij,ijc->ic", w[r0:r0 + step], dev)
        bnd = (1 + U8) * ((eta / (1 - eta))[:, None] * D + at_c_pv(hw) * S) + U8 * o.abs() + TINY
        refs.append(o)
        bnds.append(bnd)
    return torch.cat(refs), torch.cat(bnds)


@functools.lru_cache(maxsize=None)
def at_case(cid):
    """(data, ref, bound) of a case, computed once and shared."""
    c = by_id(AT_CASES, cid)
    d = at_data(c)
    ref, bnd = at_reference(c, d)
    return d, ref, bnd


AT_DEFECTS = ("skip_last_tile", "key31_zero", "v_rot", "no_log2e", "alpha1_second", "image0_keys")


def at_forward(c, d, dtype, defect=None):
    """The kernels' algorithm (32-key tiles, running maximum, exp2 with the scale folded in, probabilities rounded to bf16,
    sums and rescaling in `dtype`) -> [N * hw][C].  dtype = f32 emulates the kernel (torch's matmul order, not the MFMA's);
    float64 is the same algorithm in exact arithmetic: no rounding of p and of the output."""
    N, hw = c["N"], c["hw"]
    f32 = dtype == F32
    sl2 = d["scale"] if defect == "no_log2e" else (float(torch.tensor(d["scale"], dtype=F32) * torch.tensor(1.4426950408889634, dtype=F32))
                                                   if f32 else d["scale"] * 1.4426950408889634)
    outs = []
    for n in range(N):
        src = 0 if defect == "image0_keys" else n
        q, k, v = d["q"][n].to(dtype), d["k"][src].to(dtype), d["v"][src].to(dtype)
        m = torch.full((hw,), -float("inf"), dtype=dtype)
        l = torch.zeros(hw, dtype=dtype)
        o = torch.zeros(hw, c["C"], dtype=dtype)
        last = hw - AT_BK if defect == "skip_last_tile" and hw > AT_BK else hw
        for ti, k0 in enumerate(range(0, last, AT_BK)):
            kt, vt = k[k0:k0 + AT_BK], v[k0:k0 + AT_BK]
            if defect == "v_rot":
                vt = vt.roll(1, 0)
            t = (q @ kt.t()) * sl2
            mnew = torch.maximum(m, t.max(1).values)
            alpha = torch.exp2(m - mnew)
            if defect == "alpha1_second" and ti == 1:
                alpha = torch.ones_like(alpha)
            p = torch.exp2(t - mnew[:, None])
            if f32:
                p = p.bfloat16().to(dtype)
            if defect == "key31_zero":
                p[:, 31] = 0
            l = l * alpha + p.sum(1)
            o = o * alpha[:, None] + p @ vt
            m = mnew
        out = o * (1.0 / l)[:, None]
        outs.append(out.bfloat16().double() if f32 else out.double())
    return torch.cat(outs)


def at_check(c, got, what=None):
    _, ref, bnd = at_case(c["id"])
    return check_bound(got, ref, bnd, what or c["id"], per_image=c["hw"])


# ---- GroupNorm -------------------------------------------------------------------------------------------------------

GN_PASSES = 8
GN_V = {"f32": 4, "bf16": 8}
GN_EPS = 1e-6


def gn_tiled_ok(dtype, C, ldx, ldy, groups):
    V = GN_V[dtype]
    if C % V or groups > 64 or C % groups:
        return False
    tpr = C // V
    return tpr <= 256 and 256 % tpr == 0 and ldx % V == 0 and ldy % V == 0


def gn_rows_per_block(dtype, C):
    return (256 // (C // GN_V[dtype])) * GN_PASSES


def gn_ws_floats(dtype, N, HW, C, groups):
    n = 2 * N * groups
    if gn_tiled_ok(dtype, C, C, C, groups):
        n += 2 * N * cdiv(HW, gn_rows_per_block(dtype, C)) * groups + 4
    return n


def gn_vec_index_ok(dtype, rows, C):
    return rows * (C // GN_V[dtype]) <= (1 << 32) - (1 << 22)


def gn_route(c):
    """(statistics kernels, apply kernel, cause of a fallback) of a case: the three gates of csrc/ldm.hip.
    entry swish_ws / swish: gn_tiled_ok(ldx, ldy) && workspace && index range && x | y | gamma | beta 16-byte aligned;
    entry stats: gn_tiled_ok(ldx, ldx) && workspace && x aligned; entry apply: as swish_ws without the workspace."""
    dt, N, HW, C, G = c["dtype"], c["N"], c["HW"], c["C"], c["groups"]
    V = GN_V[dt]
    ws = {"full": gn_ws_floats(dt, N, HW, C, G), "stats_only": 2 * N * G}[c["ws"]] if c["entry"] != "swish" else 2 * N * G
    aligned = not c["misalign"]
    cause = None
    if C % V:
        cause = "C % V"
    elif C // V > 256 or 256 % (C // V):
        cause = "256 % (C / V)"
    elif c["ldx"] % V or (c["entry"] != "stats" and c["ldy"] % V):
        cause = "ld % V"
    elif not gn_tiled_ok(dt, C, c["ldx"], c["ldx"] if c["entry"] == "stats" else c["ldy"], G):
        cause = "groups"
    elif c["entry"] != "apply" and ws < gn_ws_floats(dt, N, HW, C, G):
        cause = "swish entry" if c["entry"] == "swish" else "workspace"
    elif not gn_vec_index_ok(dt, N * HW, C) and c["entry"] != "stats":
        cause = "index"
    elif not aligned:
        cause = f"{c['misalign']} alignment"
    tiled = cause is None
    stats = None if c["entry"] == "apply" else ("gn_partial_k+gn_finish_k" if tiled else "gn_stats_k")
    if c["entry"] == "stats":
        apply = None
    elif tiled:
        apply = "gn_apply_vec_k:cg4" if (C // G) % 4 == 0 else "gn_apply_vec_k:cg_odd"
    else:
        apply = "gn_apply_k"
    return stats, apply, cause


def gn_height(c):
    return gn_height_of(c["dtype"], c["HW"], c["C"], c["groups"], gn_route(c)[0] != "gn_stats_k")


def gn_height_of(dtype, HW, C, groups, tiled):
    """summation height of the statistics kernels of a shape: gn_partial_k + gn_finish_k (tiled) or gn_stats_k"""
    cg, n = C // groups, HW * (C // groups)
    if not tiled:
        return cdiv(n, 256) + 12
    rl_n = 256 // (C // GN_V[dtype])
    return GN_PASSES + rl_n + cg + cdiv(cdiv(HW, gn_rows_per_block(dtype, C)), 64) + 9


def _gn(id, dtype, C, groups, N, HW, kind, swish=1, padx=0, pady=0, entry="swish_ws", ws="full", misalign=None):
    return dict(id=id, dtype=dtype, C=C, groups=groups, N=N, HW=HW, kind=kind, swish=swish, ldx=C + padx, ldy=C + pady,
                entry=entry, ws=ws, misalign=misalign)


# rb = gn_rows_per_block: f32 C=256 and bf16 C=512 have rb = 32; HW in {1, rb - 1, rb, rb + 1, 3 rb + 5}
GN_CASES = [
    _gn("t_f32_c256_hw1", "f32", 256, 32, 1, 1, "offset"),
    _gn("t_f32_c256_hw31_ramp", "f32", 256, 32, 3, 31, "ramp"),
    _gn("t_f32_c256_hw32_far", "f32", 256, 32, 1, 32, "far", swish=0),
    _gn("t_f32_c256_hw33_outlier_ld", "f32", 256, 32, 3, 33, "outlier", padx=4, pady=8),
    _gn("t_f32_c256_hw101_far", "f32", 256, 32, 3, 101, "far"),
    _gn("t_f32_c256_hw101_ramp", "f32", 256, 32, 3, 101, "ramp", swish=0),
    _gn("t_f32_c256_hw40_const", "f32", 256, 32, 1, 40, "const"),
    _gn("t_bf16_c512_hw1", "bf16", 512, 32, 3, 1, "offset"),
    _gn("t_bf16_c512_hw31_const", "bf16", 512, 32, 1, 31, "const"),
    _gn("t_bf16_c512_hw32_ramp", "bf16", 512, 32, 3, 32, "ramp", swish=0),
    _gn("t_bf16_c512_hw33_outlier_ld", "bf16", 512, 32, 1, 33, "outlier", padx=8, pady=16),
    _gn("t_bf16_c512_hw101_ramp", "bf16", 512, 32, 3, 101, "ramp"),
    _gn("t_f32_c64_cg2_hw129_ramp", "f32", 64, 32, 3, 129, "ramp"),
    _gn("t_bf16_c64_cg2_hw257_offset", "bf16", 64, 32, 3, 257, "offset"),
    _gn("t_f32_c1024_hw515_ramp_65blocks", "f32", 1024, 32, 1, 8 * 64 + 3, "ramp"),
    _gn("t_f32_c8_g1_hw50", "f32", 8, 1, 3, 50, "offset"),
    _gn("t_bf16_c32_g4_hw600_ramp", "bf16", 32, 4, 1, 600, "ramp"),
    _gn("t_bf16_c256_g64_hw70_outlier", "bf16", 256, 64, 3, 70, "outlier"),
    _gn("f_f32_c36_hw50_offset", "f32", 36, 4, 3, 50, "offset"),
    _gn("f_bf16_c36_hw50_outlier", "bf16", 36, 4, 1, 50, "outlier"),
    _gn("f_bf16_c96_hw40_ramp", "bf16", 96, 32, 3, 40, "ramp"),
    _gn("f_f32_c384_hw20_far", "f32", 384, 32, 1, 20, "far"),
    _gn("f_f32_c128_ldx_plus2", "f32", 128, 32, 3, 70, "ramp", padx=2),
    _gn("f_bf16_c128_ldy_plus4", "bf16", 128, 32, 1, 70, "offset", pady=4),
    _gn("f_bf16_c128_x_misaligned", "bf16", 128, 32, 3, 70, "ramp", padx=8, misalign="x"),
    _gn("f_f32_c128_gamma_misaligned", "f32", 128, 32, 1, 70, "outlier", misalign="gamma"),
    _gn("f_bf16_c256_ws_stats_only", "bf16", 256, 32, 3, 70, "ramp", ws="stats_only"),
    _gn("f_f32_c256_swish_entry", "f32", 256, 32, 3, 70, "ramp", entry="swish"),
    _gn("f_bf16_c512_swish_entry_const", "bf16", 512, 32, 1, 33, "const", entry="swish", swish=0),
    _gn("s_f32_c256_hw101_ramp", "f32", 256, 32, 3, 101, "ramp", entry="stats"),
    _gn("s_bf16_c128_hw300_offset_ld", "bf16", 128, 32, 3, 300, "offset", entry="stats", padx=8),
    _gn("s_f32_c36_hw50_far", "f32", 36, 4, 1, 50, "far", entry="stats"),
    _gn("s_bf16_c256_ws_stats_only", "bf16", 256, 32, 3, 70, "outlier", entry="stats", ws="stats_only"),
    _gn("s_f32_c128_x_misaligned", "f32", 128, 32, 1, 70, "ramp", entry="stats", padx=4, misalign="x"),
    _gn("a_f32_c256_hw33", "f32", 256, 32, 3, 33, "offset", entry="apply", pady=4),
    _gn("a_bf16_c64_cg2_hw40", "bf16", 64, 32, 3, 40, "ramp", entry="apply", padx=8),
    _gn("a_bf16_c96_hw40", "bf16", 96, 32, 1, 40, "offset", entry="apply", swish=0),
    # the grid-stride loops make a second trip: rows * C > 8192 * 256, rows * C / V > 16384 * 256
    _gn("a_f32_c36_second_trip", "f32", 36, 4, 2, 30000, "offset", entry="apply"),
    _gn("a_f32_c4_second_trip", "f32", 4, 1, 2, 2150000, "offset", entry="apply"),
]
GN_ROUTES = {("gn_partial_k+gn_finish_k", "gn_apply_vec_k:cg4"), ("gn_partial_k+gn_finish_k", "gn_apply_vec_k:cg_odd"),
             ("gn_stats_k", "gn_apply_k"), ("gn_partial_k+gn_finish_k", None), ("gn_stats_k", None),
             (None, "gn_apply_vec_k:cg4"), (None, "gn_apply_vec_k:cg_odd"), (None, "gn_apply_k")}
GN_CAUSES = {"C % V", "256 % (C / V)", "ld % V", "x alignment", "gamma alignment", "workspace", "swish entry"}


def gn_data(c):
    """x [N][HW][C] in the storage type, gamma, beta (f32) and, for entry apply, given mean / rstd [N * groups] (f32,
    deliberately not x's own).
    offset   3 + 0.5 z
    far      100 + 0.01 z (f32: a one-pass variance cancels; in bf16 it would round to a constant)
    ramp     4 p / HW + 2 image + 0.1 z: the block means differ (the merge term dominates), the images differ
    const    2.5: var = 0, rstd = 1000
    outlier  0.1 z with one element of 200 per image"""
    N, HW, C, kind = c["N"], c["HW"], c["C"], c["kind"]
    g = torch.Generator().manual_seed(sum(map(ord, c["id"])))
    if N * HW * C > (1 << 22):      # a large case: a tiled pattern, not 34 M fresh normals
        base = torch.randn(4096, C, generator=g)
        z = base.repeat(cdiv(N * HW, 4096), 1)[:N * HW].reshape(N, HW, C)
    else:
        z = torch.randn(N, HW, C, generator=g)
    if kind == "offset":
        x = 3.0 + 0.5 * z
    elif kind == "far":
        assert c["dtype"] == "f32"
        x = 100.0 + 0.01 * z
    elif kind == "ramp":
        x = 4.0 * torch.arange(HW, dtype=F32)[None, :, None] / HW + 2.0 * torch.arange(N, dtype=F32)[:, None, None] + 0.1 * z
    elif kind == "const":
        x = torch.full((N, HW, C), 2.5)
    else:
        x = 0.1 * z
        x[:, 5 % HW, 3 % C] = 200.0
    d = dict(x=x.to(TDT[c["dtype"]]), gamma=torch.randn(C, generator=g), beta=torch.randn(C, generator=g))
    if c["entry"] == "apply":
        G = c["groups"]
        xg = d["x"].double().reshape(N, HW, G, C // G)
        mean, var = xg.mean((1, 3)), xg.var((1, 3), unbiased=False)
        d["mean"] = (mean + 0.1 * torch.randn(N, G, generator=g)).float().reshape(-1)
        d["rstd"] = ((var + GN_EPS).rsqrt() * (1 + 0.1 * torch.rand(N, G, generator=g))).float().reshape(-1)
    return d


def gn_reference(c, d):
    """float64 references and bounds: dict(mean, rstd [N * G], y [N * HW][C]) -> (ref, bound) each (what the entry leaves)."""
    given = (d["mean"], d["rstd"]) if c["entry"] == "apply" else None
    out = gn_bounds(d["x"], d["gamma"], d["beta"], c["groups"], TDT[c["dtype"]], c["swish"],
                    h=None if given else gn_height(c), given=given)
    if c["entry"] == "stats":
        out.pop("y")
    return out


def gn_bounds(x, gamma, beta, G, out_dtype, swish, h=None, given=None):
    """gn_reference for any operands: x [N][HW][C] as stored, the statistics kernels' summation height h, or
    given = (mean, rstd) [N * G] f32 for the apply pass from given statistics."""
    N, HW, C = x.shape
    cg, n = C // G, HW * (C // G)
    xg = x.double().reshape(N, HW, G, cg)
    out = {}
    if given is not None:
        mean, rstd = given[0].double().reshape(N, G), given[1].double().reshape(N, G)
        b_mean = b_rstd = torch.zeros(N, G, dtype=F64)
    else:
        mean = xg.mean((1, 3))
        M2 = ((xg - mean[:, None, :, None]) ** 2).sum((1, 3))
        var = M2 / n
        v = var + GN_EPS
        rstd = v.rsqrt()
        b_mean, b_M2, _ = B.tile_stats_bounds(n, cg, xg.abs().sum((1, 3)), xg.abs().amax((1, 3)), M2, h=h)
        b_var = b_M2 / n + U32 * var
        lo = v - b_var
        b_rstd = torch.where(lo > 0, lo.clamp_min(1e-300).rsqrt() - rstd, torch.full_like(v, float("inf"))) + 4 * U32 * rstd
        out["mean"] = (mean.reshape(-1), b_mean.reshape(-1))
        out["rstd"] = (rstd.reshape(-1), b_rstd.reshape(-1))
    e = lambda s: s[:, None, :, None]
    ga, be = gamma.double().reshape(1, 1, G, cg), beta.double().reshape(1, 1, G, cg)
    t = (xg - e(mean)) * e(rstd) * ga + be
    b_t = e(rstd) * ga.abs() * e(b_mean) + (xg - e(mean)).abs() * ga.abs() * e(b_rstd) \
        + 4 * U32 * ((xg.abs() + e(mean).abs()) * e(rstd) * ga.abs() + be.abs())
    tmax = float(t.abs().max())
    c_eval = B.staged_u_in(F32, bool(swish), tmax)
    y = t * torch.sigmoid(t) if swish else t
    u_out = B.U_OUT[out_dtype]
    b_y = (1 + u_out) * ((1.1 if swish else 1.0) * b_t + c_eval * y.abs()) + u_out * y.abs() + TINY
    out["y"] = (y.reshape(N * HW, C), b_y.reshape(N * HW, C))
    return out


@functools.lru_cache(maxsize=None)
def gn_case(cid):
    c = by_id(GN_CASES, cid)
    d = gn_data(c)
    return d, gn_reference(c, d)


GN_DEFECTS = ("no_merge_term", "short_block_full", "one_pass")


def gn_forward(c, d, dtype, defect=None):
    """The kernels' algorithm in `dtype` (f32: an emulation with torch's summation order; float64: exact arithmetic, no
    output rounding) -> dict(mean, rstd, y) as far as the entry leaves them.  Tiled statistics: per block of rb rows the
    mean and the M2 about it, merged by gn_finish_k's parallel-variance formula; fallback: two passes."""
    N, HW, C, G = c["N"], c["HW"], c["C"], c["groups"]
    cg = C // G
    stats, apply, _ = gn_route(c)
    x = d["x"].to(dtype).reshape(N, HW, G, cg)
    out = {}
    if c["entry"] == "apply":
        mean, rstd = d["mean"].to(dtype).reshape(N, G), d["rstd"].to(dtype).reshape(N, G)
    else:
        total = float(HW * cg)
        if defect == "one_pass":
            mean = x.sum((1, 3)) / total
            var = (x * x).sum((1, 3)) / total - mean * mean
        elif stats == "gn_stats_k":
            mean = x.sum((1, 3)) / total
            var = ((x - mean[:, None, :, None]) ** 2).sum((1, 3)) / total
        else:
            rb = gn_rows_per_block(c["dtype"], C)
            nb = cdiv(HW, rb)
            cnt, mb, m2b = [], [], []
            for b in range(nb):
                xb = x[:, b * rb:(b + 1) * rb]
                m = xb.sum((1, 3)) / float(xb.shape[1] * cg)
                mb.append(m)
                m2b.append(((xb - m[:, None, :, None]) ** 2).sum((1, 3)))
                cnt.append(float((rb if defect == "short_block_full" else xb.shape[1]) * cg))
            mean = sum(n_b * m for n_b, m in zip(cnt, mb)) / total
            q = sum(m2 + (0.0 if defect == "no_merge_term" else n_b * (m - mean) ** 2) for n_b, m, m2 in zip(cnt, mb, m2b))
            var = q / total
        rstd = (var + torch.tensor(GN_EPS, dtype=dtype)).rsqrt()
        out["mean"], out["rstd"] = mean.reshape(-1), rstd.reshape(-1)
    if c["entry"] == "stats":
        return out
    e = lambda s: s[:, None, :, None]
    ga, be = d["gamma"].to(dtype).reshape(1, 1, G, cg), d["beta"].to(dtype).reshape(1, 1, G, cg)
    if apply == "gn_apply_vec_k:cg4":
        sc = e(rstd) * ga
        t = x * sc + (be - e(mean) * sc)
    else:
        t = (x - e(mean)) * e(rstd) * ga + be
    y = t * torch.sigmoid(t) if c["swish"] else t
    if dtype == F32:
        y = y.to(TDT[c["dtype"]])
    out["y"] = y.reshape(N * HW, C)
    return out


def gn_check(c, got, what=None):
    """got: dict with the keys of gn_reference's result -> the worst ratio of each."""
    _, ref = gn_case(c["id"])
    res = {}
    for key, (r, b) in ref.items():
        res[key] = check_bound(got[key], r, b, f"{what or c['id']} {key}", per_image=c["HW"] if key == "y" else None)
    return res


AF_CASES = [dict(id="n1_c64_g32", N=1, C=64, groups=32), dict(id="n3_c36_g4", N=3, C=36, groups=4),
            dict(id="n2_c512_g32", N=2, C=512, groups=32), dict(id="n3_c300_g1", N=3, C=300, groups=1)]


def af_data(c):
    g = torch.Generator().manual_seed(70 + c["C"])
    NG = c["N"] * c["groups"]
    return dict(mean=3 * torch.randn(NG, generator=g), rstd=torch.rand(NG, generator=g) * 10 + 0.01,
                gamma=torch.randn(c["C"], generator=g), beta=torch.randn(c["C"], generator=g))


def af_reference(c, d):
    N, C, G = c["N"], c["C"], c["groups"]
    ex = lambda s: s.double().reshape(N, G, 1).expand(N, G, C // G).reshape(N, C)
    ga, be = d["gamma"].double()[None], d["beta"].double()[None]
    sc = ex(d["rstd"]) * ga
    ms = ex(d["mean"]) * sc
    return dict(scale=(sc, U32 * sc.abs() + TINY), shift=(be - ms, 3 * U32 * (be.abs() + ms.abs()) + TINY))


def af_forward(c, d, dtype):
    N, C, G = c["N"], c["C"], c["groups"]
    ex = lambda s: s.to(dtype).reshape(N, G, 1).expand(N, G, C // G).reshape(N, C)
    sc = ex(d["rstd"]) * d["gamma"].to(dtype)[None]
    return dict(scale=sc, shift=d["beta"].to(dtype)[None] - ex(d["mean"]) * sc)


# ---- row softmax -----------------------------------------------------------------------------------------------------

def _sm_cases():
    cases = []
    for i, n in enumerate((1, 63, 64, 65, 200)):
        for dtype in ("f32", "bf16"):
            pad = (4 if dtype == "f32" else 8) if i % 2 == 0 else 0
            ld = cdiv(n, 8) * 8 + pad if pad or n % 8 else n
            cases.append(dict(id=f"{dtype}_n{n}_ld{ld}_{'inplace' if (i + (dtype == 'f32')) % 2 else 'out'}", dtype=dtype,
                              n=n, ld=ld, rows=(1, 7, 10, 13, 5)[i], inplace=bool((i + (dtype == "f32")) % 2)))
    return cases


SM_CASES = _sm_cases()


def sm_data(c):
    """[rows][n]: sd 3; row 1 (if any) spans more than 200 (exp underflows to 0); the last row is constant."""
    g = torch.Generator().manual_seed(90 + c["n"])
    x = torch.randn(c["rows"], c["n"], generator=g) * 3
    if c["rows"] > 1 and c["n"] > 1:
        x[1] = torch.linspace(-150.0, 90.0, c["n"])
    x[-1] = 1.25
    return x.to(TDT[c["dtype"]])


def sm_c(n):
    return 11 + math.log(n) + cdiv(n, 64)


def sm_reference(c, x):
    return sm_bounds(x, TDT[c["dtype"]])


def sm_bounds(x, out_dtype):
    """float64 (softmax, bound) of the rows of x [rows][n] as stored"""
    xd = x.double()
    p = torch.softmax(xd, dim=1)
    u_out = B.U_OUT[out_dtype]
    dist = (xd - xd.max(1, keepdim=True).values).abs()
    return p, (1 + u_out) * (sm_c(x.shape[1]) + dist) * U32 * p + u_out * p + TINY


def sm_forward(c, x, dtype):
    xd = x.to(dtype)
    e = torch.exp(xd - xd.max(1, keepdim=True).values)
    p = e * (1.0 / e.sum(1, keepdim=True))
    return p.to(TDT[c["dtype"]]) if dtype == F32 else p


# ---- transpose -------------------------------------------------------------------------------------------------------

TR_CASES = [dict(id=f"{dtype}_{R}x{C}_ldi{ldi}_ldo{ldo}", dtype=dtype, R=R, C=C, ldi=ldi, ldo=ldo)
            for dtype in ("f32", "bf16")
            for R, C, ldi, ldo in ((1, 1, 8, 8), (1, 40, 40, 8), (33, 31, 32, 40), (64, 96, 96, 64), (100, 513, 520, 104))]


def tr_bits(c):
    """[R][C] raw bit patterns (int16 / int32): random bits, hence NaNs with payloads, infinities and denormals, and
    explicit -0, +0, signalling / quiet NaN patterns and +inf in the first six entries."""
    g = torch.Generator().manual_seed(c["R"] * 1000 + c["C"])
    it = torch.int32 if c["dtype"] == "f32" else torch.int16
    lo, hi = (-2 ** 31, 2 ** 31) if c["dtype"] == "f32" else (-2 ** 15, 2 ** 15)
    bits = torch.randint(lo, hi, (c["R"], c["C"]), generator=g, dtype=torch.int64)
    special = [0x80000000 - 2 ** 32, 0, 0x7FC0BEEF, 0x7F800001, 0xFFFFFFFF - 2 ** 32, 0x7F800000] if c["dtype"] == "f32" else \
        [0x8000 - 2 ** 16, 0, 0x7FC1, 0x7F81, 0xFFFF - 2 ** 16, 0x7F80]
    flat = bits.reshape(-1)
    flat[:min(len(special), flat.numel())] = torch.tensor(special[:flat.numel()])
    return bits.to(it)


# ---- posterior sample ------------------------------------------------------------------------------------------------

PS_CASES = [dict(id=f"{dtype}_n{N}_z{Z}_hw{HW}_ld{ld}_{'eps' if eps else 'mode'}", dtype=dtype, N=N, Z=Z, HW=HW, ld=ld, eps=eps)
            for dtype, N, Z, HW, ld, eps in (("f32", 2, 4, 64, 8, True), ("f32", 3, 4, 33, 12, False), ("bf16", 2, 4, 64, 8, False),
                                             ("bf16", 3, 3, 50, 8, True), ("f32", 1, 1, 1, 4, True), ("bf16", 1, 8, 7, 24, True),
                                             ("f32", 1, 2, 40, 4, False), ("bf16", 2, 4, 20, 8, True), ("bf16", 1, 4, 9, 16, False),
                                             ("f32", 2, 4, 270000, 8, True))]       # N Z HW > 8192 * 256: a second trip


def ps_data(c):
    """moments [N * HW][2 Z] (mean | logvar) in the storage type, eps [N][Z][HW] f32.  The logvar of the first pixels
    takes the values at and beyond both clamps: -31, -30, 20, 21."""
    N, Z, HW = c["N"], c["Z"], c["HW"]
    g = torch.Generator().manual_seed(33 + HW)
    mom = torch.randn(N * HW, 2 * Z, generator=g)
    mom[:, Z:] = mom[:, Z:] * 4 - 2
    sp = torch.tensor([-31.0, -30.0, 20.0, 21.0, -29.5, 19.5])
    k = min(N * HW, 6)
    mom[:k, Z] = sp[:k]
    mom[-k:, 2 * Z - 1] = sp[:k]
    return dict(mom=mom.to(TDT[c["dtype"]]), eps=torch.randn(N, Z, HW, generator=g), scale=0.18215)


def _ps_parts(c, d, dtype):
    N, Z, HW = c["N"], c["Z"], c["HW"]
    m = d["mom"].to(dtype).reshape(N, HW, 2 * Z).permute(0, 2, 1)
    mean, lv = m[:, :Z], m[:, Z:].clamp(-30.0, 20.0)
    eps = d["eps"].to(dtype) if c["eps"] else torch.zeros(N, Z, HW, dtype=dtype)
    return mean, lv, torch.exp(0.5 * lv) * eps


def ps_reference(c, d):
    mean, lv, ee = _ps_parts(c, d, F64)
    s = float(torch.tensor(d["scale"], dtype=F32))
    ref = s * (mean + ee)
    bnd = U32 * abs(s) * ((4 + (0.5 * lv).abs()) * ee.abs() + mean.abs()) + U32 * ref.abs() + TINY
    return ref.reshape(-1), bnd.reshape(-1)


def ps_forward(c, d, dtype):
    mean, lv, ee = _ps_parts(c, d, dtype)
    return (torch.tensor(d["scale"], dtype=F32).to(dtype) * (mean + ee)).reshape(-1)
