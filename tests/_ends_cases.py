"""The kernels at the 3/4-channel ends of the two CNNs (test_ends_bounds_gpu.py / test_ends_bounds_cpu.py): case tables, a host
restatement of each dispatcher, float64 references from the operands as the kernels see them, and the error model.

  csrc/conv_first.hip   conv_first_fused_k<CIN, MODE, NQ> (rbvae_conv_first_fused, rbvae_deconv_last_dgrad_fused),
                        wgrad_first_k / wgrad_first_wide_k<CIN, MODE> (rbvae_wgrad_first)
  csrc/deconv_last.hip  deconv_last_fused_k<ONE> (rbvae_deconv_last_fused)
  csrc/conv_in.hip      conv_in_k<CIN, NQ> (rbvae_conv_in) with GroupNorm tile statistics
  csrc/layout.hip       rbvae_im2col(_frames), rbvae_col2im_sigmoid(_frames), rbvae_sigmoid_bwd_nhwc (the two-kernel path)

Every family has X_build (operands + float64 reference), X_forward (the operation restated in float64, or with
dt = float32 as an f32 emulation, optionally with one named defect) and X_check (the element-wise comparison; returns the
worst |err| / bound per output).  The GPU tests feed X_check the library's outputs, the CPU tests X_forward's.

Error model (u = 2^-24, gamma(n) = n u / (1 - n u); nothing here is fitted to what the device returns)

  Convolutions (conv_first MODE 0 / 1, conv_in): frames / dpre and weights are rounded to bf16 before the MFMA, so the
    reference uses the rounded operands and _bounds.check's bound applies as it stands: c_acc(64) S for the one 64-deep
    chain (S includes |bias|), the bf16 store 2^-8 |ref|; ReLU, the keyed dropout and the gate are exact decisions on the
    stored value.  The reference decides every element: a dropped or gated element must be stored as zero.
  Column sums of the dgrad kernel: an f32 sum of the <= 128 stored values of a block's in-image pixels (4 per lane,
    16 lanes by DPP, then the pixel groups): _bounds.colsum_bound, (n - 1) u sum |v|, any order.
  Weight-gradient slabs: bf16 products are exact in f32; a slice of P pixels is a P-long f32 accumulation: c_acc(P) S.
  deconv_last_fused: pre = bias + four taps of C1 products, each tap one f32 MFMA chain, the taps and the bias added in
    f32: d_pre = c_acc(4 C1) S_pre.  The sigmoid is rcp(1 + exp2(-log2e v)) on v_exp_f32 / v_rcp_f32: _lstm_cases.c_sig
    (constant and product rounding 2|v| u in the exponent, 1 ulp each for exp and rcp, one rounding for 1 + e; the |v|
    term stays because saturated cases are in the table).  Through the sigmoid (slope s(1 - s) <= 1/4, |s''|/2 < 0.05):
        |xr - sigmoid(pre)| <= s(1 - s) d_pre + 0.05 d_pre^2 + c_sig(pre)
  dpre = gscale * (s - t) * s * (1 - s) from the STORED s: the subtraction, three products and 1 - s round once each:
    gamma(5) |ref| + 2^-126 (a flushed denormal).
  sse parts and dpre column sums of a block: every term passes through at most h additions (h = the thread's own terms,
    six wave_sum levels, then the waves): gamma(h + 3) sum d^2 (the square's own two roundings and d's) resp.
    gamma(h) sum |dpre| -- recursive summation along a tree of height h.
  col2im_sigmoid reads Y as stored (f32 or bf16: exact in float64), so only the tap sum (<= 4 additions onto the bias:
    gamma(4) S), and the sigmoid remain.  Both of its instantiations call sigmoidf_ = 1.0f / (1.0f + expf(-x)): the
    device library's expf and a correctly rounded DIVISION, i.e. c_sig(lib=True), in f32 and in bf16 mode alike.
  im2col and the `col` rows of the fused kernels are copies (rounded to bf16 in bf16 mode): bit for bit."""
import numpy as np
import torch
import torch.nn.functional as F

import _bounds as B
from _conv_cases import DTYPE_ID, TDT, cdiv
from _halo_cases import check_tile_stats, tile_stats_ref
from _lstm_cases import LOG2E_F32, c_sig

U = B.U32
F32_MIN = 2.0 ** -126
TA, TB = 8, 16                     # pixel block of conv_first / deconv_last / conv_in


def gamma(n):
    return n * U / (1 - n * U)


def bf16r(t):
    return t.float().bfloat16()


def seed_of(c):
    return sum(map(ord, c["id"]))


def s2_out(IH, IW):
    """3 x 3, stride 2, pad 1."""
    return (IH + 2 - 3) // 2 + 1, (IW + 2 - 3) // 2 + 1


# ---- keyed dropout (csrc/common.h: drop_key, drop_run, drop_bits, a xorshift32 walk over each 16-byte chunk) -----------

GOLD = 0x9E3779B97F4A7C15


def keyed_keep_mask(M, Nout, seed, p, seed_dev=None, row_stride=None, ec=8, rows=None):
    """Keep-mask [M][Nout] (bool, numpy) of drop_mode 1: the chunk starting at element index row * Nout + chunk is hashed
    once with the key of seed (+ seed_dev * GOLD), then a xorshift32 walk hands out 16 bits per element; an element is
    dropped iff its 16 bits < floor(p * 2^32) >> 16 (p as the f32 the ABI carries).  row_stride: the index's row pitch
    (the kernels use Nout, never the leading dimension).  ec: elements per 16-byte store chunk, 8 (bf16) or 4 (f32: the
    chunks start at every fourth column and the walk hands out two pairs with one xorshift32 step between them).
    rows: the M output rows (an int array; default 0 .. M - 1) -- mask row i is that of output row rows[i], so the
    scattered rows of a parity class come from the same function."""
    assert ec in (4, 8) and Nout % ec == 0
    u64, u32 = np.uint64, np.uint32
    if seed_dev is not None:
        seed = (seed + seed_dev * GOLD) & 0xFFFFFFFFFFFFFFFF
    stride = Nout if row_stride is None else row_stride
    rows = np.arange(M, dtype=np.uint64) if rows is None else np.asarray(rows).reshape(-1).astype(np.uint64)
    assert rows.shape == (M,)
    with np.errstate(over="ignore"):
        x = u64(seed) * u64(GOLD) + u64(0xD6E8FEB86659FD93)
        x ^= x >> u64(32); x *= u64(0xD6E8FEB86659FD93); x ^= x >> u64(32)
        k0, k1 = u32(x & u64(0xFFFFFFFF)), u32(x >> u64(32))
        thresh16 = u32(int(float(np.float32(p)) * 4294967296.0) >> 16)
        idx = rows[:, None] * u64(stride) + np.arange(0, Nout, ec, dtype=np.uint64)[None, :]   # first element of every chunk
        s = (idx & u64(0xFFFFFFFF)).astype(u32) + k0 + (idx >> u64(32)).astype(u32) * k1
        s ^= s >> u32(16); s *= u32(0x7feb352d); s ^= s >> u32(15); s *= u32(0x846ca68b); s ^= s >> u32(16)
        keep = np.empty((M, Nout), dtype=bool)
        for e in range(0, ec, 2):
            keep[:, e::ec] = (s & u32(0xffff)) >= thresh16
            keep[:, e + 1::ec] = (s >> u32(16)) >= thresh16
            s ^= s << u32(13); s ^= s >> u32(17); s ^= s << u32(5)
    return keep


# ---- restated gates and counts -------------------------------------------------------------------------------------------

def cf_shape_ok(dtype, Cin, IH, IW, Nout, N):
    OH, OW = s2_out(IH, IW)
    return int(dtype == "bf16" and 1 <= Cin <= 4 and 8 <= Nout <= 256 and Nout % 8 == 0 and N >= 1 and IH >= 1 and
               IW >= 1 and N * OH * OW * 256 < 1 << 31 and N * Cin * IH * IW < 1 << 40)


def wf_shape_ok(dtype, Cin, IH, IW, Nout, N):
    OH, OW = s2_out(IH, IW)
    return int(dtype == "bf16" and 1 <= Cin <= 4 and Nout >= 64 and Nout % 64 == 0 and N >= 1 and IH >= 1 and IW >= 1 and
               N * OH * OW * 256 < 1 << 31 and N * Cin * IH * IW < 1 << 40)


def s2_blocks(N, IH, IW):
    OH, OW = s2_out(IH, IW)
    return N * cdiv(OH, TA) * cdiv(OW, TB)


def dgrad_blocks(dtype, Cout, OH, OW, C1, N):
    """rbvae_deconv_last_dgrad_blocks (OH x OW is the deconv's output = this convolution's input)."""
    return s2_blocks(N, OH, OW) if cf_shape_ok(dtype, Cout, OH, OW, C1, N) else 0


def wgrad_first_blocks(dtype, Cin, IH, IW, Nout, N):
    return s2_blocks(N, IH, IW) if wf_shape_ok(dtype, Cin, IH, IW, Nout, N) else 0


def dl_lds(C1):
    slices, y = (2 if C1 > 64 else 1) * (160 + 48) * 128, 160 * 37 * 4
    return max(slices, y)


def dl_parts(dtype, N, IH, IW, C1, Cout):
    """rbvae_deconv_last_fused_parts."""
    if dtype != "bf16" or Cout < 1 or Cout > 4 or C1 % 64 or C1 < 64 or dl_lds(C1) > 160 * 1024 - 256:
        return 0
    if N * 2 * IH * 2 * IW * Cout >= 1 << 31 or N * IH * IW * C1 >= 1 << 31:
        return 0
    return N * cdiv(IH, TA) * cdiv(IW, TB)


def conv_in_ok(dtype, Cin, H, W, Nout, N, cg):
    return int(dtype == "bf16" and 1 <= Cin <= 4 and 8 <= Nout <= 256 and Nout % 8 == 0 and N >= 1 and H >= 1 and W >= 1 and
               (cg == 0 or (cg in (4, 8, 16) and Nout % cg == 0)) and N * H * W * 256 < 1 << 31 and
               N * Cin * H * W < 1 << 31)


def conv_in_stats_floats(N, H, W, Nout, cg):
    return 2 * N * cdiv(H, TA) * cdiv(W, TB) * (Nout // cg)


def col2im_nparts(n_out):
    return min(max(cdiv(n_out, 256), 1), 4096)


def col2im_has_dcol(N, IH, IW, ldy, OH, OW, Cout):
    small = N * OH * OW * Cout < (1 << 31) - (1 << 20) and N * IH * IW * ldy < 1 << 31
    return int(small and Cout <= 4)


def col2im_kernel(N, IH, IW, ldy, OH, OW, Cout, dpre_aligned=True):
    """'pix' (col2im_sigmoid_pix_k, one thread per pixel) or 'general' (col2im_sigmoid_k, one thread per element); the
    frame-span term of `small` does not bind at test sizes."""
    return "pix" if col2im_has_dcol(N, IH, IW, ldy, OH, OW, Cout) and dpre_aligned else "general"


def cf_instance(Cin, mode, Nout):
    return ("conv_first_fused_k", Cin, mode, 1 if Nout <= 64 else 4)


def wf_instance(Cin, mode, Nout):
    return ("wgrad_first_wide_k" if Nout % 256 == 0 else "wgrad_first_k", Cin, mode)


def dl_instance(C1):
    return ("deconv_last_fused_k", C1 == 64)          # ONE


def ci_instance(Cin, Nout):
    return ("conv_in_k", Cin, 1 if Nout <= 64 else 2 if Nout <= 128 else 4)


CF_REACHABLE = {("conv_first_fused_k", ci, m, nq) for ci in (1, 2, 3, 4) for m in (0, 1) for nq in (1, 4)}
WF_REACHABLE = {(k, ci, m) for k in ("wgrad_first_k", "wgrad_first_wide_k") for ci in (1, 2, 3, 4) for m in (0, 1)}
DL_REACHABLE = {("deconv_last_fused_k", True), ("deconv_last_fused_k", False)}
CI_REACHABLE = {("conv_in_k", ci, nq) for ci in (1, 2, 3, 4) for nq in (1, 2, 4)}


def block_of_rows(N, OH, OW, swap=False):
    """Workgroup of every pixel row (n OH + y) OW + x of an [N][OH][OW] grid cut into 8 x 16 blocks: tbi fastest, then
    tai, then the image.  swap: the tai / tbi defect."""
    p = torch.arange(N * OH * OW)
    n, y, x = p // (OH * OW), p // OW % OH, p % OW
    ta_n, tb_n = cdiv(OH, TA), cdiv(OW, TB)
    if swap:
        return (n * tb_n + x // TB) * ta_n + y // TA
    return (n * ta_n + y // TA) * tb_n + x // TB


def k_slices(nblk, ks, shift=0):
    """Blocks [b0, b1) of every K-slice of rbvae_wgrad_first: per = ceil(nblk / ksplit), slice k = blocks k per ..
    min((k + 1) per, nblk).  shift: the off-by-one defect."""
    per = cdiv(nblk, ks)
    return [(min(k * per + shift, nblk), min((k + 1) * per + shift, nblk)) for k in range(ks)]


def by_block(vals, blk, nblk):
    """Sums of the rows of vals [rows][C] per block."""
    v = vals.double()
    return torch.zeros(nblk, v.shape[1], dtype=torch.float64).index_add_(0, blk, v)


# ---- frames behind a frame map --------------------------------------------------------------------------------------------

def frame_layout(N, fsz, fmap):
    """(element offset of every frame, buffer floats, (d1, d2, s0, s1, s2)) for fmap None (dense), 'gap' (dense order, 5
    floats between frames) or (Bi, T): an item batch [Bi][2][T] of padded frames read as view 0 of every item, then view 1
    (N = 2 Bi T; frame n = (v, b, t) at b s1 + v s0 + t s2)."""
    if fmap is None:
        return [n * fsz for n in range(N)], N * fsz, (0, 0, 0, 0, fsz)
    fp = fsz + 5
    if fmap == "gap":
        return [n * fp for n in range(N)], N * fp, (0, 0, 0, 0, fp)
    Bi, T = fmap
    assert N == 2 * Bi * T
    s0, s1, s2 = T * fp, 2 * T * fp, fp
    offs = [(n % (Bi * T)) // T * s1 + n // (Bi * T) * s0 + n % T * s2 for n in range(N)]
    return offs, 2 * Bi * T * fp, (Bi * T, T, s0, s1, s2)


def frame_buffer(x, fmap):
    """The frames x [N][...] laid out by frame_layout inside NaN: (flat f32 buffer, map)."""
    N = x.shape[0]
    fsz = x[0].numel()
    offs, total, fm = frame_layout(N, fsz, fmap)
    buf = torch.full((total,), float("nan"))
    for n, o in enumerate(offs):
        buf[o:o + fsz] = x[n].reshape(-1)
    return buf, fm


def im2col_rows(x, k=3, stride=2, pad=1, order="tap"):
    """[N OH OW][k k C] rows of x [N][C][H][W]: column (kh k + kw) C + c ('tap'), or c k k + kh k + kw ('ci': the defect)."""
    N, C = x.shape[:2]
    u = F.unfold(x, k, padding=pad, stride=stride)                                  # [N][C k k][L], (c, kh, kw)
    L = u.shape[-1]
    if order == "tap":
        return u.reshape(N, C, k * k, L).permute(0, 3, 2, 1).reshape(N * L, k * k * C)
    return u.permute(0, 2, 1).reshape(N * L, C * k * k)


def col64(x, dtype=torch.bfloat16, order="tap"):
    """The [P][64] im2col image of the fused kernels in the storage type (padding columns zero)."""
    r = im2col_rows(x.float(), order=order)
    out = torch.zeros(r.shape[0], 64, dtype=dtype)
    out[:, :r.shape[1]] = r.to(dtype)
    return out


# ---- conv_first_fused_k: rbvae_conv_first_fused (mode 0) and rbvae_deconv_last_dgrad_fused (mode 1) ---------------------

def cf(id, mode, N, Cin, IH, IW, Nout, ldo=0, relu=1, bias=1, drop=None, fmap=None, scale=1.0):
    return dict(id=f"m{mode}_{id}", mode=mode, N=N, Cin=Cin, IH=IH, IW=IW, Nout=Nout, ldo=Nout + ldo, relu=relu, bias=bias,
                drop=drop, fmap=fmap, scale=1.25 if drop else scale, p=0.2 if drop else 0.0, seed=77, seed_dev=0x123456789 if drop == "seed_dev" else None)


def _cf_table(mode):
    m0 = mode == 0
    k = lambda **kw: kw if m0 else {}           # mode 1 has no bias / ReLU / dropout / frame map; it has gate, scale, colsum
    sc = 1.0 if m0 else 1.25
    return [
        cf("c1_1x1_n8", mode, 3, 1, 1, 1, 8, ldo=8, scale=sc),
        cf("c2_1x33_n24", mode, 2, 2, 1, 33, 24, scale=sc, **k(relu=0, bias=0, drop="seed")),
        cf("c3_15x17_n64_gap", mode, 2, 3, 15, 17, 64, ldo=8, scale=sc, **k(drop="seed_dev", fmap="gap")),
        cf("c4_1x33_n64", mode, 2, 4, 1, 33, 64, scale=sc, **k(relu=0)),
        cf("c4_32x64_n72_exact", mode, 2, 4, 32, 64, 72, scale=sc, **k(fmap=(1, 1))),
        cf("c3_33x65_n200_onepast", mode, 1, 3, 33, 65, 200, ldo=16, scale=sc, **k(relu=0, drop="seed")),
        cf("c1_33x65_n72", mode, 1, 1, 33, 65, 72, ldo=8, scale=sc, **k(bias=0, drop="seed_dev")),
        cf("c4_88x160_n256_native", mode, 4, 4, 88, 160, 256, scale=sc, **k(drop="seed", fmap=(1, 2))),
        cf("c2_88x160_n248", mode, 1, 2, 88, 160, 248, ldo=8, scale=sc, **k(bias=0)),
        cf("c3_256x256_n64", mode, 1, 3, 256, 256, 64, scale=sc, **k(drop="seed_dev")),
    ]


CF_CASES = _cf_table(0) + _cf_table(1)

GATE_PATTERNS = (0x0000, 0x8000, 0x7F80, 0x7FC0, 0xFFC0, 0x7F81, 0xFF80, 0x0001)   # +0 -0 +inf NaN -NaN sNaN -inf denormal


def cf_build(c, reference=True):
    """Operands of a conv_first case.  mode 0: frames x [N][Cin][IH][IW] f32; mode 1: the same numbers stored NHWC
    (`x_store`).  w [Nout][Cin][3][3] bf16-rounded, Wp [Nout][64] packed tap-major; bias; gate (mode 1: every pattern of
    GATE_PATTERNS among ordinary values); keep (mode 0 dropout: the host mask)."""
    N, Cin, IH, IW, Nout = c["N"], c["Cin"], c["IH"], c["IW"], c["Nout"]
    OH, OW = s2_out(IH, IW)
    P = N * OH * OW
    g = torch.Generator().manual_seed(seed_of(c))
    x = torch.randn(N, Cin, IH, IW, generator=g)
    w = bf16r(torch.randn(Nout, Cin, 3, 3, generator=g) * 0.3)
    Wp = torch.zeros(Nout, 64, dtype=torch.bfloat16)
    Wp[:, :9 * Cin] = w.permute(0, 2, 3, 1).reshape(Nout, 9 * Cin)
    d = dict(x=x, w=w, Wp=Wp, P=P, OH=OH, OW=OW, bias=None, gate=None, keep=None, nblk=s2_blocks(N, IH, IW),
             x_store=x if c["mode"] == 0 else x.permute(0, 2, 3, 1).contiguous())
    if c["mode"] == 0 and c["bias"]:
        d["bias"] = torch.randn(Nout, generator=g) * 0.5
    if c["mode"] == 1:
        bits = bf16r(torch.randn(P, Nout, generator=g)).view(torch.int16).clone()
        flat = bits.reshape(-1)
        pos = torch.arange(flat.numel())
        for i, pat in enumerate(GATE_PATTERNS):
            flat[pos % 13 == i] = pat - 0x10000 if pat >= 0x8000 else pat
        d["gate"] = bits.view(torch.bfloat16)
    if c["drop"]:
        d["keep"] = torch.from_numpy(keyed_keep_mask(P, Nout, c["seed"], c["p"], c["seed_dev"]))
    if reference:
        ref, S = B.ref_and_scale("conv2d", bf16r(x), w, stride=2, padding=1)
        ref, S = B.rows(ref), B.rows(S)
        if d["bias"] is not None:
            ref, S = ref + d["bias"].double(), S + d["bias"].double().abs()
        ref = ref * float(np.float32(c["scale"]))
        if c["mode"] == 0:
            if c["relu"]:
                ref = ref.clamp_min(0)
            if d["keep"] is not None:
                ref = ref * d["keep"]
        else:
            ref = ref * (d["gate"].float() > 0)                       # kept iff 0 < g <= +inf; NaN, -0.0 and negatives are not
        d["ref"], d["S"] = ref, S
    return d


def cf_forward(c, d, dt=torch.float64, defect=None):
    """The operation restated through the im2col rows (independent of the conv2d reference): out [P][Nout] (rounded to bf16
    when dt is f32), col int16 [P][64], colsum [nblk][Nout] of the out it returns."""
    N, Nout, OH, OW, P = c["N"], c["Nout"], d["OH"], d["OW"], d["P"]
    xb = bf16r(d["x"])
    w = d["w"]
    if defect == "khkw":
        w = w.transpose(2, 3)
    Wp = torch.zeros(Nout, 64, dtype=dt)
    Wp[:, :9 * c["Cin"]] = w.permute(0, 2, 3, 1).reshape(Nout, -1).to(dt)

    def rows_of(xx):
        if defect == "pad0":
            r = im2col_rows(F.pad(xx.float(), (0, 2, 0, 2)), pad=0)
            r = F.pad(r, (0, 64 - r.shape[1]))
            return r.to(dt)
        return col64(xx, torch.float32, order="ci" if defect == "ci_major" else "tap").to(dt)

    col = rows_of(xb)
    acc = col @ Wp.t()
    if defect == "halo_col":                     # the column 2 ow0 - 1 of every block but the first reads as zero
        xz = xb.clone()
        for iw in range(2 * TB - 1, c["IW"], 2 * TB):
            xz[..., iw] = 0
        az = rows_of(xz) @ Wp.t()
        first_col = (torch.arange(P) % OW) % TB == 0
        acc[first_col] = az[first_col]
    if defect == "halo_row":                     # the same for the row 2 oh0 - 1
        xz = xb.clone()
        for ih in range(2 * TA - 1, c["IH"], 2 * TA):
            xz[..., ih, :] = 0
        az = rows_of(xz) @ Wp.t()
        first_row = (torch.arange(P) // OW % OH) % TA == 0
        acc[first_row] = az[first_row]
    if d["bias"] is not None:
        b = d["bias"].to(dt).clone()
        if defect == "bias_second_chunk":
            b[torch.arange(Nout) % 16 >= 8] = 0
        acc = acc + b
    v = acc * torch.tensor(c["scale"], dtype=torch.float32).to(dt)
    if dt == torch.float32:
        v = bf16r(v).to(dt)
    if c["mode"] == 0:
        if c["relu"]:
            v = v.clamp_min(0)
        if c["drop"]:
            keep = d["keep"]
            if defect == "drop_ldo":
                keep = torch.from_numpy(keyed_keep_mask(P, Nout, c["seed"], c["p"], c["seed_dev"], row_stride=c["ldo"]))
            v = v * keep
    else:
        gt = d["gate"].float()
        keep = gt >= 0 if defect == "gate_ge0" else ~(gt <= 0) if defect == "gate_nan" else gt > 0
        v = v * keep
    if defect == "ragged_row":                   # the last image row of a block that sticks out is never stored
        assert OH % TA
        v = v.clone()
        v[torch.arange(P) // OW % OH == OH - 1] = float("nan")
    out = dict(out=v, col=col64(d["x"]).view(torch.int16))
    if c["mode"] == 1:
        out["colsum"] = by_block(v, block_of_rows(N, OH, OW, swap=defect == "colsum_swap"), d["nblk"]).to(dt)
    return out


def cf_check(c, d, got, what=""):
    """got: out [P][Nout], col int16 [P][64] or None, colsum [nblk][Nout] or None (mode 1).  Returns worst ratios."""
    what = what or c["id"]
    res = {}
    out = got["out"].detach().cpu()
    res["out"] = B.check(out, d["ref"], d["S"], out_dtype=torch.bfloat16, K=64, scale=c["scale"],
                         nhw=(c["N"], d["OH"], d["OW"]), what=what)
    if got.get("col") is not None:
        want = col64(d["x"]).view(torch.int16)
        assert torch.equal(got["col"].cpu(), want), f"{what}: col rows differ from the bf16-rounded im2col rows"
    if got.get("colsum") is not None:
        blk = block_of_rows(c["N"], d["OH"], d["OW"])
        want, sabs = by_block(out, blk, d["nblk"]), by_block(out.double().abs(), blk, d["nblk"])
        bnd = (TA * TB - 1) * U * sabs + B.TINY
        cs = got["colsum"].detach().cpu().double()
        r = (cs - want).abs() / bnd
        r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
        assert bool((r <= 1).all()), (what, "colsum row", int(r.max(1).values.argmax()), float(r.max()))
        assert bool((cs[sabs == 0] == 0).all()), f"{what}: column sum of a channel with nothing stored is not zero"
        res["colsum"] = float(r.max())
    return res


# ---- rbvae_wgrad_first ---------------------------------------------------------------------------------------------------

def wf(id, mode, N, Cin, IH, IW, Nout, ks, ldy=0, fmap=None):
    """ks: an int, or 'nblk'."""
    nblk = s2_blocks(N, IH, IW)
    return dict(id=f"m{mode}_{id}", mode=mode, N=N, Cin=Cin, IH=IH, IW=IW, Nout=Nout, ks=nblk if ks == "nblk" else ks,
                ldy=Nout + ldy, fmap=fmap if mode == 0 else None)


def _wf_table(mode):
    return [
        wf("c1_1x1_n64_ks_nblk", mode, 3, 1, 1, 1, 64, "nblk", ldy=8),
        wf("c2_33x65_n128_ks7_empty", mode, 2, 2, 33, 65, 128, 7, fmap="gap"),            # 18 blocks, per 3: slice 6 empty
        wf("c3_21x40_n192_ks1", mode, 2, 3, 21, 40, 192, 1, ldy=16),
        wf("c4_15x17_n320_ks3", mode, 4, 4, 15, 17, 320, 3, fmap=(1, 2)),                  # 4 blocks, per 2: slice 2 empty
        wf("c1_33x65_n256_ks4_empty", mode, 1, 1, 33, 65, 256, 4, ldy=8),                  # 9 blocks, per 3: slice 3 empty
        wf("c2_15x17_n512_ks_nblk", mode, 2, 2, 15, 17, 512, "nblk", fmap="gap"),
        wf("c3_88x160_n256_ks4", mode, 1, 3, 88, 160, 256, 4),
        wf("c4_32x64_n256_ks1", mode, 2, 4, 32, 64, 256, 1, ldy=8),
        wf("c3_33x65_n64_ks5", mode, 1, 3, 33, 65, 64, 5),                                # 9 blocks, per 2: 5 slices, last short
    ]


WF_CASES = _wf_table(0) + _wf_table(1)


def wf_build(c):
    N, Cin, IH, IW, Nout = c["N"], c["Cin"], c["IH"], c["IW"], c["Nout"]
    OH, OW = s2_out(IH, IW)
    P = N * OH * OW
    g = torch.Generator().manual_seed(seed_of(c))
    x = torch.randn(N, Cin, IH, IW, generator=g)
    dy = bf16r(torch.randn(P, Nout, generator=g) / 8)
    return dict(x=x, x_store=x if c["mode"] == 0 else x.permute(0, 2, 3, 1).contiguous(), dy=dy, P=P, OH=OH, OW=OW,
                nblk=s2_blocks(N, IH, IW), col=col64(x).double(), blk=block_of_rows(N, OH, OW))


def wf_slice_rows(c, d, shift=0):
    return [torch.nonzero((d["blk"] >= b0) & (d["blk"] < b1)).reshape(-1) for b0, b1 in k_slices(d["nblk"], c["ks"], shift)]


def wf_forward(c, d, dt=torch.float64, defect=None):
    """slabs [ks][Nout][64]: dW[ks][co][k] = sum over the pixels of slice ks of dY[p][co] col[p][k]."""
    col = d["col"]
    if defect == "ci_major":
        col = col64(d["x"], order="ci").double()
    out = []
    for idx in wf_slice_rows(c, d, 1 if defect == "kslice_off_by_one" else 0):
        out.append(d["dy"][idx].to(dt).t() @ col[idx].to(dt))
    return torch.stack(out)


def wf_check(c, d, slabs, what=""):
    what = what or c["id"]
    got = slabs.detach().cpu().double().reshape(c["ks"], c["Nout"], 64)
    worst = 0.0
    dy, col = d["dy"].double(), d["col"]
    for k, idx in enumerate(wf_slice_rows(c, d)):
        if idx.numel() == 0:
            assert bool((got[k] == 0).all()), f"{what}: empty K-slice {k} is not zero"
            continue
        a, u = dy[idx], col[idx]
        worst = max(worst, B.check(got[k], a.t() @ u, a.abs().t() @ u.abs(), out_dtype=torch.float32, K=idx.numel(),
                                   what=f"{what} K-slice {k}"))
        assert bool((got[k][:, 9 * c["Cin"]:] == 0).all()), f"{what}: padding columns of K-slice {k} are not zero"
    return worst


# ---- rbvae_deconv_last_fused ---------------------------------------------------------------------------------------------

def dl(id, N, IH, IW, C1, Cout, NYP=0, target="plain", dpre=1, sat=0, bias=1):
    return dict(id=id, N=N, IH=IH, IW=IW, C1=C1, Cout=Cout, NYP=NYP or cdiv(9 * Cout, 8) * 8, target=target, dpre=dpre,
                sat=sat, bias=bias, gscale=0.37)


DL_CASES = [
    dl("one_1x1_co1", 3, 1, 1, 64, 1),
    dl("k2_8x16_co2_nyp48_gap", 2, 8, 16, 128, 2, NYP=48, target="gap"),
    dl("k3_9x17_co3_mapped", 2, 9, 17, 192, 3, target=(1, 1)),
    dl("k4_5x37_co4_no_dpre", 1, 5, 37, 256, 4, dpre=0),
    dl("k5_11x20_co4_nyp48", 2, 11, 20, 320, 4, NYP=48),
    dl("k4_44x80_co4_mapped", 2, 44, 80, 256, 4, target=(1, 1)),
    dl("one_11x20_co3_nyp48_no_target", 1, 11, 20, 64, 3, NYP=48, target=None, dpre=0),
    dl("k3_5x37_co1_no_bias", 1, 5, 37, 192, 1, bias=0),
    dl("one_9x17_co2", 2, 9, 17, 64, 2, target="gap"),
    dl("sat_k2_9x17_co4", 2, 9, 17, 128, 4, sat=1),
    dl("sat_one_8x16_co3", 1, 8, 16, 64, 3, sat=1, NYP=48),
    dl("sat_k5_11x20_co2", 1, 11, 20, 320, 2, sat=1),
]


def dl_out_blocks(c):
    """Workgroup of every OUTPUT pixel row (n OH + oh) OW + ow: the 8 x 16 block of its input pixel (oh / 2, ow / 2)."""
    N, IH, IW = c["N"], c["IH"], c["IW"]
    OH, OW = 2 * IH, 2 * IW
    p = torch.arange(N * OH * OW)
    n, oh, ow = p // (OH * OW), p // OW % OH, p % OW
    return (n * cdiv(IH, TA) + oh // 2 // TA) * cdiv(IW, TB) + ow // 2 // TB


def dl_build(c):
    """a [N][C1][IH][IW] and V [C1][Cout][3][3] bf16; Vp [NYP][C1], row tap Cout + co, the rows past 9 Cout filled with
    values no output may depend on; bias; target [N][Cout][OH][OW]; pre (float64) and S_pre."""
    N, IH, IW, C1, Cout = c["N"], c["IH"], c["IW"], c["C1"], c["Cout"]
    g = torch.Generator().manual_seed(seed_of(c))
    amp = 12.0 / (0.5 * (2.25 * C1) ** 0.5) if c["sat"] else 0.1
    a = bf16r(torch.randn(N, C1, IH, IW, generator=g) * 0.5)
    V = bf16r(torch.randn(C1, Cout, 3, 3, generator=g) * amp)
    Vp = bf16r(torch.randn(c["NYP"], C1, generator=g))
    Vp[:9 * Cout] = V.permute(2, 3, 1, 0).reshape(9 * Cout, C1)
    bias = torch.randn(Cout, generator=g) if c["bias"] else None
    tgt = torch.rand(N, Cout, 2 * IH, 2 * IW, generator=g) if c["target"] is not None else None
    pre, S = B.ref_and_scale("conv_transpose2d", a, V)
    if bias is not None:
        pre, S = pre + bias.double()[None, :, None, None], S + bias.double().abs()[None, :, None, None]
    return dict(a=a, V=V, Vp=Vp, bias=bias, target=tgt, pre=pre, S=S, parts=N * cdiv(IH, TA) * cdiv(IW, TB),
                blk=dl_out_blocks(c), gscale=float(np.float32(c["gscale"])))


def _sig_fast32(v):
    """rcp(1 + exp2(-log2e v)) with every step rounded to f32."""
    e = torch.exp2(torch.tensor(-LOG2E_F32, dtype=torch.float32) * v)
    return 1.0 / (1.0 + e)


def losses_of(xr, tgt, gscale, blk, parts, dt, no_gscale=False, sse_rows=None):
    """dpre [N][OH][OW][Cout], sse [parts], dsum [parts][4] from xr [N][Cout][OH][OW] (block blk per pixel row)."""
    Cout = xr.shape[1]
    dlt = xr.to(dt) - tgt.to(dt)
    dp = (dlt if no_gscale else torch.tensor(gscale, dtype=dt) * dlt) * xr.to(dt) * (1 - xr.to(dt))
    sq = B.rows(dlt * dlt)
    if sse_rows is not None:
        sq = sq * sse_rows[:, None]
    sse = by_block(sq, blk, parts).sum(1)
    dsum = torch.zeros(parts, 4, dtype=torch.float64)
    dsum[:, :Cout] = by_block(B.rows(dp), blk, parts)
    return dp.permute(0, 2, 3, 1).contiguous(), sse.to(dt), dsum.to(dt)


def dl_forward(c, d, dt=torch.float64, defect=None):
    a, V = d["a"].to(dt), d["V"].to(dt)
    if defect == "tap_parity":
        V = V.roll(1, 2)
    if defect == "y_bf16":                       # the two-kernel arithmetic: every tap's product rounded to bf16 before the gather
        pre = 0
        for t in range(9):
            Vt = torch.zeros_like(V)
            Vt[:, :, t // 3, t % 3] = V[:, :, t // 3, t % 3]
            pre = pre + bf16r(F.conv_transpose2d(a, Vt, stride=2, padding=1, output_padding=1)).to(dt)
    else:
        pre = F.conv_transpose2d(a, V, stride=2, padding=1, output_padding=1)
    if d["bias"] is not None:
        pre = pre + d["bias"].to(dt)[None, :, None, None]
    xr = _sig_fast32(pre) if dt == torch.float32 else torch.sigmoid(pre)
    out = dict(xr=xr)
    if d["target"] is not None:
        tgt = d["target"]
        if defect == "target_plane":            # channel c read at a plane stride of OH OW + 1
            tgt = torch.stack([tgt[:, k].reshape(c["N"], -1).roll(-k, 1).reshape(tgt[:, k].shape) for k in range(c["Cout"])], 1)
        rows = None
        if defect == "sse_ragged":
            p = torch.arange(d["blk"].numel())
            oh, ow = p // (2 * c["IW"]) % (2 * c["IH"]), p % (2 * c["IW"])
            rows = ((oh < 2 * TA * (c["IH"] // TA)) & (ow < 2 * TB * (c["IW"] // TB))).double()
        dp, sse, dsum = losses_of(xr, tgt, d["gscale"], d["blk"], d["parts"], dt, no_gscale=defect == "no_gscale",
                                  sse_rows=rows)
        out["sse"] = sse
        if c["dpre"]:
            out["dpre"], out["dsum"] = dp, dsum
    return out


def sigmoid_bound(pre, S_pre, d_unit, lib):
    """|s_kernel - sigmoid(pre)| for a pre-activation off by at most d_unit S_pre (module docstring)."""
    s = torch.sigmoid(pre)
    dp = d_unit * S_pre
    return s * (1 - s) * dp + 0.05 * dp * dp + c_sig(pre, lib=lib)


def _ratio(err, bnd):
    r = err / bnd
    return torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)


def check_losses(xr, tgt, gscale, blk, parts, got, h_sse, h_dsum, what):
    """dpre / sse / dsum of `got` against float64 from the STORED xr.  Returns worst ratios."""
    res = {}
    Cout = xr.shape[1]
    dp, sse, dsum = losses_of(xr.double(), tgt, gscale, blk, parts, torch.float64)
    if got.get("dpre") is not None:
        gd = got["dpre"].detach().cpu().double()
        r = _ratio((gd - dp).abs(), gamma(5) * dp.abs() + F32_MIN)
        assert bool((r <= 1).all()), f"{what}: dpre worst |err|/bound {float(r.max()):.3g}"
        res["dpre"] = float(r.max())
        if got.get("dsum") is not None:
            gs = got["dsum"].detach().cpu().double()
            stored = gd.reshape(-1, Cout)
            want = torch.zeros(parts, 4, dtype=torch.float64)
            want[:, :Cout] = by_block(stored, blk, parts)
            sabs = torch.zeros(parts, 4, dtype=torch.float64)
            sabs[:, :Cout] = by_block(stored.abs(), blk, parts)
            r = _ratio((gs - want).abs(), gamma(h_dsum) * sabs + F32_MIN)
            assert bool((r <= 1).all()), f"{what}: dpre column sums worst |err|/bound {float(r.max()):.3g}"
            assert bool((gs[:, Cout:] == 0).all()), f"{what}: unused dpre column sums are not zero"
            res["dsum"] = float(r.max())
    if got.get("sse") is not None:
        r = _ratio((got["sse"].detach().cpu().double() - sse).abs(), gamma(h_sse + 3) * sse + F32_MIN)
        assert bool((r <= 1).all()), f"{what}: sse parts worst |err|/bound {float(r.max()):.3g} at block {int(r.argmax())}"
        res["sse"] = float(r.max())
    return res


def dl_check(c, d, got, what=""):
    what = what or c["id"]
    xr = got["xr"].detach().cpu()
    x64 = xr.double()
    assert bool(torch.isfinite(x64).all()) and float(x64.min()) >= 0.0 and float(x64.max()) <= 1.0, f"{what}: xr outside [0, 1]"
    r = _ratio((x64 - torch.sigmoid(d["pre"])).abs(), sigmoid_bound(d["pre"], d["S"], B.c_acc(4 * c["C1"]), lib=False))
    if not bool((r <= 1).all()):
        i = int(r.reshape(-1).argmax())
        raise AssertionError(f"{what}: xr worst |err|/bound {float(r.max()):.3g} at flat {i}: got {float(x64.reshape(-1)[i])!r}, "
                             f"pre {float(d['pre'].reshape(-1)[i])!r}")
    res = dict(xr=float(r.max()))
    if d["target"] is not None:
        # per thread 2 pixels x Cout terms, six wave_sum levels, three additions over the waves
        res.update(check_losses(xr, d["target"], d["gscale"], d["blk"], d["parts"], got, 2 * c["Cout"] + 9, 2 + 9, what))
    return res


# ---- rbvae_conv_in ----------------------------------------------------------------------------------------------------

def ci(id, N, Cin, H, W, Nout, cg, ldo=0, bias=1):
    return dict(id=id, N=N, Cin=Cin, H=H, W=W, Nout=Nout, cg=cg, ldo=Nout + ldo, bias=bias)


CI_CASES = [
    ci("c1_n32_cg4_1x1", 3, 1, 1, 1, 32, 4, ldo=8),
    ci("c2_n64_cg8_9x17", 2, 2, 9, 17, 64, 8),
    ci("c3_n64_cg16_8x16", 2, 3, 8, 16, 64, 16, ldo=16),
    ci("c4_n32_cg8_5x37", 1, 4, 5, 37, 32, 8, bias=0),
    ci("c1_n128_cg16_20x33", 1, 1, 20, 33, 128, 16, ldo=8),
    ci("c2_n128_cg4_9x17", 2, 2, 9, 17, 128, 4),
    ci("c3_n128_cg8_64x64", 1, 3, 64, 64, 128, 8),
    ci("c4_n128_cg16_5x37", 2, 4, 5, 37, 128, 16, ldo=8, bias=0),
    ci("c1_n256_cg4_9x17", 1, 1, 9, 17, 256, 4),
    ci("c2_n256_cg8_20x33", 1, 2, 20, 33, 256, 8, ldo=8),
    ci("c3_n256_cg16_5x37", 2, 3, 5, 37, 256, 16),
    ci("c4_n256_cg4_24x40", 1, 4, 24, 40, 256, 4),
]


def ci_build(c):
    N, Cin, H, W, Nout = c["N"], c["Cin"], c["H"], c["W"], c["Nout"]
    g = torch.Generator().manual_seed(seed_of(c))
    x = torch.randn(N, Cin, H, W, generator=g)
    w = bf16r(torch.randn(Nout, Cin, 3, 3, generator=g) * 0.3)
    Wp = torch.zeros(Nout, 64, dtype=torch.bfloat16)
    Wp[:, :9 * Cin] = w.permute(0, 2, 3, 1).reshape(Nout, 9 * Cin)
    bias = torch.randn(Nout, generator=g) * 0.5 if c["bias"] else None
    ref, S = B.ref_and_scale("conv2d", bf16r(x), w, stride=1, padding=1)
    ref, S = B.rows(ref), B.rows(S)
    if bias is not None:
        ref, S = ref + bias.double(), S + bias.double().abs()
    return dict(x=x, w=w, Wp=Wp, bias=bias, ref=ref, S=S, tile=block_of_rows(N, H, W), ntiles=N * cdiv(H, TA) * cdiv(W, TB))


def ci_forward(c, d, dt=torch.float64, defect=None):
    """out [P][Nout] (bf16-rounded for f32) and stats [ntiles Nout/cg][2] = (mean, M2) of the out it returns."""
    w = d["w"].transpose(2, 3) if defect == "khkw" else d["w"]
    v = B.rows(F.conv2d(bf16r(d["x"]).to(dt), w.to(dt), None, stride=1, padding=1))
    if d["bias"] is not None:
        v = v + d["bias"].to(dt)
    if dt == torch.float32:
        v = bf16r(v).to(dt)
    mean, m2 = tile_stats_ref(v, d["tile"], d["ntiles"], c["cg"])[:2]
    return dict(out=v, stats=torch.stack([mean, m2], -1).reshape(-1, 2).to(dt))


def ci_check(c, d, got, what=""):
    what = what or c["id"]
    out = got["out"].detach().cpu()
    res = dict(out=B.check(out, d["ref"], d["S"], out_dtype=torch.bfloat16, K=64, nhw=(c["N"], c["H"], c["W"]), what=what))
    if got.get("stats") is not None:
        # conv_in_k's sums are shallower than conv_halo_k's (<= 4 pixels x 16 channels per lane, four DPP levels, <= 8
        # waves, one division: height <= 21 < stats_height(cg) = cg + 28), and its M2 is two-pass (n E^2 from the mean's
        # error, inside tile_stats_bounds' 5 n E^2): the halo bound holds as it stands
        res["stats"] = max(check_tile_stats(got["stats"].reshape(-1, 2), out, d["tile"], d["ntiles"], c["cg"], what=what))
    return res


def ci_gn_finish_ref(c, stored, eps):
    """float64 (mean, rstd) per image and group of the stored output and the bounds of rbvae_gn_finish_tiles(.., 8, 16):
    _halo_cases.gn_finish_ref with conv_in's 8 x 16 tiles."""
    N, H, W, cg = c["N"], c["H"], c["W"], c["cg"]
    tile, ntiles = block_of_rows(N, H, W), N * cdiv(H, TA) * cdiv(W, TB)
    v = stored.double().reshape(N, H * W, -1)
    G, nb, total = v.shape[-1] // cg, cdiv(H, TA) * cdiv(W, TB), H * W * cg
    grp = v.reshape(N, H * W, G, cg).permute(0, 2, 1, 3).reshape(N, G, -1)
    mean = grp.mean(-1)
    var = ((grp - mean[..., None]) ** 2).sum(-1) / total
    amax = grp.abs().amax(-1)
    tmean, tm2, tcnt, tsabs, tamax = tile_stats_ref(stored, tile, ntiles, cg)
    _, bM2_t, E_t = B.tile_stats_bounds(tcnt, cg, tsabs, tamax, tm2)
    hf = cdiv(nb, 256) + 6 + 3 + 2
    E_f = E_t.reshape(N, nb, G).amax(1) + hf * U * amax
    Q = var * total
    bq = bM2_t.reshape(N, nb, G).sum(1) + (hf + 3) * U * Q + 2 * E_f * (total * Q) ** 0.5 + total * E_f ** 2
    b_var = bq / total + U * var
    veps = var + float(torch.tensor(eps, dtype=torch.float32))
    rstd = veps.rsqrt()
    return mean, rstd, E_f + B.TINY, (0.5 * (b_var / veps + U) + 2 * U) * rstd * 1.01 + B.TINY


# ---- rbvae_im2col(_frames) ----------------------------------------------------------------------------------------------

def im(id, dtype, N, C, H, W, stride, layout="nchw", fmap=None, Kpad=64):
    return dict(id=id, dtype=dtype, N=N, C=C, H=H, W=W, stride=stride, layout=layout, fmap=fmap, Kpad=Kpad)


IM_CASES = [
    im("f32_c4_s2", "f32", 2, 4, 9, 14, 2),
    im("f32_c3_s1_gap", "f32", 2, 3, 7, 10, 1, fmap="gap", Kpad=32),
    im("f32_c2_s2_nhwc", "f32", 3, 2, 8, 12, 2, layout="nhwc", Kpad=24),
    im("f32_c1_s1", "f32", 1, 1, 5, 37, 1, Kpad=16),
    im("bf16_c4_s2_nhwc", "bf16", 2, 4, 21, 40, 2, layout="nhwc"),
    im("bf16_c3_s2_mapped", "bf16", 4, 3, 15, 17, 2, fmap=(1, 2)),
    im("bf16_c2_s1", "bf16", 2, 2, 9, 14, 1, Kpad=24),
    im("bf16_c1_s2_gap", "bf16", 3, 1, 1, 33, 2, fmap="gap"),
    im("bf16_c4_s1_1x1", "bf16", 2, 4, 1, 1, 1, Kpad=40),
]


def im_kernel(c):
    return ("im2col_fast_k", c["dtype"], c["C"] if c["C"] in (3, 4) else 0)


def im_build(c):
    g = torch.Generator().manual_seed(seed_of(c))
    x = torch.randn(c["N"], c["C"], c["H"], c["W"], generator=g)
    OH = (c["H"] + 2 - 3) // c["stride"] + 1
    OW = (c["W"] + 2 - 3) // c["stride"] + 1
    r = im2col_rows(x, stride=c["stride"]).to(TDT[c["dtype"]])
    want = torch.zeros(r.shape[0], c["Kpad"], dtype=r.dtype)
    want[:, :r.shape[1]] = r
    return dict(x=x, x_store=x if c["layout"] == "nchw" else x.permute(0, 2, 3, 1).contiguous(), OH=OH, OW=OW, want=want)


def same_bits(a, b):
    it = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))


# ---- rbvae_col2im_sigmoid(_frames) and rbvae_sigmoid_bwd_nhwc --------------------------------------------------------------

def c2(id, dtype, N, IH, IW, Cout, ldy=0, target="plain", dpre=1, sse_mean=1, gs_dev=0, bias=1):
    return dict(id=id, dtype=dtype, N=N, IH=IH, IW=IW, Cout=Cout, ldy=cdiv(9 * Cout, 8) * 8 + ldy, target=target, dpre=dpre,
                sse_mean=sse_mean, gs_dev=gs_dev, bias=bias, gscale=0.37)


C2_CASES = [
    c2("f32_co1_1x1", "f32", 3, 1, 1, 1, ldy=8),
    c2("f32_co2_9x17_gap_parts", "f32", 2, 9, 17, 2, target="gap", sse_mean=0),
    c2("f32_co3_11x20_gsdev", "f32", 2, 11, 20, 3, ldy=8, gs_dev=1),
    c2("f32_co4_5x37_mapped", "f32", 2, 5, 37, 4, target=(1, 1)),
    c2("f32_co5_general", "f32", 2, 9, 17, 5, ldy=4),
    c2("bf16_co1_9x17_gsdev", "bf16", 2, 9, 17, 1, gs_dev=1, sse_mean=0),
    c2("bf16_co2_5x37_no_dpre", "bf16", 1, 5, 37, 2, ldy=16, dpre=0),
    c2("bf16_co3_11x20_mapped", "bf16", 2, 11, 20, 3, target=(1, 1)),
    c2("bf16_co4_44x80", "bf16", 1, 44, 80, 4, ldy=8),
    c2("bf16_co5_general_gap", "bf16", 1, 5, 37, 5, target="gap", sse_mean=0),
    c2("bf16_co4_no_target", "bf16", 1, 8, 16, 4, target=None, dpre=0, sse_mean=0, bias=0),
]


def c2_geom(c):
    OH, OW = 2 * c["IH"], 2 * c["IW"]
    tot = c["N"] * OH * OW * c["Cout"]
    kern = col2im_kernel(c["N"], c["IH"], c["IW"], c["ldy"], OH, OW, c["Cout"])
    return OH, OW, tot, col2im_nparts(tot), kern


def c2_blocks(c):
    """Workgroup whose partial sums a pixel row (pix kernel) or an NCHW element (general kernel) lands in: a grid-stride
    loop of nb blocks of 256 threads -> (i / 256) % nb."""
    OH, OW, tot, nb, kern = c2_geom(c)
    n = c["N"] * OH * OW if kern == "pix" else tot
    return torch.arange(n) // 256 % nb


def c2_build(c):
    """Y [N IH IW][9 Cout] in the storage type (every tap's product per input pixel), bias, target; pre / S_pre in float64
    from the STORED Y: bias + the (<= 4) taps that reach an output pixel."""
    N, IH, IW, Cout = c["N"], c["IH"], c["IW"], c["Cout"]
    g = torch.Generator().manual_seed(seed_of(c))
    Y = (torch.randn(N * IH * IW, 9 * Cout, generator=g) * 0.8).to(TDT[c["dtype"]])
    bias = torch.randn(Cout, generator=g) if c["bias"] else None
    tgt = torch.rand(N, Cout, 2 * IH, 2 * IW, generator=g) if c["target"] is not None else None
    return dict(Y=Y, bias=bias, target=tgt, gs=float(np.float32(0.61)),
                gscale=float(np.float32(c["gscale"]) * (np.float32(0.61) if c["gs_dev"] else np.float32(1.0))))


def c2_gather(c, Y, bias, dt):
    """(pre, S_pre) [N][Cout][OH][OW]: fold of the per-tap products (col2im of a stride-2, pad-1, 3 x 3 transposed conv)."""
    N, IH, IW, Cout = c["N"], c["IH"], c["IW"], c["Cout"]
    y = Y.to(dt).reshape(N, IH * IW, 9, Cout).permute(0, 3, 2, 1).reshape(N, Cout * 9, IH * IW)   # fold wants (c, kh, kw)

    def fold(t):
        return F.fold(t, (2 * IH, 2 * IW), 3, padding=1, stride=2)         # block (a, b), tap (kh, kw) -> (2a - 1 + kh, 2b - 1 + kw)
    pre, S = fold(y), fold(y.abs())
    if bias is not None:
        pre, S = pre + bias.to(dt)[None, :, None, None], S + bias.to(dt).abs()[None, :, None, None]
    return pre, S


def c2_forward(c, d, dt=torch.float64, defect=None):
    pre = c2_gather(c, d["Y"], d["bias"], dt)[0]
    if defect == "tap_parity":
        pre = pre.roll(1, 2)
    xr = 1.0 / (1.0 + torch.exp(-pre)) if dt == torch.float32 else torch.sigmoid(pre)
    out = dict(xr=xr)
    if d["target"] is not None:
        OH, OW, tot, nb, kern = c2_geom(c)
        blk = c2_blocks(c)
        out.update(c2_losses(c, xr, d, dt, no_gscale=defect == "no_gscale"))
    return out


def c2_losses(c, xr, d, dt, no_gscale=False):
    OH, OW, tot, nb, kern = c2_geom(c)
    blk = c2_blocks(c)
    tgt = d["target"]
    if kern == "pix":
        dp, sse, dsum = losses_of(xr, tgt, d["gscale"], blk, nb, dt, no_gscale=no_gscale)
    else:
        dlt = xr.to(dt) - tgt.to(dt)
        dp = ((dlt if no_gscale else torch.tensor(d["gscale"], dtype=dt) * dlt) * xr.to(dt) * (1 - xr.to(dt))).permute(0, 2, 3, 1).contiguous()
        sse = by_block((dlt * dlt).reshape(-1, 1), blk, nb).reshape(-1).to(dt)
        dsum = None
    out = dict(sse=sse, sse_mean=sse.double().sum() / tot)
    if c["dpre"]:
        out["dpre"] = dp
        if kern == "pix":
            out["dsum"] = dsum
    return out


def c2_check(c, d, got, what=""):
    what = what or c["id"]
    OH, OW, tot, nb, kern = c2_geom(c)
    xr = got["xr"].detach().cpu()
    pre, S = c2_gather(c, d["Y"], d["bias"], torch.float64)
    r = _ratio((xr.double() - torch.sigmoid(pre)).abs(), sigmoid_bound(pre, S, gamma(4), lib=True))
    assert bool((r <= 1).all()), f"{what}: xr worst |err|/bound {float(r.max()):.3g}"
    res = dict(xr=float(r.max()))
    if d["target"] is None:
        return res
    blk = c2_blocks(c)
    iters = cdiv(cdiv(c["N"] * OH * OW if kern == "pix" else tot, 256), nb)       # grid-stride rounds of a thread
    if kern == "pix":
        res.update(check_losses(xr, d["target"], d["gscale"], blk, nb, got, iters * c["Cout"] + 9, iters + 9, what))
    else:
        want = c2_losses(c, xr.double(), d, torch.float64)
        if got.get("dpre") is not None:
            r = _ratio((got["dpre"].detach().cpu().double() - want["dpre"]).abs(), gamma(5) * want["dpre"].abs() + F32_MIN)
            assert bool((r <= 1).all()), f"{what}: dpre worst |err|/bound {float(r.max()):.3g}"
            res["dpre"] = float(r.max())
        if got.get("sse") is not None:
            r = _ratio((got["sse"].detach().cpu().double() - want["sse"]).abs(), gamma(iters + 6 + 4 + 3) * want["sse"] + F32_MIN)
            assert bool((r <= 1).all()), f"{what}: sse parts worst |err|/bound {float(r.max()):.3g}"
            res["sse"] = float(r.max())
    if got.get("sse_mean") is not None and got.get("sse") is not None:
        # sum_partials_k over the STORED parts: <= ceil(nb / 1024) per thread, six shuffle levels, 16 waves, the scale
        parts = got["sse"].detach().cpu().double()
        want = float(parts.sum()) / tot
        err = abs(float(got["sse_mean"]) - want)
        bnd = gamma(cdiv(nb, 1024) + 6 + 16 + 2) * want + F32_MIN
        assert err <= bnd, f"{what}: sse_mean {float(got['sse_mean'])!r} against {want!r}"
        res["sse_mean"] = err / bnd
    return res


def sb_check(g, xr, got):
    """rbvae_sigmoid_bwd_nhwc: dpre[n][h][w][c] = g[n][c][h][w] xr (1 - xr): 1 - xr and two products round once each."""
    want = (g.double() * xr.double() * (1 - xr.double())).permute(0, 2, 3, 1)
    r = _ratio((got.detach().cpu().double() - want).abs(), gamma(3) * want.abs() + F32_MIN)
    assert bool((r <= 1).all()), f"sigmoid_bwd_nhwc worst |err|/bound {float(r.max()):.3g}"
    return float(r.max())


# ---- gates over a grid (the library against the restatement) -------------------------------------------------------------

def gate_grid():
    """(library entry point, argument tuple, restated value) over shapes inside and outside every gate."""
    out = []
    for dt in ("bf16", "f32"):
        di = DTYPE_ID[dt]
        for Cin in (0, 1, 3, 4, 5):
            for (IH, IW) in ((1, 1), (15, 17), (88, 160), (0, 8), (4096, 4096)):
                for Nout in (0, 8, 12, 64, 192, 256, 264, 320, 512):
                    for N in (0, 1, 5, 128):
                        out.append(("rbvae_conv_first_fused_ok", (di, Cin, IH, IW, Nout, N), cf_shape_ok(dt, Cin, IH, IW, Nout, N)))
                        out.append(("rbvae_deconv_last_dgrad_blocks", (di, Cin, IH, IW, Nout, N), dgrad_blocks(dt, Cin, IH, IW, Nout, N)))
                        out.append(("rbvae_wgrad_first_blocks", (di, Cin, IH, IW, Nout, N), wgrad_first_blocks(dt, Cin, IH, IW, Nout, N)))
                        for cg in (0, 4, 8, 16, 32):
                            out.append(("rbvae_conv_in_ok", (di, Cin, IH, IW, Nout, N, cg), conv_in_ok(dt, Cin, IH, IW, Nout, N, cg)))
        for N in (1, 3, 4096):
            for (IH, IW) in ((1, 1), (9, 17), (44, 80), (512, 512)):
                for C1 in (0, 32, 64, 96, 128, 320, 640, 1024):
                    for Cout in (0, 1, 4, 5):
                        out.append(("rbvae_deconv_last_fused_parts", (di, N, IH, IW, C1, Cout), dl_parts(dt, N, IH, IW, C1, Cout)))
    for n_out in (0, 1, 256, 257, 4096 * 256, 4096 * 256 + 1, 1 << 33):
        out.append(("rbvae_col2im_nparts", (n_out,), col2im_nparts(n_out)))
    for (N, IH, IW, ldy, Cout) in ((2, 9, 17, 40, 4), (2, 9, 17, 48, 5), (1, 1, 1, 16, 1), (128, 128, 128, 40, 4),
                                   (2048, 256, 256, 40, 4), (4096, 128, 128, 40, 3)):
        out.append(("rbvae_col2im_has_dcol", (N, IH, IW, ldy, 2 * IH, 2 * IW, Cout), col2im_has_dcol(N, IH, IW, ldy, 2 * IH, 2 * IW, Cout)))
    for (N, H, W, Nout, cg) in ((1, 1, 1, 32, 4), (2, 9, 17, 256, 16), (3, 64, 64, 128, 8)):
        out.append(("rbvae_conv_in_stats_floats", (N, H, W, Nout, cg), conv_in_stats_floats(N, H, W, Nout, cg)))
    return out
