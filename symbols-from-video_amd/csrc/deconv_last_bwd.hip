// The last ConvTranspose2d(C1 -> Cout <= 4, k3 s2 p1 op1) + Sigmoid + recon_loss of the decoder AND the layer's input
// gradient as ONE kernel (bf16 storage): rbvae_deconv_last_fused (deconv_last.hip) followed by
// rbvae_deconv_last_dgrad_fused (conv_first.hip, MODE 1) on the same 8 x 16 block of d2 pixels, with d2 read once and
// d(loss)/d(pre-sigmoid) handed over in LDS.  Every stored value and every partial sum is the one the two launches leave:
// same MFMA chains, same expressions, same thread -> pixel map inside a sum slot, same slots.
//
//   a workgroup (8 waves) owns the d2 pixels a0 .. a0+7 x b0 .. b0+15 of one frame.  The input gradient of pixel (r, c)
//   reads dpre at the output pixels 2r-1 .. 2r+1 x 2c-1 .. 2c+1, the forward of output pixel (oh, ow) reads d2 at
//   (oh+1-kh)/2: the block stages the 10 x 18 d2 pixels a0-1 .. a0+8 x b0-1 .. b0+16 (channel slice by slice through two
//   buffers; the second half needs only the sign of the block's own pixels, kept as gate bits) and forms
//   Y[pixel][(tap, co)] for all of them.  Waves 0-3 run the forward
//   epilogue of the block's own 16 x 32 output pixels exactly as deconv_last_fused_k does (x_recon, squared error, dpre and
//   their sums: each output pixel once, from the block that owns it); waves 4-7 recompute dpre on the 49-pixel rim (output
//   row 2 a0 - 1, output column 2 b0 - 1) beside them, for the patch only.  No flags, no atomics, nothing read that
//   another workgroup writes.
//   Then conv_first_fused_k<MODE 1>'s steps on the 17 x 33 patch of dpre: im2col rows (to LDS and, when asked for, to
//   `col`), 128 x C1 x 64 on the matrix cores, scale, gate (the bits), dd2 as 16-byte chunks of NHWC rows,
//   column sums of the stored values.
//   The steps this kernel has in common with those two are ends.h's (block decode, offset table, swizzles, fragment reads,
//   MFMA, sigmoid and dpre, the fixed-order sums); where a step is typed out here although the other kernel has it too, the
//   comment "(inline: mirrors ...)" names the copy, and DESIGN.md ("Shared steps of the end kernels") says which forms of a
//   helper changed a listing.
//
// LDS (dynamic; KS = C1 / 64 slices, NBUF = 2 slice buffers (1 for C1 = 64), NQ = 4 for C1 > 64 else 1):
//   [0, NBUF*30720)                   d2 tile slice [NBUF][192][128 B] + V slice [NBUF][48][128 B], swizzled 16-byte chunks
//                                     ->  Y [192][37] f32 (28416)  ->  im2col rows [128][128 B] + W [64 NQ][128 B]
//   [.., + 9248)                      dpre patch [17][34][Cout] f32 (zeroed first); the column-sum scratch at the end
//   [.., + 128 * C1 / 16 * 2)         gate bits [128 px][C1 / 16] u16: d2 > 0 of the block's own pixels, taken from the
//                                     slices as they pass -- all that the second half needs of d2, so the tile itself need
//                                     not stay: C1 = 256: 74784 bytes + 80 static, TWO workgroups per CU (all of C1 resident,
//                                     156704 bytes, one per CU: 29.9 us for the bench shape's launch against 13.8 + 16.0 of
//                                     the two kernels); C1 = 64: 40992 bytes.
// Registers (compiler's resource report, __launch_bounds__(512, 4) = two workgroups per CU): 128 vector registers for C1 > 64,
// 117-123 for C1 = 64, no scratch, no spills.  Barriers behind global stores are lds_barrier() (LDS only): with
// __syncthreads() every one of them waited for the x_recon / dpre / col / dd2 stores in flight (23.3 -> 21.7 us at the bench
// shape; DESIGN.md 5, profiles/deconv_last_bwd_ab.txt).
#include "ends.h"
#include <stdlib.h>

namespace rbvae {

struct FbArgs {
    const unsigned char* D2;     // [N*IH*IW][C1] bf16
    const unsigned char* V;      // [NYP][C1] bf16, row = tap*Cout + co
    const unsigned char* W;      // [C1][64] bf16, column (kh*3+kw)*Cout + co
    const float* bias;           // [Cout]
    const unsigned char* zero;   // >= 16 zero bytes
    float* xr;                   // [N][Cout][OH][OW]
    const float* target;         // frames through tfm
    FrameMap tfm;
    float* ws;                   // [blocks] squared-error sums, then [blocks][4] column sums of dpre
    float* dpre;                 // [N][OH][OW][Cout]
    unsigned char* col;          // [N*IH*IW][64] bf16 im2col rows of dpre, or null
    unsigned char* dd2;          // [N*IH*IW][C1] bf16
    float* colsum_ws;            // [blocks][C1] column sums of the stored dd2
    float gscale, gs;
    int N, IH, IW, C1, NYP;
};

constexpr int FB_HB = EN_TB + 2;                        // staged tile 10 x 18
constexpr int FB_PIX = (EN_TA + 2) * FB_HB;             // 180
constexpr int FB_MROWS = 192;
constexpr int FB_PATCH_BYTES = 4 * EN_PA * EN_PP * 4;
constexpr int FB_RIM = EN_PB + 2 * EN_TA;               // 49

// slice buffers (two for a layer of several slices), over them later Y and then the im2col rows + W
static size_t fb_region(int C1) {
    const int NBUF = C1 > 64 ? 2 : 1, NQ = C1 > 64 ? 4 : 1;
    size_t b = (size_t)NBUF * (FB_MROWS + EN_WROWS) * 128;
    if (b < (size_t)FB_MROWS * EN_YP * 4) b = (size_t)FB_MROWS * EN_YP * 4;
    if (b < (size_t)16384 + NQ * 8192) b = (size_t)16384 + NQ * 8192;
    return b;
}
static size_t fb_lds(int C1) { return fb_region(C1) + FB_PATCH_BYTES + (size_t)128 * (C1 / 16) * 2; }

template <int CIN, int NQ> __global__ __launch_bounds__(512, 4) void deconv_last_fwd_bwd_k(const FbArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ float red5[4][5];
    constexpr int Cout = CIN;
    constexpr int MT = NQ == 4 ? 4 : 1;
    const int KS = p.C1 >> 6;
    constexpr int NBUF = NQ == 4 ? 2 : 1;                                    // NQ == 1: one slice in all
    constexpr int REGION = (NBUF * (FB_MROWS + EN_WROWS) * 128 > FB_MROWS * EN_YP * 4) ? NBUF * (FB_MROWS + EN_WROWS) * 128
                                                                                      : FB_MROWS * EN_YP * 4;
    static_assert(REGION >= 16384 + NQ * 8192, "the im2col rows and W take the slices' place");
    unsigned char* s_pix = smem;                                             // [NBUF][FB_MROWS][128]
    unsigned char* s_wts = smem + NBUF * FB_MROWS * 128;                     // [NBUF][EN_WROWS][128]
    float* s_y = (float*)smem;                                               // [FB_MROWS][EN_YP], once the slices are dead
    unsigned char* s_a = smem;                                               // [128][128], once Y is dead
    unsigned char* s_b = smem + 16384;                                       // [64 NQ][128]
    float* s_patch = (float*)(smem + REGION);                                // [17][34][CIN]
    unsigned short* s_gate = (unsigned short*)(smem + REGION + FB_PATCH_BYTES);   // [128 px][C1 / 16]: bit j = d2[px][16 g + j] > 0
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int OH = 2 * p.IH, OW = 2 * p.IW;
    const int tb_n = en_tb_n(p.IW), ta_n = en_ta_n(p.IH);
    const EnBlk bk = en_blk(blockIdx.x, ta_n, tb_n);
    const int n = bk.n, a0 = bk.tai * EN_TA, b0 = bk.tbi * EN_TB;

    // the input gradient's weight, through registers: asked for first (the oldest loads of the wave:
    // landed long before the counted waits below), written to LDS once Y is dead (its place)
    // (inline: mirrors the row permutation of conv_first_fused_k's weight tile)
    u32x4_t wreg[NQ];
#pragma unroll
    for (int it = 0; it < NQ; ++it) {
        const int idx = it * 512 + tid;
        const int r = idx >> 3, sc = idx & 7;
        const int ct = r >> 4, j = r & 15;
        const int ch = 64 * (ct >> 2) + 16 * (j >> 2) + 4 * (ct & 3) + (j & 3);
        wreg[it] = *(const u32x4_t*)(ch < p.C1 ? p.W + (size_t)ch * 128 + swz16(r, sc) : p.zero);
    }
    // the patch starts as zeros: output pixels outside the image and channels never written read as padding
    for (int i = tid; i < FB_PATCH_BYTES / 4; i += 512) s_patch[i] = 0.f;

    // ---- epilogue operands that depend on nothing, asked for first: waves 0-3 the two output pixels a thread owns, waves 4-7
    // one rim pixel (inline: mirrors deconv_last_fused_k's prefetch, with the rim arm)
    constexpr int EPI = (2 * EN_TA * 2 * EN_TB) / 256;
    const int OHW = OH * OW;
    float tg[EPI][4], bz[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) bz[c] = (p.bias && c < Cout) ? p.bias[c] : 0.f;
    int rim_oh = -1, rim_ow = -1, rim_pos = 0;
    if (w >= 4) {
        const int j = tid - 256;
        if (j < EN_PB) { rim_oh = 2 * a0 - 1; rim_ow = 2 * b0 - 1 + j; rim_pos = j; }
        else if (j < FB_RIM) { rim_oh = 2 * a0 + (j - EN_PB); rim_ow = 2 * b0 - 1; rim_pos = (j - EN_PB + 1) * EN_PP; }
        if (rim_oh >= OH || rim_ow >= OW || rim_ow < 0) rim_oh = -1;
    }
#pragma unroll
    for (int it = 0; it < EPI; ++it) {
        const int q = tid + 256 * it;
        int oh = 2 * a0 + q / (2 * EN_TB), ow = 2 * b0 + q % (2 * EN_TB);
        bool ok = oh < OH && ow < OW;
        if (w >= 4) { oh = rim_oh; ow = rim_ow; ok = it == 0 && rim_oh >= 0; }
        const float* tp = p.target + (ok ? frame_off_u32(p.tfm, n) + (long)oh * OW + ow : 0);
#pragma unroll
        for (int c = 0; c < 4; ++c) tg[it][c] = (ok && c < Cout) ? tp[(long)c * OHW] : 0.f;
    }

    // ---- stage d2 tile + V slice by slice (double buffer, slice s + 1 in flight under slice s's MFMAs): 30 LDS-DMA
    // instructions of 8 rows per slice, q = w, w + 8, ... (inline: mirrors deconv_last_fused_k's piece table and slice loop; the
    // tile here has a halo on all four sides and eight waves share it)
    const int srow = lane >> 3, schunk = lane & 7;
    const int fi = lane & 15, fg = lane >> 4;
    const int fsw = (fi >> 1) & 7;
    constexpr int PIX_I = FB_MROWS / 8, WTS_I = EN_WROWS / 8;
    const unsigned char* psrc[4];
    unsigned pinc[4], pdst[4], pstep[4];
    {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int q = w + 8 * i;
            const bool is_w = q >= PIX_I;
            const int r = (is_w ? q - PIX_I : q) * 8 + srow;
            const int sw = swz16(r, schunk);
            const unsigned char* src = p.zero;
            unsigned inc = 0;
            if (is_w) {
                if (r < p.NYP) { src = en_row_src(p.V, r, p.C1, sw); inc = 128; }
            } else if (r < FB_PIX) {
                const int la = r / FB_HB, lb = r - la * FB_HB;
                const int a = a0 - 1 + la, b = b0 - 1 + lb;
                if (a >= 0 && a < p.IH && b >= 0 && b < p.IW) {
                    src = en_row_src(p.D2, (n * p.IH + a) * p.IW + b, p.C1, sw); inc = 128;
                }
            }
            psrc[i] = src; pinc[i] = inc;
            pdst[i] = (unsigned)((is_w ? (size_t)(s_wts - smem) : 0) + (size_t)(r - srow) * 128);
            pstep[i] = is_w ? EN_WROWS * 128 : FB_MROWS * 128;
        }
    }
    auto stage = [&](int s, int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (w + 8 * i < PIX_I + WTS_I) glds16(psrc[i] + (size_t)(pinc[i] * (unsigned)s), smem + pdst[i] + pstep[i] * (unsigned)buf);
    };
    static_assert(PIX_I + WTS_I == 30, "waves 0-5 issue 4 pieces per slice, waves 6, 7 issue 3");
    // the gate of the second half, taken from the slices as they pass: thread = (owned pixel tid / 4, 16-channel group tid % 4)
    const int gpx = tid >> 2, ggrp = tid & 3;
    const int gtr = ((gpx >> 4) + 1) * FB_HB + (gpx & 15) + 1;
    const unsigned lds_gate = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)s_gate;

    // ---- Y = pixels x V^T: wave w takes pixel tile w + 4 and, waves 0-3, tile w; all three (tap, co) tiles
    f32x4_t acc[2][3];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) acc[a][b] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    const unsigned lds_pix = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)s_pix;
    const unsigned lds_wts = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)s_wts;
    stage(0, 0);
    for (int s = 0; s < KS; ++s) {
        const int buf = s & (NBUF - 1);
        if (s + 1 < KS) {
            stage(s + 1, buf ^ 1);
            // slice s landed for this wave (its pieces of slice s + 1 stay in flight), then the workgroup barrier
            if (w < 6) wait_vm_lgkm_barrier<4>();
            else wait_vm_lgkm_barrier<3>();
        } else {
            wait_vm_lgkm_barrier<0>();
        }
        u32x4_t gq[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const unsigned ad = lds_pix + (unsigned)((buf * FB_MROWS + gtr) * 128 + (((2 * ggrp + h) ^ ((gtr >> 1) & 7)) * 16));
            gq[h] = en_frag_asm(ad);
        }
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const int ch = frag_ch(kk, fg, fsw);
            u32x4_t wf[3], pf[2];
#pragma unroll
            for (int rt = 0; rt < 3; ++rt) wf[rt] = en_frag_asm(lds_wts + (unsigned)((buf * EN_WROWS + rt * 16 + fi) * 128 + ch));
#pragma unroll
            for (int pi = 0; pi < 2; ++pi) {
                const int pt = pi == 0 ? w + 4 : (w & 3);                     // waves 4-7 have no second tile: read, not used
                pf[pi] = en_frag_asm(lds_pix + (unsigned)((buf * FB_MROWS + pt * 16 + fi) * 128 + ch));
            }
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(wf[0]), "+v"(wf[1]), "+v"(wf[2]), "+v"(pf[0]), "+v"(pf[1]), "+v"(gq[0]), "+v"(gq[1]));
#pragma unroll
            for (int pi = 0; pi < 2; ++pi) {
                if (pi == 0 || w < 4) {
#pragma unroll
                    for (int rt = 0; rt < 3; ++rt)
                        acc[pi][rt] = en_mma(wf[rt], pf[pi], acc[pi][rt]);
                }
            }
        }
        {
            // a bf16 pattern g is > 0 (NaN excluded) iff (g - 1) mod 2^16 < 0x7f80: the test of conv_first_fused_k's gate, as bits
            unsigned bits = 0;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const unsigned wd = gq[j >> 2][j & 3];
                bits |= (((wd & 0xffffu) - 1u) & 0xffffu) < 0x7f80u ? 1u << (2 * j) : 0u;
                bits |= (((wd >> 16) - 1u) & 0xffffu) < 0x7f80u ? 2u << (2 * j) : 0u;
            }
            const unsigned ad = lds_gate + (unsigned)((gpx * (KS * 4) + s * 4 + ggrp) * 2);
            asm volatile("ds_write_b16 %0, %1" ::"v"(ad), "v"(bits) : "memory");
        }
        // everyone is done reading this buffer (every read above was waited for): slice s + 2 may land in it
        if (s + 2 < KS) asm volatile("s_barrier" ::: "memory");
    }
#pragma unroll
    for (int it = 0; it < EPI; ++it)
#pragma unroll
        for (int c = 0; c < 4; ++c) asm volatile("" : "+v"(tg[it][c]));
#pragma unroll
    for (int c = 0; c < 4; ++c) asm volatile("" : "+v"(bz[c]));
#pragma unroll
    for (int it = 0; it < NQ; ++it) asm volatile("" : "+v"(wreg[it]));
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the gate bits this wave wrote
    __syncthreads();                     // every wave has read its last fragments: the products go where the slices were
    // D[(tap,co) row 4g + r][pixel i] (inline: mirrors deconv_last_fused_k's Y store)
#pragma unroll
    for (int pi = 0; pi < 2; ++pi) {
        const int pt = pi == 0 ? w + 4 : w;
        if (pi == 0 || w < 4) {
#pragma unroll
            for (int rt = 0; rt < 3; ++rt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int wr = rt * 16 + 4 * fg + r;
                    if (wr < 36) s_y[(pt * 16 + fi) * EN_YP + wr] = acc[pi][rt][r];
                }
        }
    }
    __syncthreads();

    // ---- forward epilogue.  Waves 0-3: the block's 16 x 32 output pixels (same thread -> pixel map, same order of additions),
    // dpre also into the patch.  Waves 4-7: dpre of the rim pixels, the same expressions.
    // (inline: mirrors deconv_last_fused_k's loop -- tap gather, stores, sum terms -- with the rim arm; the sigmoid, dpre and the
    // five-sum total are ends.h's)
    const long plane = (long)OH * OW;
    float sse = 0.f, dsum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int it = 0; it < EPI; ++it) {
        const int q = tid + 256 * it;
        const int oy = q / (2 * EN_TB), ox = q - oy * (2 * EN_TB);
        int oh = 2 * a0 + oy, ow = 2 * b0 + ox;
        int ppos = (oy + 1) * EN_PP + ox + 1;
        if (w >= 4) {
            if (it > 0 || rim_oh < 0) continue;
            oh = rim_oh; ow = rim_ow; ppos = rim_pos;
        }
        if (oh >= OH || ow >= OW) continue;
        float v[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = bz[c];
        for (int kh = (oh + 1) & 1; kh < 3; kh += 2) {
            const int a = (oh + 1 - kh) >> 1;
            if (a < 0 || a >= p.IH) continue;
            for (int kw = (ow + 1) & 1; kw < 3; kw += 2) {
                const int b = (ow + 1 - kw) >> 1;
                if (b < 0 || b >= p.IW) continue;
                const float* yp = s_y + ((a - a0 + 1) * FB_HB + (b - b0 + 1)) * EN_YP + (kh * 3 + kw) * Cout;
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (c < Cout) v[c] += yp[c];
            }
        }
        const size_t xo = (size_t)n * Cout * plane + (size_t)oh * OW + ow;
        float d4[4] = {0.f, 0.f, 0.f, 0.f}, sg[4];
#pragma unroll
        for (int c = 0; c < 4; ++c)
            sg[c] = en_sigmoid(v[c]);
        if (w < 4) {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c < Cout) p.xr[xo + (size_t)c * plane] = sg[c];
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (c >= Cout) break;
            const float d = sg[c] - tg[it][c];
            // deconv_last_fused_k's chain: one fused multiply-add per term, in this order (the opaque use keeps the
            // compiler from regrouping the chain into packed operations)
            sse = __builtin_fmaf(d, d, sse);
            asm volatile("" : "+v"(sse));
            d4[c] = en_dpre(p.gscale, d, sg[c]);
        }
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (c < Cout) s_patch[ppos * CIN + c] = d4[c];
        if (w < 4) {
            float* dp = p.dpre + ((size_t)(n * OH + oh) * OW + ow) * Cout;
            if (Cout == 4) *(float4*)dp = make_float4(d4[0], d4[1], d4[2], d4[3]);
            else
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (c < Cout) dp[c] = d4[c];
#pragma unroll
            for (int c = 0; c < 4; ++c) dsum[c] += d4[c];
        }
    }
    {
        float vals[5] = {sse, dsum[0], dsum[1], dsum[2], dsum[3]};
        if (w < 4) {
#pragma unroll
            for (int k = 0; k < 5; ++k) vals[k] = wave_sum(vals[k]);
            if (lane == 0) {
#pragma unroll
                for (int k = 0; k < 5; ++k) red5[w][k] = vals[k];
            }
        }
        lds_barrier();                   // also: the patch is complete and Y is dead (LDS only: the stores drain behind it)
        if (tid < 5) {
            const float t = en_red5_total(red5, tid);
            if (tid == 0) p.ws[blockIdx.x] = t;
            else p.ws[gridDim.x + 4 * blockIdx.x + (tid - 1)] = t;
        }
    }

    // ---- input gradient: the steps of conv_first_fused_k<CIN, 1, NQ> from here on, its operands already on chip
#pragma unroll
    for (int it = 0; it < NQ; ++it) *(u32x4_t*)(s_b + (size_t)(it * 512 + tid) * 16) = wreg[it];
    static constexpr EnOff<CIN, 1, EN_PA, EN_PP> otab{};
    int koff[8];
#pragma unroll
    for (int k8 = 0; k8 < 8; ++k8) koff[k8] = otab.v[(tid & 7) * 8 + k8];
    // im2col rows: 128 rows x 8 chunks of 8 columns (inline: mirrors conv_first_fused_k's row build; elements, pack and the
    // swizzled offset are ends.h's)
#pragma unroll
    for (int i0 = 0; i0 < 128 * 8; i0 += 512) {
        const int i = i0 + tid;
        const int r = i >> 3, c = i & 7;
        const int oy = r >> 4, ox = r & 15;
        const int corner = (2 * oy * EN_PP + 2 * ox) * CIN;
        unsigned short e[8];
#pragma unroll
        for (int k8 = 0; k8 < 8; ++k8) e[k8] = en_col_elem(s_patch, corner, koff[k8]);
        u32x4_t pk;
        pk[0] = en_pack2(e[0], e[1]); pk[1] = en_pack2(e[2], e[3]);
        pk[2] = en_pack2(e[4], e[5]); pk[3] = en_pack2(e[6], e[7]);
        *(u32x4_t*)(s_a + en_a_off(r, c)) = pk;
        const int a = a0 + oy, b = b0 + ox;
        if (p.col && a < p.IH && b < p.IW)
            *(u32x4_t*)(p.col + ((size_t)(n * p.IH + a) * p.IW + b) * 128 + c * 16) = pk;
    }
    lds_barrier();

    // 128 x 64 NQ x 64 on the matrix cores: wave w owns pixels 16 MT (w / NQ) .. x the channel quad w % NQ
    // (inline: mirrors conv_first_fused_k's block; the chunk offset and the MFMA are ends.h's)
    const int wq = NQ == 4 ? (w & 3) : 0, wm = NQ == 4 ? (w >> 2) : w;
    const int col = 64 * wq + 16 * fg;
    const bool first = col < p.C1, second = col + 8 < p.C1;
    f32x4_t dacc[MT][4];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int h = 0; h < 4; ++h) dacc[mt][h] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        const int ch = frag_ch(kk, fg, fsw);
        u32x4_t wv[4], av[MT];
#pragma unroll
        for (int h = 0; h < 4; ++h) wv[h] = *(const u32x4_t*)(s_b + ((4 * wq + h) * 16 + fi) * 128 + ch);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) av[mt] = *(const u32x4_t*)(s_a + ((MT * wm + mt) * 16 + fi) * 128 + ch);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int h = 0; h < 4; ++h)
                dacc[mt][h] = en_mma(wv[h], av[mt], dacc[mt][h]);
    }
    // epilogue from registers: lane = pixel fi of tile mt, channels 64*wq + 16*fg .. +15 (two 16-byte chunks); the gate is
    // the 16 bits of (pixel, channel group 4 wq + fg)
    float csum[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) csum[e] = 0.f;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int r = (MT * wm + mt) * 16 + fi;
        const int oy = r >> 4, ox = r & 15;
        const int a = a0 + oy, b = b0 + ox;
        if (a >= p.IH || b >= p.IW || !first) continue;
        const size_t orow = (size_t)(n * p.IH + a) * p.IW + b;
        const unsigned gbits = s_gate[r * (KS * 4) + 4 * wq + fg];
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            if (half == 1 && !second) break;
            u32x4_t val;
            // the rounded product where the gate bit is set, +0 elsewhere (conv_first_fused_k multiplies by 0 or 1)
            typedef float v2f __attribute__((ext_vector_type(2)));
            typedef __bf16 v2b __attribute__((ext_vector_type(2)));
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const f32x4_t a4 = dacc[mt][2 * half + (e >> 1)];
                const v2f x = v2f{a4[2 * (e & 1)], a4[2 * (e & 1) + 1]} * p.gs;
                const v2b rr = __builtin_convertvector(x, v2b);
                const unsigned b2 = gbits >> (8 * half + 2 * e);
                const unsigned mask = ((b2 & 1u) ? 0xffffu : 0u) | ((b2 & 2u) ? 0xffff0000u : 0u);
                val[e] = *(const unsigned*)&rr & mask;
            }
            *(u32x4_t*)(p.dd2 + (orow * p.C1 + col + 8 * half) * 2) = val;
#pragma unroll
            for (int e = 0; e < 8; ++e)
                csum[8 * half + e] += __uint_as_float((e & 1) ? (val[e >> 1] & 0xffff0000u) : (val[e >> 1] << 16));
        }
    }
    {
        // bias gradient of the layer below: column sums of this block's stored values, pixels then wave groups
        // (inline: mirrors conv_first_fused_k's row sums and scratch writes; the total is ends.h's)
        float* red = s_patch;                                  // the patch is dead since the last barrier
        constexpr int RW = 64 * NQ;
#pragma unroll
        for (int e = 0; e < 16; ++e) csum[e] = row_sum(csum[e]);
        if (fi == 0) {
#pragma unroll
            for (int e = 0; e < 16; ++e) red[wm * RW + col + e] = csum[e];
        }
        lds_barrier();
        if (tid < p.C1) {
            const float t = en_colsum_total<NQ>(red, tid);
            p.colsum_ws[(size_t)blockIdx.x * p.C1 + tid] = t;
        }
    }
}

// 0: the fused launch where it covers the shape; 1: rbvae_deconv_last_fwd_bwd_ok answers 0 (the callers take the two
// launches).  Written only by librbvae_dbg's rbvae_dbg_deconv_last_variant (include/rbvae_dbg_variants.h).
int deconv_last_variant = 0;

static int fb_shape_ok(int dtype, int N, int IH, int IW, int C1, int Cout) {
    if (dtype != RBVAE_BF16 || Cout < 1 || Cout > 4 || C1 % 64 || C1 < 64 || C1 > 256 || N < 1 || IH < 1 || IW < 1) return 0;
    if (fb_lds(C1) > 160 * 1024 - 256) return 0;
    if ((long)N * 2 * IH * 2 * IW * Cout >= (1l << 31) || (long)N * IH * IW * 256 >= (1l << 31)) return 0;
    return 1;
}

}  // namespace rbvae

using namespace rbvae;

extern "C" int rbvae_deconv_last_fwd_bwd_ok(int dtype, int N, int IH, int IW, int C1, int Cout) {
    return deconv_last_variant == 1 ? 0 : fb_shape_ok(dtype, N, IH, IW, C1, Cout);
}

extern "C" int rbvae_deconv_last_fwd_bwd(int dtype, const void* D2, const void* V, int NYP, const void* W, const float* bias,
                                         const void* zero_page, int N, int IH, int IW, int C1, int Cout, float* xr,
                                         const float* target, int fd1, int fd2, long fs0, long fs1, long fs2, float* ws,
                                         float* dpre, float gscale, void* col, void* dd2, float gs, float* colsum_ws,
                                         void* stream) {
    RBVAE_CHECK_ARG(D2 && V && W && zero_page && xr && target && ws && dpre && dd2 && colsum_ws, "deconv_last_fwd_bwd: null pointer");
    RBVAE_CHECK_ARG(fb_shape_ok(dtype, N, IH, IW, C1, Cout),
                    "deconv_last_fwd_bwd: shape outside the fused kernel (bf16, Cout <= 4, C1 %% 64 == 0, C1 <= 256): N=%d %dx%d "
                    "C1=%d Cout=%d", N, IH, IW, C1, Cout);
    if (const int e = en_check_nyp("deconv_last_fwd_bwd", NYP, Cout)) return e;
    RBVAE_CHECK_ARG(((uintptr_t)D2 | (uintptr_t)V | (uintptr_t)W | (uintptr_t)zero_page | (uintptr_t)dpre | (uintptr_t)col |
                     (uintptr_t)dd2) % 16 == 0, "deconv_last_fwd_bwd: pointers must be 16-byte aligned");
    FbArgs a;
    a.D2 = (const unsigned char*)D2; a.V = (const unsigned char*)V; a.W = (const unsigned char*)W; a.bias = bias;
    a.zero = (const unsigned char*)zero_page; a.xr = xr; a.target = target; a.tfm = FrameMap{fd1, fd2, fs0, fs1, fs2};
    a.ws = ws; a.dpre = dpre; a.col = (unsigned char*)col; a.dd2 = (unsigned char*)dd2; a.colsum_ws = colsum_ws;
    a.gscale = gscale; a.gs = gs; a.N = N; a.IH = IH; a.IW = IW; a.C1 = C1; a.NYP = NYP;
    const int blocks = en_blocks(N, IH, IW);
    const size_t lds = fb_lds(C1);
    const int rc = en_for_cin(Cout, [&](auto cin) -> int {
        constexpr int CIN = decltype(cin)::value;
        const auto launch = [&](auto nq) -> int {
            constexpr int NQ = decltype(nq)::value;
            if (const int e = lds_attr_grow<deconv_last_fwd_bwd_k<CIN, NQ>>("deconv_last_fwd_bwd", lds)) return e;
            hipLaunchKernelGGL((deconv_last_fwd_bwd_k<CIN, NQ>), dim3(blocks), dim3(512), lds, (hipStream_t)stream, a);
            return RBVAE_OK;
        };
        return C1 > 64 ? launch(std::integral_constant<int, 4>{}) : launch(std::integral_constant<int, 1>{});
    });
    if (rc != RBVAE_OK) return rc;
    RBVAE_CHECK_LAUNCH("deconv_last_fwd_bwd");
    return RBVAE_OK;
}
