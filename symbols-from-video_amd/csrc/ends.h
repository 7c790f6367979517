// Shared declarations and steps of the kernels at the 3/4-channel ends of the two CNNs: conv_first_fused_k, wgrad_first_k,
// wgrad_first_wide_k (conv_first.hip), deconv_last_fused_k (deconv_last.hip), deconv_last_fwd_bwd_k (deconv_last_bwd.hip) and
// conv_in_k (conv_in.hip).  All of them give a workgroup an 8 x 16 block of pixels of one frame, and deconv_last_fwd_bwd_k
// promises the bits of deconv_last_fused_k followed by conv_first_fused_k<CIN, 1, NQ>, so the constants, tables and
// expressions they have in common are defined here, once.  Conventions as in epilogue.h: __device__ __forceinline__, values
// and plain pointers in, values out, mode branches in the kernels.  Every helper leaves every kernel instance that takes it
// text-identical to its inline form (tools/isa_diff.py); DESIGN.md ("Shared steps of the end kernels") lists the forms that did
// not, and the steps that therefore stay typed out in the kernels with a comment "(inline: mirrors ...)".
#pragma once
#include "epilogue.h"
#include <stdlib.h>
#include <type_traits>

namespace rbvae {

constexpr int EN_TA = 8, EN_TB = 16;                          // a workgroup's block of pixels
constexpr int EN_PA = 2 * EN_TA + 1, EN_PB = 2 * EN_TB + 1;   // stride 2: input patch 17 x 33
constexpr int EN_PP = EN_PB + 1;                              // its row pitch (pixels)
constexpr int EN_WROWS = 48, EN_YP = 37;                      // last deconv: rows of a V slice (9 taps x Cout, padded); Y row pitch

// ---- workgroup -> (frame, block row, block column)
__host__ __device__ __forceinline__ int en_ta_n(int rows) { return (rows + EN_TA - 1) / EN_TA; }
__host__ __device__ __forceinline__ int en_tb_n(int cols) { return (cols + EN_TB - 1) / EN_TB; }
struct EnBlk { int n, tai, tbi; };
__device__ __forceinline__ EnBlk en_blk(unsigned blk, int ta_n, int tb_n) {
    const int tbi = blk % (unsigned)tb_n; blk /= (unsigned)tb_n;
    const int tai = blk % (unsigned)ta_n;
    const int n = blk / (unsigned)ta_n;
    return EnBlk{n, tai, tbi};
}

// ---- patch offset of im2col column k = (kh*3+kw)*CIN + ci relative to the output pixel's corner; -1 = padding column.
// LAYOUT 0 keeps the patch as [ci][PA rows][PP], LAYOUT 1 as [row][PP][ci] (the order the input arrives in).
template <int CIN, int LAYOUT, int PA, int PP> struct EnOff {
    int v[64];
    constexpr EnOff() : v{} {
        for (int k = 0; k < 64; ++k) {
            const int t = k / CIN, ci = k % CIN, kh = t / 3, kw = t % 3;
            v[k] = k >= 9 * CIN ? -1 : LAYOUT == 0 ? (ci * PA + kh) * PP + kw : (kh * PP + kw) * CIN + ci;
        }
    }
};
// the three tables this one replaced, entry by entry: conv_first.hip's CfOff<CIN, MODE> (patch 17 x 34), deconv_last_bwd.hip's
// FbOff<CIN> (= CfOff<CIN, 1>) and conv_in.hip's CiOff<CIN> (patch 10 x 19, [ci][row][col])
template <int CIN, int LAYOUT, int PA, int PP> constexpr bool en_off_is(int which) {
    constexpr EnOff<CIN, LAYOUT, PA, PP> t{};
    for (int k = 0; k < 64; ++k) {
        const int q = k / CIN, ci = k % CIN, kh = q / 3, kw = q % 3;
        const int cf0 = (ci * 17 + kh) * 34 + kw, fb = (kh * 34 + kw) * CIN + ci, ci0 = (ci * 10 + kh) * 19 + kw;
        if (t.v[k] != (k >= 9 * CIN ? -1 : which == 0 ? cf0 : which == 1 ? fb : ci0)) return false;
    }
    return true;
}
#define EN_OFF_ALL(LAYOUT, PA, PP, WHICH) \
    (en_off_is<1, LAYOUT, PA, PP>(WHICH) && en_off_is<2, LAYOUT, PA, PP>(WHICH) && en_off_is<3, LAYOUT, PA, PP>(WHICH) && \
     en_off_is<4, LAYOUT, PA, PP>(WHICH))
static_assert(EN_OFF_ALL(0, EN_PA, EN_PP, 0), "EnOff<CIN, 0, 17, 34> is CfOff<CIN, 0>");
static_assert(EN_OFF_ALL(1, EN_PA, EN_PP, 1), "EnOff<CIN, 1, 17, 34> is CfOff<CIN, 1> and FbOff<CIN>");
static_assert(EN_OFF_ALL(0, 10, 19, 2), "EnOff<CIN, 0, 10, 19> is CiOff<CIN>");
#undef EN_OFF_ALL

// ---- addresses
// row of pixel (y, x) of frame n in an NHWC matrix [N*H*W][..]
__device__ __forceinline__ size_t en_pix_row(int n, int H, int W, int y, int x) { return (size_t)(n * H + y) * W + x; }
// 128-byte slice 0 of row `row` of a bf16 matrix [rows][C1], from byte sw on
__device__ __forceinline__ const unsigned char* en_row_src(const unsigned char* M, int row, int C1, int sw) {
    return M + ((size_t)row * C1) * 2 + sw;
}
// The [rows][128 B] LDS images the b128 fragment reads take (im2col rows, weight rows, d2 / V slices) keep 16-byte chunk c of
// row r at chunk c ^ ((r >> 1) & 7): its byte offset in the row (an LDS-DMA writes a row's chunks in lane order, so the lane
// swizzles its SOURCE chunk with the same expression): mma.h's swz16(r, c); ...
// ... in the image, ...
__device__ __forceinline__ int en_a_off(int r, int c) { return r * 128 + swz16(r, c); }
// ... and the offset of a lane's fragment chunk in a 32-k half: mma.h's frag_ch(kk, fg, fsw)
// a fragment by asm, at an LDS address: behind LDS-DMA in flight a C++ read would make the compiler drain all of it; the
// caller's tied s_waitcnt covers the read
__device__ __forceinline__ u32x4_t en_frag_asm(unsigned ad) {
    u32x4_t v;
    asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(ad));
    return v;
}
// acc += w x a on the matrix cores, 16 x 16 x 32 bf16: column fi of the a tile, rows 4 fg .. + 3 of the w tile
__device__ __forceinline__ f32x4_t en_mma(u32x4_t w, u32x4_t a, f32x4_t acc) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8_t*)&w, *(const bf16x8_t*)&a, acc, 0, 0, 0);
}

// ---- im2col rows: column element of offset `off` (-1: padding) of the pixel whose patch corner is `corner`, as bf16, ...
__device__ __forceinline__ unsigned short en_col_elem(const float* s_patch, int corner, int off) {
    const float v = off >= 0 ? s_patch[corner + max(off, 0)] : 0.f;
    return f32_to_bf16(v);
}
// ... and two of them as one word, the lower column in the low half
__device__ __forceinline__ unsigned en_pack2(unsigned short lo, unsigned short hi) { return (unsigned)lo | ((unsigned)hi << 16); }

// ---- column sums of a block's stored values through the LDS scratch red [pixel groups][64 NQ]: column tid over the groups
// (two wave halves for NQ = 4, eight waves for NQ = 1), fixed order
template <int NQ> __device__ __forceinline__ float en_colsum_total(const float* red, int tid) {
    constexpr int RW = 64 * NQ, NGRP = NQ == 4 ? 2 : 8;
    float t = red[tid];
#pragma unroll
    for (int g2 = 1; g2 < NGRP; ++g2) t += red[g2 * RW + tid];
    return t;
}

// ---- the last deconv's forward epilogue (deconv_last_fused_k and deconv_last_fwd_bwd_k: the same expressions, the same bits)
// hardware exp2 / rcp (about 1 ulp each; these kernels are the bf16-storage path)
__device__ __forceinline__ float en_sigmoid(float v) { return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * v)); }
// d(loss)/d(pre-sigmoid) from d = sigmoid - target
__device__ __forceinline__ float en_dpre(float gscale, float d, float sg) { return gscale * d * sg * (1.f - sg); }
// the four waves' partial sums of slot k (squared error, then the four column sums of dpre), fixed order
__device__ __forceinline__ float en_red5_total(const float (*red5)[5], int k) {
    return ((red5[0][k] + red5[1][k]) + red5[2][k]) + red5[3][k];
}

// (wgrad_first_k / wgrad_first_wide_k take the transposing fragment reads of their [128 px][128 B] tr-swizzled LDS images from
// mma.h: tr_off<128>, tr_frag)

// ---- host
// output extent of the 3x3 stride-2 pad-1 convolution (= input extent of the transposed one)
static inline int ends_out_dim(int in) { return (in + 2 - 3) / 2 + 1; }
// workgroups of a launch over N frames of rows x cols pixels
static inline int en_blocks(int N, int rows, int cols) { return N * cdiv(rows, EN_TA) * cdiv(cols, EN_TB); }
// the instantiation for Cin = 1 .. 4 (the shape checks come first): f(std::integral_constant<int, CIN>{})
template <typename F> static inline auto en_for_cin(int Cin, F&& f) {
    switch (Cin) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        default: return f(std::integral_constant<int, 4>{});
    }
}
// rows of the per-tap product matrix V that the last deconv of the wrapper `who` stages: 9 taps x Cout, padded by the caller
static inline int en_check_nyp(const char* who, int NYP, int Cout) {
    RBVAE_CHECK_ARG(NYP >= 9 * Cout && NYP <= EN_WROWS, "%s: NYP=%d", who, NYP);
    return RBVAE_OK;
}

}  // namespace rbvae
