// Shared declarations of the halo-resident 3x3 stride-1 convolution kernels (conv_halo.hip: one tile per workgroup, f32 and
// the debug comparison; conv_halo_ws.hip: persistent workgroups with producer / MFMA wave roles, bf16).
#pragma once
#include "mma.h"
#include <stdlib.h>
#include <type_traits>

namespace rbvae {

struct ChArgs {
    const unsigned char* A;        // [Nimg*IH*IW][lda] T
    const unsigned char* W;        // [Nout][9][Kc] T
    unsigned char* Out;            // [Nimg*OH*OW][ldo] T
    const float* bias;             // [Nout] or null
    const unsigned char* addend;   // [Nimg*OH*OW][ldo] T or null (residual)
    const unsigned char* zero;     // >= 128 zero bytes
    const float* gn_scale;         // [Nimg][Kc] or null: input -> swish?(x * scale + shift) while staging
    const float* gn_shift;
    float* stats;                  // null or [m tiles][Nout / cg] float2 (mean, M2) of the stored tile per group
    int gn_swish, stats_cg;        // channels per group of the output statistics
    int Nimg, IH, IW, OH, OW, dh0, dw0;
    int Kc, Nout, lda, ldo;
    int tiles_r, tiles_c, ntn, total;
};

constexpr int CH_BM = 256, CH_BN = 128, CH_T = 16;          // tile: 16 x 16 pixels x 128 channels
constexpr int CH_PW = CH_T + 2, CH_NSLOT = CH_PW * CH_PW;    // 18 x 18 patch
constexpr int CH_NSLOT_PAD = 336;                             // multiple of 16
constexpr int CH_PLANE = CH_NSLOT_PAD * 16;                   // bytes per chunk plane
constexpr int CH_KKOFF = 4 * CH_PLANE + 64;                   // chunk 4kk+fg = kk * KKOFF + fg part
constexpr int CH_ABUF = 8 * CH_PLANE + 128;                   // 43136: one patch image (planes + staggers)
constexpr int CH_BBYTES = CH_BN * 128;
constexpr int CH_NA = 6;                                      // register-staged 16-B pieces per thread and slice

__device__ __forceinline__ unsigned ch_plane_off(int chunk) { return (unsigned)(chunk * CH_PLANE + (chunk >> 1) * 32); }

// conv_halo_ws.hip: the persistent bf16 kernel (covers = operands below 2 GiB: 32-bit buffer offsets)
bool ch_ws_covers(const ChArgs& a);
int launch_ch_ws(const ChArgs& a, hipStream_t st);

}  // namespace rbvae
