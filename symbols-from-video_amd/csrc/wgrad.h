// Shared steps of the weight-gradient kernels wgrad_gemm_k (wgrad_gemm.hip), wgrad_row_k (wgrad_row.hip) and wgrad_halo_k
// (wgrad_halo.hip): the lane decode, the slice-major XCD order of the workgroups, the slab layout, the LDS-DMA pieces and
// stage bodies of wgrad_gemm_k's two staging arms, and the host checks of the two 3x3 wrappers.  mma.h's conventions:
// everything on the device is __forceinline__, takes values and plain pointers, and a kernel takes a helper only where its
// listing stays what it was (tools/isa_diff.py); DESIGN.md ("Shared steps of the weight-gradient kernels") lists what stayed
// inline and why.  The transposing-read offset and fragment pack are mma.h's (tr_off, tr_off_swz, tr_frag).
#pragma once
#include "mma.h"

namespace rbvae {

// ---- lane (fi, fg) = (lane & 15, lane >> 4) of a 16 x 16 MFMA tile; (q, pp) = (fi >> 2, fi & 3) of a transposing read
// (mma.h: tr_off).  The MFMA waves' decode (wr, wc) = (w >> 2, w & 3) stays in the kernels: as a helper it changes their listings.
struct WgLane { int fi, fg, q, pp; };
__device__ __forceinline__ WgLane wg_lane(int lane) {
    const int fi = lane & 15;
    return {fi, lane >> 4, fi >> 2, fi & 3};
}

// ---- workgroup lin of a grid of 8 * per workgroups, per = ceil(total / 8) -> item of `total` (K-slice, tile) items in
// slice-major order: workgroups are dealt to the 8 XCDs round-robin by id, and XCD x takes items x per .. x per + per - 1, so
// its workgroups share one or a few pixel slices in that XCD's L2.  Not mma.h's xcd_item: here the last XCDs' surplus
// workgroups are not live and exit (uniformly, before any barrier).  Placement is a speed matter only.
struct WgItem { int item; bool live; };
__device__ __forceinline__ WgItem wg_item(unsigned lin, int total) {
    const int per = (total + 7) >> 3;
    const int x = lin & 7, q = lin >> 3;
    const int item = x * per + q;
    return {item, !(q >= per || item >= total)};
}

// ---- slab layout [ks][a][taps][b] f32: K-slice ks's slab, and the element offset of a lane's 16-byte store in it
__device__ __forceinline__ float* wg_slab(float* dW, int ks, int Ca, int taps, int Cb) { return dW + (size_t)ks * Ca * taps * Cb; }
__device__ __forceinline__ size_t wg_slab_off(int a, int taps, int tap, int Cb, int b) { return ((size_t)a * taps + tap) * Cb + b; }

// ---- one LDS-DMA piece (64 lanes x 16 bytes = 1 KiB = 1024 / RB rows) of wgrad_gemm_k's images with RB-byte rows of ES-byte
// elements, the same for the pieces w N + i of the 8-wave form and pw + 4 j of the producer waves: the lane's image row, the
// 16-byte source chunk its image chunk `lane % (RB / 16)` holds (XORed by tr_swz when SWZ), and whether that chunk's channels
// c0 + .. lie below C.  (One struct-returning wg_piece holds in the producer arm and changes the twelve 8-wave instances.)
template <int RB> __device__ __forceinline__ int wg_piece_row(int piece, int lane) { return piece * (1024 / RB) + lane / (RB / 16); }
template <int RB, bool SWZ> __device__ __forceinline__ int wg_piece_chunk(int row, int lane) { return (lane % (RB / 16)) ^ (SWZ ? tr_swz<RB>(row) : 0); }
template <int ES> __device__ __forceinline__ bool wg_piece_cval(int c0, int chunk, int C) { return c0 + chunk * (16 / ES) < C; }

// the Dy pieces of one stage: piece j goes to la + j * STEP from the wave's current row (the zero row where the channel chunk or
// the pixel base + row[j] lies outside), and the row pointer moves one K step on
template <int N, int STEP>
__device__ __forceinline__ void wg_stage_rows(unsigned char* la, const unsigned char** cur, const bool* cval, const int* row, int base, int npix,
                                              size_t stride, const unsigned char* zero) {
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const bool v = cval[j] && base + row[j] < npix;
        glds16(v ? cur[j] : zero, la + j * STEP);
        cur[j] += stride;
    }
}
// the gathered In pieces of one stage: piece j goes to lb + j * STEP from row s_idx[base + row[j]] of the wave's chunk column
// (the zero row where the channel chunk lies outside or the index is negative).  AHEAD: all of the stage's indices are read
// first, so no LDS wait sits between the pieces (the producer waves; the 8-wave form reads each index in front of its piece)
template <int N, int STEP, bool AHEAD>
__device__ __forceinline__ void wg_stage_gather(unsigned char* lb, const unsigned char* const* colbase, const bool* cval, const int* row,
                                                const int* s_idx, int base, size_t ld_b, const unsigned char* zero) {
    int src[N];
    if constexpr (AHEAD) {
#pragma unroll
        for (int j = 0; j < N; ++j) src[j] = s_idx[base + row[j]];
    }
#pragma unroll
    for (int j = 0; j < N; ++j) {
        if constexpr (!AHEAD) src[j] = s_idx[base + row[j]];
        const bool v = cval[j] && src[j] >= 0;
        glds16(v ? colbase[j] + (size_t)src[j] * ld_b : zero, lb + j * STEP);
    }
}
// ---- host: the two 3x3 stride-2 kernels (rbvae_wgrad3x3s2_row: 128 x 128 channel tiles, rbvae_wgrad3x3s2_halo: 64 x 64)
static inline int wg3x3_ok(int tile, int dtype, int Nimg, int OH, int OW, int Ca, int Cb) {
    return dtype == RBVAE_BF16 && Nimg >= 1 && OH >= 1 && OW >= 1 && Ca >= tile && Cb >= tile && Ca % tile == 0 && Cb % tile == 0 &&
           (long)Nimg * OH * OW * 4 < (1l << 31);       /* pixel rows; the byte sizes are checked against the leading dimensions at launch */
}
// the argument checks their wrappers share, in the wrappers' order; `name` is the wrapper's name without the rbvae_ prefix
static inline int wg3x3_check(const char* name, int tile, int dtype, const void* S, const void* G, const float* dW_slabs, const void* zero_page,
                              int Nimg, int OH, int OW, int Ca, int Cb, int lds_, int ldg) {
    RBVAE_CHECK_ARG(S && G && dW_slabs && zero_page, "%s: null pointer", name);
    RBVAE_CHECK_ARG(wg3x3_ok(tile, dtype, Nimg, OH, OW, Ca, Cb), "%s: shape not covered (dtype %d, %d x %d x %d, %d x %d channels): "
                    "query rbvae_%s_ok", name, dtype, Nimg, OH, OW, Ca, Cb, name);
    RBVAE_CHECK_ARG(lds_ >= Ca && ldg >= Cb && lds_ % 8 == 0 && ldg % 8 == 0, "%s: leading dimensions lds=%d ldg=%d", name, lds_, ldg);
    RBVAE_CHECK_ARG(((uintptr_t)S | (uintptr_t)G | (uintptr_t)dW_slabs | (uintptr_t)zero_page) % 16 == 0,
                    "%s: pointers must be 16-byte aligned", name);
    return RBVAE_OK;
}

}  // namespace rbvae
