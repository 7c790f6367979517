// Shared declarations and steps of the halo-resident 3x3 stride-1 kernels: conv_halo_k (conv_halo.hip: one tile per workgroup;
// f32, and bf16 launches of fewer than 512 tiles or outside ch_ws_covers), conv_halo_ws_k (conv_halo_ws.hip: persistent
// workgroups with producer / MFMA wave roles; bf16 launches of at least 512 tiles with Kc % 64 == 0, Nout <= 512 and operands
// below 2 GiB) and upconv_halo_k (upconv.hip: the parity-folded Upsample).  The three share tile geometry and LDS images, and
// the first two promise the same bits, so each step below exists once.  Conventions as in epilogue.h: __device__
// __forceinline__, values and plain pointers in, values out (register arrays by reference where tools/isa_diff.py showed the
// listings unchanged), mode branches and ablation switches in the kernels.  Every helper leaves every kernel instance that takes
// it text-identical to its inline form; DESIGN.md lists the forms that did not and the steps that therefore stay inline.
#pragma once
#include "epilogue.h"
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

constexpr int CH_MT = 4, CH_NTW = 4;                         // 16 x 16 MFMA tiles per wave: 64 pixels x 64 channels
constexpr int CH_LOADS = 2;                                   // weight LDS-DMA instructions per wave and step (8 waves)

// chunk plane `chunk` of a patch image whose planes hold `plane` bytes (+ a 32-byte stagger per chunk pair); deconv_halo_k's
// planes depend on its strip geometry
__device__ __forceinline__ unsigned ch_plane_off(int chunk, int plane = CH_PLANE) { return (unsigned)(chunk * plane + (chunk >> 1) * 32); }

// ---- staging of conv_halo_k and upconv_halo_k (512 threads).  Patch: piece i of a thread = (slot (tid >> 3) + 64 i, chunk
// tid & 7): 8 lanes read one pixel's 128-byte slice (coalesced) and write it to 8 chunk planes.
// source pixel row of piece i from the slot table: -1 = zeros (padding), -2 = no such slot (SPP slots per staging pass of a
// table of NSLOT: deconv_halo_k's depend on its waves and strip geometry)
template <int SPP = 64, int NSLOT = CH_NSLOT_PAD> __device__ __forceinline__ int ch_piece_pix(const int* s_pix, int tid, int i) {
    const int slot = (tid >> 3) + SPP * i;
    return slot < NSLOT ? s_pix[slot] : -2;
}
// the 16 bytes of slice kc a piece loads: chunk `chunk` of pixel row pv, or of the zero page
template <int ES>
__device__ __forceinline__ const unsigned char* ch_piece_src(const unsigned char* A, int pv, int lda, int kc, int chunk,
                                                             const unsigned char* zsrc) {
    return pv >= 0 ? A + ((size_t)pv * lda) * ES + (size_t)kc * 128 + chunk * 16 : zsrc;
}
// ... loaded by asm (the compiler would drain the weight tiles' LDS-DMA in front of a load of its own); the destination stays
// untouched until the counted wait that covers it (ch_a_landed: the build's ISA check proves it)
__device__ __forceinline__ u32x4_t ch_piece_load(const unsigned char* src) {
    u32x4_t v;
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(v) : "v"(src) : "memory");
    return v;
}
// the six pieces have landed: at most YOUNGER vector-memory operations are still outstanding
template <int YOUNGER> __device__ __forceinline__ void ch_a_landed(u32x4_t (&ar)[CH_NA]) {
    asm volatile("s_waitcnt vmcnt(%6)" : "+v"(ar[0]), "+v"(ar[1]), "+v"(ar[2]), "+v"(ar[3]), "+v"(ar[4]), "+v"(ar[5]) : "n"(YOUNGER));
}
// Weights (LDS-DMA): instruction i of wave w moves rows (w * 2 + i) * 8 .. + 7 of a tap tile [128 co][128 B].  Source = a
// uniform base (tile, tap, slice: scalar registers) + this 32-bit per-lane offset (row r, swizzled chunk): with per-tap 64-bit
// lane pointers the unrolled slice body kept 18 of them live and spilled.  TAPS = tap tiles per output channel in W.
template <int ES, int TAPS> __device__ __forceinline__ unsigned ch_blane(int r, int schunk, int Kc) {
    return (unsigned)(r * TAPS * Kc) * ES + (unsigned)swz16(r, schunk);
}
// tap tile J of slice kc in W (wtile: the workgroup's first tap tile)
template <int ES, int J> __device__ __forceinline__ const unsigned char* ch_tap_src(const unsigned char* wtile, int Kc, int kc) {
    return wtile + ((size_t)J * Kc) * ES + (size_t)kc * 128;
}
// ... -> lb, this wave's rows of the tile's ring slot
__device__ __forceinline__ void ch_tile_issue(const unsigned char* src, const unsigned (&blane)[CH_LOADS], unsigned char* lb) {
#pragma unroll
    for (int i = 0; i < CH_LOADS; ++i) glds16(src + blane[i], lb + i * 1024);
}

// ---- fragment reads and MFMA groups (inside the slice loops: every caller's listing is text-identical to its inline form)
// LDS address of a lane's patch fragments: chunk plane fg of patch buffer 0; the caller adds its slot (row * CH_PW + column) * 16
__device__ __forceinline__ unsigned ch_aplane(unsigned lds0, int fg, int plane = CH_PLANE) {
    return lds0 + (unsigned)fg * plane + (unsigned)(fg >> 1) * 32;
}
// ... and of its weight fragment in ring slot 0: row `row` of the tap tile, 16-byte chunk `chunk` (swizzled by the caller:
// XOR (fi >> 1) & 7)
__device__ __forceinline__ unsigned ch_boff(unsigned lds0, int row, int chunk) {
    return lds0 + 2 * CH_ABUF + (unsigned)row * 128 + (unsigned)(chunk * 16);
}
// patch read address of slice kc: its buffer folded in
__device__ __forceinline__ unsigned ch_slice_addr(unsigned abase, int kc) { return abase + (unsigned)((kc & 1) * CH_ABUF); }
// One 32-k half of a step: CH_MT + CH_NTW fragment reads (inline asm, counted waits: see gather_gemm.hip).  The tap's shift of
// the patch (AOFF) and a static ring slot (BOFF) are immediate offsets of the reads; rs = a run-time ring slot's offset.
template <int AOFF, int BOFF>
__device__ __forceinline__ void ch_read_half(const unsigned (&ta)[CH_MT], unsigned ab, unsigned rs, u32x4_t (&fa)[CH_MT],
                                             u32x4_t (&fb)[CH_NTW]) {
#pragma unroll
    for (int mt = 0; mt < CH_MT; ++mt)
        asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(fa[mt]) : "v"(ta[mt]), "n"(AOFF));
    const unsigned ab_ = ab + rs;
#pragma unroll
    for (int nt = 0; nt < CH_NTW; ++nt)
        asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(fb[nt]) : "v"(ab_), "n"(BOFF + nt * 2048));
}
// (their counted wait and the 4 x 4 MFMA group are mma.h's frag_landed<YOUNGER> and mma_group<T>)

// ---- epilogue
// two accumulators + bias -> one word of two bf16 (the lower index in the low half).  The sums are formed HERE: with epilogue.h's
// pack_bf16x2 on sums formed by the caller both additions move in front of both conversions (conv_halo_k's bf16 instances change).
__device__ __forceinline__ unsigned ch_bias_pack2(float a0, float b0, float a1, float b1) {
    return (unsigned)f32_to_bf16(a0 + b0) | ((unsigned)f32_to_bf16(a1 + b1) << 16);
}

// store phase, per 16-byte chunk of an NHWC row (orow < 0: the tile row is outside the image): the residual's chunk (a row
// outside reads row 0: the value is not stored), and the guarded store.  The addition between them stays inline in the kernels.
template <int ES> __device__ __forceinline__ u32x4_t ch_addend_chunk(const unsigned char* addend, int orow, int ldo, int scol) {
    return *(const u32x4_t*)(addend + ((size_t)(orow < 0 ? 0 : orow) * ldo + scol) * ES);
}
template <int ES> __device__ __forceinline__ void ch_store_chunk(unsigned char* Out, int orow, int ldo, int scol, u32x4_t val) {
    if (orow >= 0) *(u32x4_t*)(Out + ((size_t)orow * ldo + scol) * ES) = val;
}

// ---- host
// bytes of the staging buffers (two patch images + RING weight tiles) / the epilogue tile of conv_halo_k and upconv_halo_k (the
// statistics scratch reuses the tile); the pixel tables follow
template <typename T, int RING> constexpr int ch_lds_main() {
    constexpr int ring = 2 * CH_ABUF + RING * CH_BBYTES;
    constexpr int epi = CH_BM * (CH_BN * (int)sizeof(T) + 16);
    return ring > epi ? ring : epi;
}

// conv_halo_ws.hip: the persistent bf16 kernel (covers: operands below 2 GiB -- 32-bit buffer offsets --, Kc % 64 == 0,
// Nout <= 512, a statistics group within one wave's lanes)
bool ch_ws_covers(const ChArgs& a);
int launch_ch_ws(const ChArgs& a, hipStream_t st);

}  // namespace rbvae
