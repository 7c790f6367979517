// The store epilogue shared by the convolution-type GEMM kernels (gather_gemm_k, deconv_halo_k, conv_s2_k): the three are
// picked by shape and must produce the same values element for element, so the steps are defined once, here.
//
// Conventions (the same in every kernel that takes these helpers):
//   * register phase: epi_act (accumulator + bias, ReLU, scale), then four values go to the LDS tile as one f32x4 /
//     bf16x4 group (epi_stage);
//   * store phase, per 16-byte chunk of EC = 16 / sizeof(T) elements, in THIS order:
//       dropout -> addend -> ReLU gate -> store -> column sum;
//   * keyed dropout: the chunk's element index is  orow * Nout + col  (the logical width Nout, NOT the pitch ldo), the key
//     is epi_drop_key(seed, seed_dev) and an element is dropped iff its 16 bits are below
//     thresh16 = drop_thresh >> 16;  explicit dropout reads the u8 keep-mask at the same index;
//   * the gate keeps an element iff elem_pos<T> of the saved activation (> 0, NaN excluded);
//   * the column sums add the values as STORED (after dropout, addend and gate), read back from the chunk.
//
// Rule for the device helpers, found by compiling: they take VALUES and return VALUES.  A helper that writes through a
// pointer or reference to the calling lane's locals (u32x4_t& val, T* ev, float (&bz)[4]) or takes the kernel's args struct
// by const reference changes the register allocation and the branch forms of the kernels; the forms below leave the
// listings text-identical (tools/isa_diff.py).  For the same reason the mode branches -- if (p.drop_mode == 1) .. else if
// (.. == 2), if (p.addend), if (p.gate), if (p.colsum_ws) -- stay in the kernel, around the calls.  Identical is decided per
// kernel instance: where some instance changes with every form tried, that kernel keeps the step as inline text, with a
// comment naming the helper and the instance (DESIGN.md lists these sites).  A new kernel starts from the helpers.
//
// Host part: epi_drop_args, the dropout argument check and threshold of the C-ABI wrappers; epi_check_rows and its halves,
// their pitch / alignment check (also the halo stride-1 wrappers').
#pragma once
#include "mma.h"

namespace rbvae {

// ---- host -----------------------------------------------------------------------------------------------------------
// Dropout arguments of the wrapper named `who`: drop_mode 0 none / 1 keyed / 2 explicit keep-mask.  Sets the message
// behind rbvae_last_error() and returns its code on a bad argument, else writes floor(drop_p * 2^32) to *drop_thresh.
static inline int epi_drop_args(const char* who, int drop_mode, const void* mask, float drop_p, unsigned* drop_thresh) {
    RBVAE_CHECK_ARG(drop_mode >= 0 && drop_mode <= 2 && (drop_mode != 2 || mask), "%s: drop_mode/mask", who);
    RBVAE_CHECK_ARG(drop_mode != 1 || (drop_p >= 0 && drop_p < 1), "%s: drop_p=%g outside [0, 1)", who, (double)drop_p);
    *drop_thresh = (unsigned)((double)drop_p * 4294967296.0);
    return RBVAE_OK;
}
// Row pitches and pointer alignment of the wrapper named `who` (ptrs: every pointer of the call OR-ed together).  Two halves,
// called one by one where a wrapper has other checks between them (a caller sees the messages in the old order), and both.
static inline int epi_check_pitch(const char* who, int ES, int Kc, int Nout, int lda, int ldo) {
    RBVAE_CHECK_ARG(lda >= Kc && ((long)lda * ES) % 16 == 0 && ldo >= Nout && ((long)ldo * ES) % 16 == 0,
                    "%s: leading dimensions lda=%d ldo=%d", who, lda, ldo);
    return RBVAE_OK;
}
static inline int epi_check_align(const char* who, uintptr_t ptrs) {
    RBVAE_CHECK_ARG(ptrs % 16 == 0, "%s: pointers must be 16-byte aligned", who);
    return RBVAE_OK;
}
static inline int epi_check_rows(const char* who, int ES, int Kc, int Nout, int lda, int ldo, uintptr_t ptrs) {
    if (const int e = epi_check_pitch(who, ES, Kc, Nout, lda, ldo)) return e;
    return epi_check_align(who, ptrs);
}

// ---- device ---------------------------------------------------------------------------------------------------------
// the launch's seed with the optional device step counter mixed in
__device__ __forceinline__ unsigned long long epi_seed(unsigned long long seed, const unsigned long long* seed_dev) {
    return seed + (seed_dev ? seed_dev[0] * 0x9E3779B97F4A7C15ull : 0ull);
}
// the keyed-dropout key of a launch (computed under the kernel's own `if (p.drop_mode == 1)`: with the branch inside, the
// listing of conv_s2_k changed)
__device__ __forceinline__ DropKey epi_drop_key(unsigned long long seed, const unsigned long long* seed_dev) {
    return drop_key(epi_seed(seed, seed_dev));
}

// register phase: one accumulator element
__device__ __forceinline__ float epi_act(float acc, float bias, int relu, float scale) {
    float x = acc + bias;
    if (relu) x = fmaxf(x, 0.f);
    return x * scale;
}

// two f32 -> one word of two bf16 (the lower index in the low half)
__device__ __forceinline__ unsigned pack_bf16x2(float a, float b) {
    return (unsigned)f32_to_bf16(a) | ((unsigned)f32_to_bf16(b) << 16);
}
// four consecutive channels of one pixel -> the LDS tile (dst: 16-byte aligned for f32, 8-byte for bf16)
template <typename T> __device__ __forceinline__ void epi_stage(unsigned char* dst, float v0, float v1, float v2, float v3) {
    if constexpr (sizeof(T) == 4) {
        *(float4*)dst = make_float4(v0, v1, v2, v3);
    } else {
        uint2 pk;
        pk.x = pack_bf16x2(v0, v1);
        pk.y = pack_bf16x2(v2, v3);
        *(uint2*)dst = pk;
    }
}

// store phase: keyed dropout of the chunk whose first element has index idx
template <typename T>
__device__ __forceinline__ u32x4_t epi_keyed(u32x4_t val, DropKey k, unsigned thresh16, unsigned long long idx) {
    const unsigned run = drop_run(k, idx);
    if constexpr (sizeof(T) == 2) drop_chunk_zero_b16<8>(run, thresh16, (unsigned*)&val);
    else drop_chunk_zero_f32<4>(run, thresh16, (float*)&val);
    return val;
}
// explicit dropout: mk = the chunk's first keep byte
template <typename T> __device__ __forceinline__ u32x4_t epi_masked(u32x4_t val, const unsigned char* mk) {
    T* ev = (T*)&val;
#pragma unroll
    for (int e = 0; e < (int)(16 / sizeof(T)); ++e)
        if (!mk[e]) ev[e] = 0;
    return val;
}
// ReLU gate: g = the saved activation's chunk
template <typename T> __device__ __forceinline__ u32x4_t epi_gate(u32x4_t val, u32x4_t g) {
    T* ev = (T*)&val;
#pragma unroll
    for (int e = 0; e < (int)(16 / sizeof(T)); ++e)
        if (!elem_pos<T>((const unsigned char*)&g, e)) ev[e] = 0;
    return val;
}
// column sums: csum[0 .. EC) += the chunk as stored.  csum is the lane's own array -- the one exception to the rule above:
// conv_s2_k changes with the value form (a kernel loop over csum[e] += <element e of val as f32>) and stays identical with
// this one.  f32 instances of the other two kernels change with it, so they keep the loop (see their sites).
template <typename T> __device__ __forceinline__ void epi_csum(u32x4_t val, float* csum) {
    const T* ev = (const T*)&val;
#pragma unroll
    for (int e = 0; e < (int)(16 / sizeof(T)); ++e) csum[e] += Elem<T>::load(ev + e);
}

}  // namespace rbvae
