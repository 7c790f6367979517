// Shared device helpers of the matrix-core kernels (gfx950 only): vector types, the LDS-DMA wrapper, the LDS-only and
// counted-vmcnt barriers, DPP row sums, static_for, the MFMA dispatch, the tied wait and MFMA group of a 32-k half, the
// 128-byte-row swizzle, the store-phase roles, the transposing-read swizzle, lane offset and fragment pack, the ReLU-gate test
// and the frame map.  Everything is __forceinline__: a kernel that takes a helper from here compiles to the code it had
// with a private copy (tools/isa_diff.py proves it).  New kernels take these; they do not copy them.
#pragma once
#include "common.h"
#include <type_traits>

namespace rbvae {

typedef __attribute__((ext_vector_type(8))) short bf16x8_t;
typedef __attribute__((ext_vector_type(4))) short s16x4_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4_t;

// LDS-DMA: 16 bytes per lane from global memory straight into LDS (counted by vmcnt)
__device__ __forceinline__ void glds16(const void* g, void* lds) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                     (__attribute__((address_space(3))) void*)lds, 16, 0, 0);
}

// workgroup barrier that orders LDS traffic only.  __syncthreads() also waits vmcnt(0): behind global stores or LDS-DMA in
// flight every barrier then costs a full memory round trip.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Counted waits in front of the workgroup barrier: all but the N youngest vector-memory operations of THIS wave (the
// LDS-DMA of the slice about to be read) have landed; no vmcnt(0) drain, so younger slices stay in flight across the barrier.
// Two forms; the question is whether the wave's OWN LDS writes must have landed before the barrier:
//   wait_vm_barrier       no: everything the other waves will read arrived by LDS-DMA, which vmcnt counts
//                         (attn_flash_db_k, conv_s2_k, wgrad_row_k, wgrad_halo_k: no ds_write feeds another wave);
//   wait_vm_lgkm_barrier  yes: the wave also filled LDS with ds_write (register-staged patches, gather-index and row
//                         tables), which lgkmcnt counts, not vmcnt.
// An existing kernel keeps the form it was measured and ISA-checked with.
template <int N> __device__ __forceinline__ void wait_vm_barrier() {
    asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(N) : "memory");
}
template <int N> __device__ __forceinline__ void wait_vm_lgkm_barrier() {
    asm volatile("s_waitcnt vmcnt(%0)\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier" ::"n"(N) : "memory");
}

template <int CTRL> __device__ __forceinline__ float dpp(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
// sum over the 16 lanes of a DPP row (lane & 15), every lane gets the total
__device__ __forceinline__ float row_sum(float v) {
    v += dpp<0x128>(v);     // row_ror:8
    v += dpp<0x124>(v);     // row_ror:4
    v += dpp<0x4E>(v);      // quad_perm [2,3,0,1]
    v += dpp<0xB1>(v);      // quad_perm [1,0,3,2]
    return v;
}

// f(integral_constant<int, I>{}) for I in [I, N): a loop whose index is a constant expression in the body
template <int I, int N, typename F> __device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

// Workgroup lin of a one-dimensional grid -> work item: workgroups are dealt to the 8 XCDs round-robin by id, and XCD x walks
// the x-th contiguous eighth of the items (neighbouring items share an L2).  Bijective for any total.
__device__ __forceinline__ int xcd_item(int lin, int total) {
    const int xcd = lin & 7, q = total >> 3, r = total & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (lin >> 3);
}

// acc += rowop x colop over one 16-byte fragment per lane of both operands
template <typename T> struct Mma;
template <> struct Mma<bf16_t> {
    // one 128-B LDS row slice = 64 k: two 32-k MFMAs, lane group g reads chunk 4*kk+g
    static __device__ __forceinline__ void run(f32x4_t& acc, const u32x4_t& rowop, const u32x4_t& colop) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8_t*)&rowop, *(const bf16x8_t*)&colop, acc,
                                                      0, 0, 0);
    }
};
template <> struct Mma<float> {
    // 32 k per row slice; lane group g holds k = 16*kk + 4*g + c for MFMA c (same on both operands)
    static __device__ __forceinline__ void run(f32x4_t& acc, const u32x4_t& rowop, const u32x4_t& colop) {
        const f32x4_t r = *(const f32x4_t*)&rowop, c = *(const f32x4_t*)&colop;
#pragma unroll
        for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(r[q], c[q], acc, 0, 0, 0);
    }
};

// One 32-k half of a K step in registers: MT + NT fragments read by inline-asm ds_read_b128, which the compiler's wait-count
// pass does not see.  frag_landed<YOUNGER>(fa, fb) is the counted wait that guards them: at most YOUNGER LDS operations issued
// after them are still outstanding (in-order return), and the "+v" ties keep every use of a fragment behind the wait
// (tools/check_tr_asm.py and the build's ISA check prove that nothing touches one between its read and its wait).  One operand
// list per pair of array extents in use: a new tile shape adds its overload here.
template <int YOUNGER> __device__ __forceinline__ void frag_landed(u32x4_t (&fa)[2], u32x4_t (&fb)[2]) {
    asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(fa[0]), "+v"(fa[1]), "+v"(fb[0]), "+v"(fb[1]) : "n"(YOUNGER));
}
template <int YOUNGER> __device__ __forceinline__ void frag_landed(u32x4_t (&fa)[2], u32x4_t (&fb)[4]) {
    asm volatile("s_waitcnt lgkmcnt(%6)" : "+v"(fa[0]), "+v"(fa[1]), "+v"(fb[0]), "+v"(fb[1]), "+v"(fb[2]), "+v"(fb[3]) : "n"(YOUNGER));
}
template <int YOUNGER> __device__ __forceinline__ void frag_landed(u32x4_t (&fa)[4], u32x4_t (&fb)[1]) {
    asm volatile("s_waitcnt lgkmcnt(%5)" : "+v"(fa[0]), "+v"(fa[1]), "+v"(fa[2]), "+v"(fa[3]), "+v"(fb[0]) : "n"(YOUNGER));
}
template <int YOUNGER> __device__ __forceinline__ void frag_landed(u32x4_t (&fa)[4], u32x4_t (&fb)[2]) {
    asm volatile("s_waitcnt lgkmcnt(%6)" : "+v"(fa[0]), "+v"(fa[1]), "+v"(fa[2]), "+v"(fa[3]), "+v"(fb[0]), "+v"(fb[1]) : "n"(YOUNGER));
}
template <int YOUNGER> __device__ __forceinline__ void frag_landed(u32x4_t (&fa)[4], u32x4_t (&fb)[4]) {
    asm volatile("s_waitcnt lgkmcnt(%8)"
                 : "+v"(fa[0]), "+v"(fa[1]), "+v"(fa[2]), "+v"(fa[3]), "+v"(fb[0]), "+v"(fb[1]), "+v"(fb[2]), "+v"(fb[3])
                 : "n"(YOUNGER));
}
// the MFMAs of rows M0 .. M1 - 1 of a wave's MT x NT block of 16 x 16 tiles (weights fb as the row operand: a lane owns 4
// consecutive output channels of one pixel); mma_group: the whole block
template <typename T, int M0, int M1, int MT, int NT>
__device__ __forceinline__ void mma_rows(f32x4_t (&acc)[MT][NT], const u32x4_t (&fa)[MT], const u32x4_t (&fb)[NT]) {
#pragma unroll
    for (int mt = M0; mt < M1; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) Mma<T>::run(acc[mt][nt], fb[nt], fa[mt]);
}
template <typename T, int MT, int NT>
__device__ __forceinline__ void mma_group(f32x4_t (&acc)[MT][NT], const u32x4_t (&fa)[MT], const u32x4_t (&fb)[NT]) {
    mma_rows<T, 0, MT>(acc, fa, fb);
}

// byte offset of 16-byte chunk c in row r of an LDS image of 128-byte rows: the chunk index XORed with (r >> 1) & 7, on the
// source address of the LDS-DMA that fills the image and again on the ds_read_b128 fragment read (conflict-free)
__device__ __forceinline__ int swz16(int r, int c) { return (c ^ ((r >> 1) & 7)) * 16; }
// ... of a lane's fragment chunk in 32-k half kk: chunk 4 kk + fg of row fi, with fsw = (fi >> 1) & 7 formed by the caller
// (formed inside, the kernels' listings change)
__device__ __forceinline__ int frag_ch(int kk, int fg, int fsw) { return ((4 * kk + fg) ^ fsw) * 16; }

// the roles of a GEMM's store phase: the BM x BN tile of T goes through LDS (row pitch PITCH) and leaves as 16-byte chunks,
// CPR per row; thread tid takes chunk tid % CPR of rows it * RL + tid / CPR, it < ITERS
template <typename T, int BN, int THREADS, int BM> struct StoreRoles {
    static constexpr int PITCH = BN * (int)sizeof(T) + 16;
    static constexpr int CPR = BN / (16 / (int)sizeof(T));
    static constexpr int RL = THREADS / CPR;
    static constexpr int ITERS = BM / RL;
};

// XOR applied to the 16-B chunk index of an LDS image row (RB bytes per row) so that the transposed
// reads of a 32-lane half (rows {q, 8+q} or {4+q, 12+q}) hit distinct banks.
template <int RB> __device__ __forceinline__ int tr_swz(int row) {
    if constexpr (RB >= 256) return ((row & 3) | (((row >> 3) & 1) << 2)) << 1;   // 8 chunk pairs
    else return (((row >> 1) & 1) | (((row >> 3) & 1) << 1)) << 1;                // 128-B rows: 4 pairs
}

// Transposing fragment reads (ds_read_b64_tr_b16) of an image whose ROW is the reduction index: lane (fg, q, pp) = (lane >> 4,
// (lane & 15) >> 2, lane & 3) addresses row 8 fg + q (+ 4 for the second read), elements 4 pp .. + 3 of a 16-column sub-tile.
// The lane's byte offset, two forms because no single one leaves every taker's listing alone ("Shared steps of the
// weight-gradient kernels"):
//   tr_off_swz  image at byte 0, sub-tile `tile`, chunks swizzled by tr_swz<RB>(row) (wgrad_gemm_k's and wgrad_row_k's first
//               operand, both wgrad_first kernels);
//   tr_off      image at byte `base`; `chunk` = (tile * 2 + (pp >> 1)) ^ swizzle is formed at the call (second operands and
//               patches with a swizzle of their own; wgrad_halo_k's S tile).  tr_off_swz written as a call of tr_off changes
//               the wgrad_first kernels, so it spells the sum out.
// tr_frag: the 32-k MFMA operand from the two reads.
template <int RB> __device__ __forceinline__ int tr_off(int base, int row, int chunk, int pp) { return base + row * RB + chunk * 16 + (pp & 1) * 8; }
template <int RB> __device__ __forceinline__ int tr_off_swz(int row, int tile, int pp) {
    return row * RB + (((tile * 2 + (pp >> 1)) ^ tr_swz<RB>(row)) * 16) + (pp & 1) * 8;
}
__device__ __forceinline__ bf16x8_t tr_frag(s16x4_t lo, s16x4_t hi) {
    return bf16x8_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// ReLU gate: element e of a stored activation is > 0 (NaN excluded)
template <typename T> __device__ __forceinline__ bool elem_pos(const unsigned char* p, int e);
template <> __device__ __forceinline__ bool elem_pos<float>(const unsigned char* p, int e) {
    return ((const float*)p)[e] > 0.f;
}
template <> __device__ __forceinline__ bool elem_pos<bf16_t>(const unsigned char* p, int e) {
    const bf16_t v = ((const bf16_t*)p)[e];
    return (v & 0x8000u) == 0 && (v & 0x7fffu) != 0 && (v & 0x7fffu) <= 0x7f80u;
}

// Frame n of a batch -> element offset of its first value.  d1 == 0: n * s2.  Otherwise n is read as the
// mixed-radix number (n / d1, (n % d1) / d2, n % d2) with strides (s0, s1, s2): the fused trainer runs both
// views of an item batch [B][2][T] as frames v*(B*T) + b*T + t without first copying them into that order.
struct FrameMap {
    int d1, d2;
    long s0, s1, s2;
};
template <typename I> __device__ __forceinline__ I frame_off(const FrameMap& f, I n) {
    if (f.d1 == 0) return n * (I)f.s2;
    const I a = n / (I)f.d1, r = n - a * (I)f.d1;
    const I b = r / (I)f.d2, c = r - b * (I)f.d2;
    return a * (I)f.s0 + b * (I)f.s1 + c * (I)f.s2;
}
// the same offset with the divisions in 32 bits and the products in 64 (the fused end kernels: one frame per workgroup)
__device__ __forceinline__ long frame_off_u32(const FrameMap& f, unsigned n) {
    if (f.d1 == 0) return (long)n * f.s2;
    const unsigned a = n / (unsigned)f.d1, r = n - a * (unsigned)f.d1;
    const unsigned b = r / (unsigned)f.d2, c = r - b * (unsigned)f.d2;
    return (long)a * f.s0 + (long)b * f.s1 + (long)c * f.s2;
}

}  // namespace rbvae
