// The steps that the six wavefront LSTM kernels of lstm.hip repeat (lstm_fwd_wave_k, lstm_pair_fwd_k, lstm_pair_fwd_unit_k,
// lstm_bwd_wave_k, lstm_pair_bwd_k, lstm_pair_bwd_unit_k).  The kernels promise bit-identical results, so each step has
// ONE definition, here; only lstm.hip includes this header.
//
// Conventions (those of epilogue.h): helpers take values and plain pointers and return values (a small struct where a
// step has several results); the mode branches -- if (acts), if (p.cast_out), if (p.kl_parts), if (p.dz), if (row),
// q == layers - 1 -- stay in the kernels, around the calls.  Whether a helper may replace a kernel's text is decided per
// kernel instance by tools/isa_diff.py, and every helper here leaves every listing text-identical.  The once-per-launch
// steps (weight rows, input staging, slab sums, the BPTT staging prologue, the KL tail) changed listings in every form
// tried and did not pass the timing check: they stay typed out in the kernels, each copy naming the one it mirrors.
// DESIGN.md lists which kernel takes which helper and every step left inline.
#pragma once
#include "mma.h"

namespace rbvae {

typedef __attribute__((ext_vector_type(2))) float f32x2_t;

// sigmoid / tanh on the hardware exp2 and reciprocal (about 1 ulp each): the wavefront kernels sit on a
// short dependent chain where the library expf/tanhf sequences would dominate.
__device__ __forceinline__ float fast_sigmoid(float x) {
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * x));
}
__device__ __forceinline__ float fast_tanh(float x) {
    return 2.0f * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-2.8853900817779268f * x)) - 1.0f;
}

// ---- the cast copy: a stack's output once more in the next GEMM's operand type, rows of cast_ld elements ---------------
__device__ __forceinline__ void lstm_cast_store(void* __restrict__ cast_out, int cast_bf16, long o, float v) {
    if (cast_bf16) ((bf16_t*)cast_out)[o] = f32_to_bf16(v); else ((float*)cast_out)[o] = v;
}
// Zero the padding columns [L, cast_ld) of sequence s's T rows (the consumer GEMM reads whole 128-byte K slices), by all
// threads of the workgroup.  Called under the kernel's own `if (cast_out)`: with the null test in here every listing changed.
__device__ __forceinline__ void lstm_cast_pad(void* __restrict__ cast_out, int cast_bf16, int cast_ld, int s, int T, int L) {
    const int pw = cast_ld - L;
    for (int i = threadIdx.x; i < T * pw; i += blockDim.x) {
        const long o = ((long)s * T + i / pw) * cast_ld + L + i % pw;
        if (cast_bf16) ((bf16_t*)cast_out)[o] = 0; else ((float*)cast_out)[o] = 0.f;
    }
}

// ---- forward ---------------------------------------------------------------------------------------------------------
// The cell update.  The fma is explicit: the same rounding wherever this cell runs, whatever the compiler would contract.
struct LstmCell { float c, h; };
__device__ __forceinline__ LstmCell lstm_cell(float ig, float fg, float gg, float og, float c) {
    LstmCell r;
    r.c = fmaf(fg, c, ig * gg);
    r.h = og * fast_tanh(r.c);
    return r;
}

// The seam, forward: bin_code (common.h, shared with the binarise kernels of losses.hip) on the encoder's output; z feeds
// the decoder stack

// ---- backward --------------------------------------------------------------------------------------------------------
// The seam, backward: the gradient of the codes gz (extra gradient and klw * dKL/dz already added, in that order) through
// the binarisation (straight-through: the same with hard codes), plus the direct gradient g_hs of the encoder's output
__device__ __forceinline__ float lstm_seam_bwd(float gz, float yv, float g_hs, float bin_tau) {
    return g_hs + gz * yv * (1.0f - yv) / bin_tau;
}

// Column kcol of gate block blk of the transposed weights into registers: wic[jj] = W_ih[blk * L + jj][kcol], whc likewise
// from W_hh (zero for jj >= L)
template <int LMAX>
__device__ __forceinline__ void lstm_load_gate_cols(float (&wic)[LMAX], float (&whc)[LMAX], const float* wl, int L, int blk,
                                                    int kcol) {
    const float* pi = wl + blk * L * L + kcol;
    const float* ph = pi + 4 * L * L;
#pragma unroll
    for (int jj = 0; jj < LMAX; ++jj) {
        const int o = (jj < L ? jj : L - 1) * L;
        const float a = pi[o], b = ph[o];
        wic[jj] = jj < L ? a : 0.f;
        whc[jj] = jj < L ? b : 0.f;
    }
}

// Gate gradients of one cell from its saved gates, c_t, c_{t-1}, dh_t and the dc carried back from step t + 1
struct LstmGateGrad { float d_i, d_f, d_g, d_o, dc_next; };
__device__ __forceinline__ LstmGateGrad lstm_gate_grad(float ig, float fg, float gg, float og, float c, float cprev, float dh,
                                                       float dc_next) {
    const float tc = fast_tanh(c);
    const float dc = dc_next + dh * og * (1.f - tc * tc);
    LstmGateGrad r;
    r.d_o = dh * tc * og * (1.f - og);
    r.d_i = dc * gg * ig * (1.f - ig);
    r.d_f = dc * cprev * fg * (1.f - fg);
    r.d_g = dc * ig * (1.f - gg * gg);
    r.dc_next = dc * fg;
    return r;
}
// ... and to one row of 4L gate values (the LDS row the transposed product reads, or the cell's row of dG)
__device__ __forceinline__ void lstm_store_gates(float* p, int L, int j, float vi, float vf, float vg, float vo) {
    p[j] = vi; p[L + j] = vf; p[2 * L + j] = vg; p[3 * L + j] = vo;
}

}  // namespace rbvae
