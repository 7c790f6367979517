// Hidden Markov model of the soft latents in time order: the mixture's diagonal Gaussian emissions (csrc/diag_gauss.h), a K x K
// transition matrix, the scaled forward and backward recursions, the smoothed posterior, the expected transition counts and
// the most likely state sequence (hmm.py drives Baum-Welch with rbvae_gmm_mstep and rbvae_gmm_decide and finishes BIC / AIC
// on the host).  DESIGN.md section 7 has the formulation; include/rbvae_hip.h every order.
//   hmm_emit_k      gmm_estep_k's shape: a lane per row, the means and precision roots through LDS in chunks; lb into logb, the
//                   row maximum, and e = exp(lb - max) read back from the lane's own column
//   hmm_carry_k     the recurrence, launch (i): a wave per (block of rows, unit start vector) carries the vector through the
//                   block, normalised after every row, with a running log scale.  A lane per state holds its column (forward)
//                   or row (backward) of A in registers; the vector is broadcast lane by lane
//   hmm_chain_k     launch (ii): one wave walks the blocks in order and turns a block's K carried vectors into the next block's
//                   incoming vector
//   hmm_rows_k      launch (iii): a wave per block reruns the plain recursion from its incoming vector and writes its rows
//   hmm_gamma_k     a thread per row: gamma, and Z_t, the sum of the transition terms of (t, t + 1)
//   hmm_xi_k        stage one of the expected transition counts: a thread per cell (i, j) walks a block's rows ascending
//   hmm_finish_k    stage two: the partials in block order, Xi, A' and pi'
//   hmm_viterbi_k   one wave, a lane per state, sequential in t; byte backpointers, the backtrace through LDS chunks
// state int32 [4] is the mixture's {done, n_iter, why, 0}: every kernel returns at once when done is set.  No floating-point
// atomics (status takes integer atomics, which commute); two runs agree bit for bit.  Contraction is off.
// Several sequences stacked in time order (the rbvae_hmm_seq_ entries) run the same kernels with SEQ set: a block, or for the
// walk and Viterbi a wave, takes its sequence's rows [lo, hi) from the device plan (hm_block, hm_seq_rows) where the
// single-sequence form has [0, N); every index read from the plan is clamped before use.
#include "common.h"
#include "diag_gauss.h"

#include <limits.h>
#include <math.h>

#include <vector>

#pragma clang fp contract(off)

namespace rbvae {

constexpr int HM_MAX_K = 64, HM_MAX_N = 1 << 20;
constexpr int HM_BLOCK_ROWS = 64;       // the default block of the recurrence: a constant, never derived from the device
constexpr int HM_THREADS = 256;
constexpr int HG_ROWS = 64;             // rows per workgroup of hmm_gamma_k
constexpr int HV_ROWS = 256;            // rows of backpointers per LDS chunk of the backtrace
constexpr int HST_DONE = 0;

__global__ __launch_bounds__(HM_THREADS) void hmm_emit_k(const float* __restrict__ X, int N, int L,
                                                         const double* __restrict__ means,
                                                         const double* __restrict__ prec, int K, double* logb,
                                                         double* __restrict__ rowmax, double* __restrict__ e,
                                                         const int* __restrict__ state) {
    __shared__ __attribute__((aligned(16))) double ps[DG_CHUNK];
    __shared__ double lc[HM_MAX_K];
    if (state && state[HST_DONE]) return;
    const int tid = threadIdx.x;
    const int i = blockIdx.x * HM_THREADS + tid;
    const bool live = i < N;
    const int Lp = (L + 7) & ~7;
    const int KC = DG_CHUNK / (2 * Lp);
    float xi[DG_MAX_L];
#pragma unroll
    for (int l = 0; l < DG_MAX_L; ++l) xi[l] = (live && l < L) ? X[(long)i * L + l] : 0.f;
    if (tid < K) {                                          // c_k = sum_l log s_kl - L / 2 log 2 pi, l ascending from zero
        double t = 0.0;
        for (int l = 0; l < L; ++l) t += log(prec[(long)tid * L + l]);
        lc[tid] = t - 0.5 * L * DG_LOG_2PI;
    }
    double m = -INFINITY;
    for (int k0 = 0; k0 < K; k0 += KC) {
        const int n = min(KC, K - k0);
        __syncthreads();                                    // the previous chunk's reads are done; lc is written
        for (int c = tid; c < n * 2 * Lp; c += HM_THREADS) {
            const int r = c / (2 * Lp), cc = c - r * 2 * Lp, l = cc < Lp ? cc : cc - Lp;
            const double* src = cc < Lp ? means : prec;
            ps[c] = l < L ? src[(long)(k0 + r) * L + l] : 0.0;
        }
        __syncthreads();
        for (int r = 0; r < n; ++r) {
            const double lb = lc[k0 + r] - 0.5 * diag_gauss_q(xi, ps + r * 2 * Lp, L, Lp);
            if (live) logb[(long)(k0 + r) * N + i] = lb;
            if (lb > m) m = lb;
        }
    }
    if (!live) return;
    rowmax[i] = m;
    for (int k = 0; k < K; ++k) e[(long)i * K + k] = exp(logb[(long)k * N + i] - m);
}

// ---- the recurrence -------------------------------------------------------------------------------------------------------

__device__ __forceinline__ double hm_wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// sum_i x_i a[i] with i ascending from zero, x_i lane i's x; beyond K the terms are exact zeros
__device__ __forceinline__ double hm_dot(double x, const double (&a)[HM_MAX_K], int K) {
    double s = 0.0;
#pragma unroll
    for (int i0 = 0; i0 < HM_MAX_K; i0 += 8) {
        if (i0 < K) {
#pragma unroll
            for (int i = i0; i < i0 + 8; ++i) s += __shfl(x, i, 64) * a[i];
        }
    }
    return s;
}

// the lane's column (forward) or row (backward) of A; zeros beyond K
template <bool FWD>
__device__ __forceinline__ void hm_load_a(const double* __restrict__ A, int K, int lane, double (&a)[HM_MAX_K]) {
#pragma unroll
    for (int i = 0; i < HM_MAX_K; ++i)
        a[i] = (i < K && lane < K) ? (FWD ? A[(long)i * K + lane] : A[(long)lane * K + i]) : 0.0;
}

// one row: forward y_j = (sum_i v_i A_ij) e_j; backward y_i = sum_j A_ij (e_j v_j); z = sum y
template <bool FWD>
__device__ __forceinline__ double hm_step(double v, double ev, const double (&a)[HM_MAX_K], int K, double& z) {
    const double x = FWD ? v : ev * v;
    const double s = hm_dot(x, a, K);
    const double y = FWD ? s * ev : s;
    z = wave_sum_f64(y);
    return y;
}

__device__ __forceinline__ bool hm_bad(double z) { return !(z > 0.0) || z == INFINITY; }

// ---- the plan of several sequences -------------------------------------------------------------------------------------------

// the parts of the device plan (include/rbvae_hip.h has the layout); all zero in the single-sequence kernels
struct HmPlan {
    const int *hdr, *row, *end, *blk, *seq;
    int S, maxb;
};

__device__ __forceinline__ int hm_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }

// the rows [lo, hi) of sequence s, 0 <= lo < hi <= N whatever the plan holds
struct HmRows { int lo, hi; };
__device__ __forceinline__ HmRows hm_seq_rows(const HmPlan& p, int N, int s) {
    s = hm_clamp(s, 0, p.S - 1);
    const int lo = hm_clamp(p.row[s], 0, N - 1);
    return {lo, hm_clamp(p.row[s + 1], lo + 1, N)};
}

// block b of the grid: its sequence's rows, its index bs among that sequence's nb blocks; !ok: not a block of the plan
struct HmBlock { int lo, hi, bs, nb; bool ok; };
template <bool SEQ>
__device__ __forceinline__ HmBlock hm_block(const HmPlan& p, int N, int R, int blocks, int b) {
    if (!SEQ) return {0, N, b, blocks, true};
    if (b >= hm_clamp(p.hdr[3], 0, p.maxb)) return {0, 0, 0, 0, false};
    const int s = hm_clamp(p.seq[b], 0, p.S - 1);
    const HmRows r = hm_seq_rows(p, N, s);
    const int nb = (r.hi - r.lo + R - 1) / R, bs = b - p.blk[s];
    return {r.lo, r.hi, bs, nb, bs >= 0 && bs < nb};
}

// launch (i).  U f64 [blocks][K][K]: the carried vector of unit start vector `start` of block b; S f64 [blocks][K] its log scale.
// Forward: the last block needs no transfer and block 0 carries the true recursion from pi in slot 0.  Backward: mirrored.
// Several sequences: the grid runs over the blocks of all of them, and a sequence's own first (backward: last) block carries.
template <bool FWD, bool SEQ>
__global__ __launch_bounds__(64) void hmm_carry_k(const double* __restrict__ e, int N, int K, const double* __restrict__ pi,
                                                  const double* __restrict__ A, int R, int blocks, HmPlan plan,
                                                  double* __restrict__ U, double* __restrict__ S,
                                                  const int* __restrict__ state) {
    if (state && state[HST_DONE]) return;
    const int b = blockIdx.x, start = blockIdx.y, lane = threadIdx.x;
    const HmBlock q = hm_block<SEQ>(plan, N, R, blocks, b);
    if (!q.ok) return;
    const bool own = FWD ? q.bs == 0 : q.bs == q.nb - 1;     // the block that holds the recursion's first row
    if ((FWD ? q.bs == q.nb - 1 : q.bs == 0) || (own && start != 0)) return;
    const int r0 = q.lo + q.bs * R, r1 = min(q.hi, r0 + R);
    const bool in = lane < K;
    double a[HM_MAX_K];
    hm_load_a<FWD>(A, K, lane, a);
    double v, s = 0.0, z;
    if (FWD) {
        int t = r0;
        if (own) {
            const double y = in ? pi[lane] * e[(long)q.lo * K + lane] : 0.0;
            z = wave_sum_f64(y);
            v = z > 0.0 ? y / z : 0.0;
            t = q.lo + 1;
        } else {
            v = lane == start ? 1.0 : 0.0;
        }
        double en = (in && t < r1) ? e[(long)t * K + lane] : 0.0;
        for (; t < r1; ++t) {
            const double ev = en;
            if (t + 1 < r1) en = in ? e[(long)(t + 1) * K + lane] : 0.0;
            const double y = hm_step<true>(v, ev, a, K, z);
            v = z > 0.0 ? y / z : 0.0;                      // a start vector may die: zeros and a scale of -inf
            s += log(z);
        }
    } else {
        int t = r1 - 1;                                     // the row being written; it reads e of row t + 1
        if (own) {
            v = in ? 1.0 / (double)K : 0.0;
            t = q.hi - 2;
        } else {
            v = lane == start ? 1.0 : 0.0;
        }
        double en = (in && t >= r0) ? e[(long)(t + 1) * K + lane] : 0.0;
        for (; t >= r0; --t) {
            const double ev = en;
            if (t - 1 >= r0) en = in ? e[(long)t * K + lane] : 0.0;
            const double y = hm_step<false>(v, ev, a, K, z);
            v = z > 0.0 ? y / z : 0.0;
            s += log(z);
        }
    }
    if (in) U[((long)b * K + start) * K + lane] = v;
    if (lane == 0) S[(long)b * K + start] = own ? 0.0 : s;
}

// launch (ii).  VIN f64 [blocks][K]: the vector block b starts from (forward: alpha of the row before it; backward: beta of
// the row after it).  out_j = sum_i w_i U[b][i][j], w_i = v_i exp(s_i - max_i s_i) (0 where s_i = -inf), i ascending.
// (Loading the next block's vectors into a second register set ahead of the combine was tried: 256 VGPRs and 114 AGPRs, and
// the two passes together no faster -- the walk is bound by its dependent cross-lane steps as much as by the loads.)
// Several sequences: a wave per sequence walks that sequence's blocks, [base, base + blocks) of the grid.
template <bool FWD, bool SEQ>
__global__ __launch_bounds__(64) void hmm_chain_k(int N, int K, int R, int blocks, HmPlan plan, const double* __restrict__ U,
                                                  const double* __restrict__ S, double* __restrict__ VIN,
                                                  const int* __restrict__ state) {
    if (state && state[HST_DONE]) return;
    const int lane = threadIdx.x;
    const bool in = lane < K;
    int base = 0;
    if (SEQ) {
        const HmRows r = hm_seq_rows(plan, N, blockIdx.x);
        blocks = (r.hi - r.lo + R - 1) / R;
        // one block: nothing enters it.  Two blocks have nothing to combine, but the second still takes the first's own
        // recursion below (VIN of the second = slot 0 of the first): the return is for fewer than two, not fewer than three
        if (blocks < 2) return;
        base = hm_clamp(plan.blk[hm_clamp(blockIdx.x, 0, plan.S - 1)], 0, plan.maxb - blocks);
    }
    const int first = base + (FWD ? 0 : blocks - 1), step = FWD ? 1 : -1;
    double v = in ? U[((long)first * K) * K + lane] : 0.0;
    if (in) VIN[(long)(first + step) * K + lane] = v;
    double u[HM_MAX_K];
    for (int n = 1; n < blocks - 1; ++n) {
        const int b = first + n * step;
#pragma unroll
        for (int i = 0; i < HM_MAX_K; ++i) u[i] = (i < K && in) ? U[((long)b * K + i) * K + lane] : 0.0;
        const double s = in ? S[(long)b * K + lane] : -INFINITY;
        const double mx = hm_wave_max(s);
        const double w = s == -INFINITY ? 0.0 : v * exp(s - mx);
        const double y = hm_dot(w, u, K);
        const double z = wave_sum_f64(y);
        v = z > 0.0 ? y / z : 0.0;
        if (in) VIN[(long)(b + step) * K + lane] = v;
    }
}

// launch (iii): the plain recursion of block b from VIN[b]; nothing is done about a row whose normaliser is 0 or not finite
// but to count it
template <bool FWD, bool SEQ>
__global__ __launch_bounds__(64) void hmm_rows_k(const double* __restrict__ e, const double* __restrict__ rowmax, int N, int K,
                                                 const double* __restrict__ pi, const double* __restrict__ A, int R,
                                                 int blocks, HmPlan plan, const double* __restrict__ VIN,
                                                 double* __restrict__ out, double* __restrict__ ll, int* __restrict__ status,
                                                 const int* __restrict__ state) {
    if (state && state[HST_DONE]) return;
    const int b = blockIdx.x, lane = threadIdx.x;
    const HmBlock q = hm_block<SEQ>(plan, N, R, blocks, b);
    if (!q.ok) return;
    const int r0 = q.lo + q.bs * R, r1 = min(q.hi, r0 + R);
    const bool in = lane < K;
    double a[HM_MAX_K];
    hm_load_a<FWD>(A, K, lane, a);
    double v, z;
    int bad = 0, first = INT_MAX;
    if (FWD) {
        int t = r0;
        if (q.bs == 0) {
            const double y = in ? pi[lane] * e[(long)q.lo * K + lane] : 0.0;
            z = wave_sum_f64(y);
            v = y / z;
            if (in) out[(long)q.lo * K + lane] = v;
            if (lane == 0) ll[q.lo] = log(z) + rowmax[q.lo];
            if (hm_bad(z)) { ++bad; first = q.lo; }
            t = q.lo + 1;
        } else {
            v = in ? VIN[(long)b * K + lane] : 0.0;
        }
        double en = (in && t < r1) ? e[(long)t * K + lane] : 0.0;
        for (; t < r1; ++t) {
            const double ev = en;
            if (t + 1 < r1) en = in ? e[(long)(t + 1) * K + lane] : 0.0;
            const double y = hm_step<true>(v, ev, a, K, z);
            v = y / z;
            if (in) out[(long)t * K + lane] = v;
            if (lane == 0) ll[t] = log(z) + rowmax[t];
            if (hm_bad(z)) { if (!bad) first = t; ++bad; }
        }
    } else {
        int t = r1 - 1;
        if (q.bs == q.nb - 1) {
            v = in ? 1.0 / (double)K : 0.0;
            if (in) out[(long)(q.hi - 1) * K + lane] = v;
            t = q.hi - 2;
        } else {
            v = in ? VIN[(long)b * K + lane] : 0.0;
        }
        double en = (in && t >= r0) ? e[(long)(t + 1) * K + lane] : 0.0;
        for (; t >= r0; --t) {
            const double ev = en;
            if (t - 1 >= r0) en = in ? e[(long)t * K + lane] : 0.0;
            const double y = hm_step<false>(v, ev, a, K, z);
            v = y / z;
            if (in) out[(long)t * K + lane] = v;
            if (hm_bad(z)) { first = t; ++bad; }            // t descends: the last one found is the first row
        }
    }
    if (lane == 0 && bad) {
        atomicAdd(&status[0], bad);
        atomicMin(&status[1], first);
    }
}

// ---- the posterior --------------------------------------------------------------------------------------------------------

// gamma_kt = alpha_tk beta_tk / g_t, g_t = sum_k alpha_tk beta_tk (k ascending); Z_t = sum_i sum_j (alpha_ti A_ij) w_j with
// w_j = e_(t+1)j beta_(t+1)j, i ascending and inside it j ascending, one running sum from zero
// Several sequences: the pair (t, t + 1) exists where t does not end a sequence (end int32 [N], the plan's).
template <bool SEQ>
__global__ __launch_bounds__(HG_ROWS) void hmm_gamma_k(const double* __restrict__ alpha, const double* __restrict__ beta,
                                                       const double* __restrict__ e, int N, int K,
                                                       const double* __restrict__ A, const int* __restrict__ end,
                                                       double* __restrict__ gamma,
                                                       double* __restrict__ Z, int* __restrict__ status,
                                                       const int* __restrict__ state) {
    __shared__ double As[HM_MAX_K * HM_MAX_K];
    __shared__ double ws[HG_ROWS * (HM_MAX_K + 1)];
    if (state && state[HST_DONE]) return;
    const int tid = threadIdx.x, t = blockIdx.x * HG_ROWS + tid;
    const int Kp = K | 1;                                   // an odd stride: the lanes' rows fall on different banks
    for (int c = tid; c < K * K; c += HG_ROWS) As[c] = A[c];
    const bool live = t < N, pair = t < N - 1 && !(SEQ && end[t]);
    double* w = ws + tid * Kp;
    int bad = 0;
    if (live) {
        double g = 0.0;
        for (int k = 0; k < K; ++k) g += alpha[(long)t * K + k] * beta[(long)t * K + k];
        for (int k = 0; k < K; ++k) gamma[(long)k * N + t] = (alpha[(long)t * K + k] * beta[(long)t * K + k]) / g;
        if (hm_bad(g)) ++bad;
    }
    if (pair)
        for (int j = 0; j < K; ++j) w[j] = e[(long)(t + 1) * K + j] * beta[(long)(t + 1) * K + j];
    __syncthreads();
    if (pair) {
        double z = 0.0;
        for (int i = 0; i < K; ++i) {
            const double ai = alpha[(long)t * K + i];
            for (int j = 0; j < K; ++j) z += (ai * As[i * K + j]) * w[j];
        }
        Z[t] = z;
        if (hm_bad(z)) ++bad;
    }
    if (bad) {
        atomicAdd(&status[0], bad);
        atomicMin(&status[1], t);
    }
}

// part f64 [blocks][K][K]; grid (blocks, ceil(K K / 256)): cell (i, j) adds xi_t(i, j) over the block's rows t ascending
template <bool SEQ>
__global__ __launch_bounds__(HM_THREADS) void hmm_xi_k(const double* __restrict__ alpha, const double* __restrict__ beta,
                                                       const double* __restrict__ e, int N, int K,
                                                       const double* __restrict__ A, const double* __restrict__ Z,
                                                       const int* __restrict__ end, int rows, double* __restrict__ part,
                                                       const int* __restrict__ state) {
    if (state && state[HST_DONE]) return;
    const int c = blockIdx.y * HM_THREADS + threadIdx.x;
    if (c >= K * K) return;
    const int i = c / K, j = c - i * K;
    const int r0 = blockIdx.x * rows, r1 = min(N - 1, r0 + rows);
    const double aij = A[c];
    double acc = 0.0;
    for (int t = r0; t < r1; ++t) {
        const double w = e[(long)(t + 1) * K + j] * beta[(long)(t + 1) * K + j];
        const double x = ((alpha[(long)t * K + i] * aij) * w) / Z[t];
        // no term across a boundary: a select, not a branch, which keeps the rows' loads in flight together (Z of such a row
        // is whatever the workspace held; the quotient is dropped unseen)
        acc = (SEQ && end[t]) ? acc : acc + x;
    }
    part[(long)blockIdx.x * K * K + c] = acc;
}

// Several sequences: pi'_k = (sum_s gamma_k,first(s)) / S, thread k's one running sum with s ascending.  The first rows of 256
// sequences at a time pass through LDS (one coalesced load of the plan), so that a thread's loads of gamma do not wait for
// the plan and only the additions are a dependent chain; DESIGN.md section 7 has what it costs.
template <bool SEQ>
__global__ __launch_bounds__(HM_THREADS) void hmm_finish_k(const double* __restrict__ part, int blocks, int N, int K,
                                                           HmPlan plan, const double* __restrict__ gamma,
                                                           double* __restrict__ xi,
                                                           double* __restrict__ A_new, double* __restrict__ pi_new,
                                                           const int* __restrict__ state) {
    __shared__ double xs[HM_MAX_K * HM_MAX_K];
    __shared__ double rs[HM_MAX_K];
    __shared__ int los[SEQ ? HM_THREADS : 1];
    if (state && state[HST_DONE]) return;
    const int tid = threadIdx.x;
    double p = 0.0;
    if (SEQ) {
        for (int s0 = 0; s0 < plan.S; s0 += HM_THREADS) {
            __syncthreads();                                // the previous chunk has been read
            if (s0 + tid < plan.S) los[tid] = hm_seq_rows(plan, N, s0 + tid).lo;
            __syncthreads();
            const int n = min(HM_THREADS, plan.S - s0);
            if (tid < K) {
#pragma unroll 8
                for (int i = 0; i < n; ++i) p += gamma[(long)tid * N + los[i]];
            }
        }
    }
    for (int c = tid; c < K * K; c += HM_THREADS) {
        double a = 0.0;
        for (int b = 0; b < blocks; ++b) a += part[(long)b * K * K + c];
        xs[c] = a;
        xi[c] = a;
    }
    __syncthreads();
    if (tid < K) {
        double a = 0.0;
        for (int j = 0; j < K; ++j) a += xs[tid * K + j];
        rs[tid] = a;
        if (SEQ) {
            pi_new[tid] = p / (double)plan.S;
        } else {
            pi_new[tid] = gamma[(long)tid * N];
        }
    }
    __syncthreads();
    for (int c = tid; c < K * K; c += HM_THREADS) A_new[c] = (xs[c] + DG_NK_EPS / (double)K) / (rs[c / K] + DG_NK_EPS);
}

// ---- Viterbi --------------------------------------------------------------------------------------------------------------

// Several sequences: a wave per sequence, over its rows [lo, hi) of the stacked arrays; score[s].
template <bool SEQ>
__global__ __launch_bounds__(64) void hmm_viterbi_k(const double* __restrict__ logb, int N, int K, HmPlan plan,
                                                    const double* __restrict__ log_pi, const double* __restrict__ log_A,
                                                    unsigned char* __restrict__ back, int* __restrict__ path,
                                                    double* __restrict__ score, const int* __restrict__ state) {
    __shared__ unsigned char bs[HV_ROWS * HM_MAX_K];
    if (state && state[HST_DONE]) return;
    const int lane = threadIdx.x;
    const bool in = lane < K;
    int lo = 0, hi = N;
    if (SEQ) {
        const HmRows r = hm_seq_rows(plan, N, blockIdx.x);
        lo = r.lo;
        hi = r.hi;
    }
    double la[HM_MAX_K];
#pragma unroll
    for (int i = 0; i < HM_MAX_K; ++i) la[i] = (i < K && in) ? log_A[(long)i * K + lane] : -INFINITY;
    double d = in ? log_pi[lane] + logb[(long)lane * N + lo] : -INFINITY;
    if (in) back[(long)lo * K + lane] = 0;
    double bn = (in && hi - lo > 1) ? logb[(long)lane * N + lo + 1] : 0.0;
    for (int t = lo + 1; t < hi; ++t) {
        const double bt = bn;
        if (t + 1 < hi) bn = in ? logb[(long)lane * N + t + 1] : 0.0;
        double best = -INFINITY;
        int arg = 0;
#pragma unroll
        for (int i0 = 0; i0 < HM_MAX_K; i0 += 8) {
            if (i0 < K) {
#pragma unroll
                for (int i = i0; i < i0 + 8; ++i) {
                    const double c = __shfl(d, i, 64) + la[i];
                    if (c > best) {                         // i ascends: a tie stays with the lower state
                        best = c;
                        arg = i;
                    }
                }
            }
        }
        d = in ? best + bt : -INFINITY;
        if (in) back[(long)t * K + lane] = (unsigned char)arg;
    }
    double best = -INFINITY;
    int s = 0;
    for (int i = 0; i < K; ++i) {
        const double c = __shfl(d, i, 64);
        if (c > best) {
            best = c;
            s = i;
        }
    }
    if (lane == 0) score[SEQ ? hm_clamp(blockIdx.x, 0, plan.S - 1) : 0] = best;
    __threadfence_block();
    // the backtrace: chunks of HV_ROWS rows of backpointers pass through LDS, lane 0 walks them
    for (int c1 = hi; c1 > lo; c1 -= HV_ROWS) {
        const int c0 = max(lo, c1 - HV_ROWS);
        __syncthreads();
        for (int x = lane; x < (c1 - c0) * K; x += 64) bs[x] = back[(long)c0 * K + x];
        __syncthreads();
        if (lane == 0) {
            for (int t = c1 - 1; t >= c0; --t) {
                path[t] = s;
                s = bs[(t - c0) * K + s];
            }
        }
        s = __shfl(s, 0, 64);
    }
}

static bool hm_ok(int N, int L, int K) {
    return L >= 1 && L <= DG_MAX_L && K >= 1 && K <= HM_MAX_K && N >= (K > 2 ? K : 2) && N <= HM_MAX_N &&
           (long)N * K <= DG_MAX_NK;
}
static size_t hm_ws_bytes(int N, int K, int R) {
    const size_t blocks = (size_t)cdiv(N, R);
    const size_t rec = blocks * ((size_t)K * K + 2 * (size_t)K);
    const size_t post = (size_t)N + (size_t)row_blocks(N) * K * K;
    return sizeof(double) * (rec > post ? rec : post);
}

// Several sequences.  The plan, int32: {S, N, block_rows, B}, row [S + 1], end [N], blk [S + 1], seq [maxb]; the parts that
// do not depend on block_rows come first, so the posterior and Viterbi find theirs without it.
static int hm_max_blocks(int N, int S, int R) {
    if (R > N) R = N;
    const long m = (long)cdiv(N, R) + S;
    return (int)(m < N ? m : N);
}
struct HmPlanAt { size_t row, end, blk, seq; };
static HmPlanAt hm_plan_at(int N, int S, int R) {
    (void)R;
    const size_t row = 4, end = row + S + 1, blk = end + N;
    return {row, end, blk, blk + S + 1};
}
static size_t hm_plan_ints(int N, int S, int R) { return hm_plan_at(N, S, R).seq + (size_t)hm_max_blocks(N, S, R); }
static HmPlan hm_plan(const void* dev, int N, int S, int R) {
    const int* p = (const int*)dev;
    const HmPlanAt at = hm_plan_at(N, S, R);
    return {p, p + at.row, p + at.end, p + at.blk, p + at.seq, S, hm_max_blocks(N, S, R)};
}
static size_t hm_post_ws_bytes(int N, int K) { return sizeof(double) * ((size_t)N + (size_t)row_blocks(N) * K * K); }
static size_t hm_seq_ws_bytes(int N, int K, int S, int R) {
    const size_t rec = sizeof(double) * (size_t)hm_max_blocks(N, S, R) * ((size_t)K * K + 2 * (size_t)K);
    const size_t post = hm_post_ws_bytes(N, K);
    return rec > post ? rec : post;
}

}  // namespace rbvae

using namespace rbvae;

#define HM_CHECK_SHAPE(name, L)                                                                                        \
    do {                                                                                                               \
        if (!hm_ok(N, L, K))                                                                                           \
            return fail(RBVAE_E_UNSUPPORTED,                                                                           \
                        name ": (N=%d, L=%d, K=%d) outside 1 <= L <= %d, 1 <= K <= %d, max(K, 2) <= N <= %d, N K <= %ld", N, \
                        L, K, DG_MAX_L, HM_MAX_K, HM_MAX_N, DG_MAX_NK);                                                \
    } while (0)

#define HM_CHECK_WS(name, R)                                                                                           \
    do {                                                                                                               \
        RBVAE_CHECK_ARG(R >= 1, name ": block_rows=%d", R);                                                            \
        RBVAE_CHECK_ARG(ws && ws_bytes >= hm_ws_bytes(N, K, R), name ": workspace of %zu bytes, %zu needed", ws_bytes,  \
                        hm_ws_bytes(N, K, R));                                                                         \
    } while (0)

extern "C" int rbvae_hmm_ok(int N, int L, int K) { return hm_ok(N, L, K) ? 1 : 0; }

extern "C" int rbvae_hmm_block_rows(void) { return HM_BLOCK_ROWS; }

extern "C" size_t rbvae_hmm_ws_bytes(int N, int K, int block_rows) {
    if (!hm_ok(N, 1, K) || block_rows < 1) return 0;
    return hm_ws_bytes(N, K, block_rows);
}

extern "C" int rbvae_hmm_emit(const float* X, int N, int L, const double* means, const double* prec_chol, int K, double* logb,
                              double* rowmax, double* e, const int* state, void* stream) {
    HM_CHECK_SHAPE("hmm_emit", L);
    RBVAE_CHECK_ARG(X && means && prec_chol && logb && rowmax && e, "hmm_emit: null pointer");
    hipLaunchKernelGGL(hmm_emit_k, dim3(cdiv(N, HM_THREADS)), dim3(HM_THREADS), 0, (hipStream_t)stream, X, N, L, means,
                       prec_chol, K, logb, rowmax, e, state);
    RBVAE_CHECK_LAUNCH("hmm_emit");
    return RBVAE_OK;
}

template <bool FWD, bool SEQ>
static int hm_recurrence(const char* name, const double* e, const double* rowmax, int N, int K, const double* pi,
                         const double* A, int R, const HmPlan& plan, double* out, double* ll, int* status, double* ws,
                         const int* state, hipStream_t st) {
    if (R > N) R = N;
    const int blocks = SEQ ? plan.maxb : cdiv(N, R);        // several sequences: the grid's extent, of which the plan uses some
    double* U = ws;
    double* S = U + (size_t)blocks * K * K;
    double* VIN = S + (size_t)blocks * K;
    if (SEQ || blocks > 1) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(hmm_carry_k<FWD, SEQ>), dim3(blocks, K), dim3(64), 0, st, e, N, K, pi, A, R, blocks,
                           plan, U, S, state);
        RBVAE_CHECK_LAUNCH(name);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(hmm_chain_k<FWD, SEQ>), dim3(SEQ ? plan.S : 1), dim3(64), 0, st, N, K, R, blocks,
                           plan, (const double*)U, (const double*)S, VIN, state);
        RBVAE_CHECK_LAUNCH(name);
    }
    hipLaunchKernelGGL(HIP_KERNEL_NAME(hmm_rows_k<FWD, SEQ>), dim3(blocks), dim3(64), 0, st, e, rowmax, N, K, pi, A, R, blocks,
                       plan, (const double*)VIN, out, ll, status, state);
    RBVAE_CHECK_LAUNCH(name);
    return RBVAE_OK;
}

extern "C" int rbvae_hmm_forward(const double* e, const double* rowmax, int N, int K, const double* pi, const double* A,
                                 int block_rows, double* alpha, double* ll, int* status, void* ws, size_t ws_bytes,
                                 const int* state, void* stream) {
    HM_CHECK_SHAPE("hmm_forward", 1);
    RBVAE_CHECK_ARG(e && rowmax && pi && A && alpha && ll && status, "hmm_forward: null pointer");
    HM_CHECK_WS("hmm_forward", block_rows);
    return hm_recurrence<true, false>("hmm_forward", e, rowmax, N, K, pi, A, block_rows, HmPlan{}, alpha, ll, status,
                                      (double*)ws, state, (hipStream_t)stream);
}

extern "C" int rbvae_hmm_backward(const double* e, int N, int K, const double* A, int block_rows, double* beta, int* status,
                                  void* ws, size_t ws_bytes, const int* state, void* stream) {
    HM_CHECK_SHAPE("hmm_backward", 1);
    RBVAE_CHECK_ARG(e && A && beta && status, "hmm_backward: null pointer");
    HM_CHECK_WS("hmm_backward", block_rows);
    return hm_recurrence<false, false>("hmm_backward", e, nullptr, N, K, nullptr, A, block_rows, HmPlan{}, beta, nullptr,
                                       status, (double*)ws, state, (hipStream_t)stream);
}

template <bool SEQ>
static int hm_posterior(const char* name, const double* alpha, const double* beta, const double* e, int N, int K,
                        const double* A, const HmPlan& plan, double* gamma, double* xi, double* A_new, double* pi_new,
                        int* status, double* ws, const int* state, hipStream_t st) {
    const int blocks = row_blocks(N), rows = row_block_rows(N);
    double* Z = ws;
    double* part = Z + N;
    hipLaunchKernelGGL(hmm_gamma_k<SEQ>, dim3(cdiv(N, HG_ROWS)), dim3(HG_ROWS), 0, st, alpha, beta, e, N, K, A, plan.end, gamma,
                       Z, status, state);
    RBVAE_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(hmm_xi_k<SEQ>, dim3(blocks, cdiv((long)K * K, HM_THREADS)), dim3(HM_THREADS), 0, st, alpha, beta, e, N,
                       K, A, (const double*)Z, plan.end, rows, part, state);
    RBVAE_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(hmm_finish_k<SEQ>, dim3(1), dim3(HM_THREADS), 0, st, (const double*)part, blocks, N, K, plan,
                       (const double*)gamma, xi, A_new, pi_new, state);
    RBVAE_CHECK_LAUNCH(name);
    return RBVAE_OK;
}

extern "C" int rbvae_hmm_posterior(const double* alpha, const double* beta, const double* e, int N, int K, const double* A,
                                   double* gamma, double* xi, double* A_new, double* pi_new, int* status, void* ws,
                                   size_t ws_bytes, const int* state, void* stream) {
    HM_CHECK_SHAPE("hmm_posterior", 1);
    RBVAE_CHECK_ARG(alpha && beta && e && A && gamma && xi && A_new && pi_new && status, "hmm_posterior: null pointer");
    HM_CHECK_WS("hmm_posterior", N);
    return hm_posterior<false>("hmm_posterior", alpha, beta, e, N, K, A, HmPlan{}, gamma, xi, A_new, pi_new, status,
                               (double*)ws, state, (hipStream_t)stream);
}

extern "C" int rbvae_hmm_viterbi(const double* logb, int N, int K, const double* log_pi, const double* log_A,
                                 unsigned char* back, int* path, double* score, const int* state, void* stream) {
    HM_CHECK_SHAPE("hmm_viterbi", 1);
    RBVAE_CHECK_ARG(logb && log_pi && log_A && back && path && score, "hmm_viterbi: null pointer");
    hipLaunchKernelGGL(hmm_viterbi_k<false>, dim3(1), dim3(64), 0, (hipStream_t)stream, logb, N, K, HmPlan{}, log_pi, log_A,
                       back, path, score, state);
    RBVAE_CHECK_LAUNCH("hmm_viterbi");
    return RBVAE_OK;
}

// ---- several sequences ----------------------------------------------------------------------------------------------------

#define HM_CHECK_SEQ(name)                                                                                             \
    do {                                                                                                               \
        HM_CHECK_SHAPE(name, 1);                                                                                       \
        if (S < 1 || S > N) return fail(RBVAE_E_UNSUPPORTED, name ": S=%d outside 1 <= S <= N = %d", S, N);            \
    } while (0)

#define HM_CHECK_SEQ_WS(name, R)                                                                                       \
    do {                                                                                                               \
        RBVAE_CHECK_ARG(R >= 1, name ": block_rows=%d", R);                                                            \
        RBVAE_CHECK_ARG(ws && ws_bytes >= hm_seq_ws_bytes(N, K, S, R), name ": workspace of %zu bytes, %zu needed",    \
                        ws_bytes, hm_seq_ws_bytes(N, K, S, R));                                                        \
    } while (0)

extern "C" int rbvae_hmm_seq_ok(int N, int L, int K, int S) { return hm_ok(N, L, K) && S >= 1 && S <= N ? 1 : 0; }

extern "C" size_t rbvae_hmm_seq_plan_bytes(int N, int S, int block_rows) {
    if (N < 1 || N > HM_MAX_N || S < 1 || S > N || block_rows < 1) return 0;
    return hm_plan_ints(N, S, block_rows) * sizeof(int);
}

extern "C" size_t rbvae_hmm_seq_ws_bytes(int N, int K, int S, int block_rows) {
    if (!hm_ok(N, 1, K) || S < 1 || S > N || block_rows < 1) return 0;
    return hm_seq_ws_bytes(N, K, S, block_rows);
}

extern "C" int rbvae_hmm_seq_plan(const int* lengths_host, int S, int N, int block_rows, void* plan_dev, size_t plan_bytes,
                                  void* stream) {
    if (N < 1 || N > HM_MAX_N || S < 1 || S > N)
        return fail(RBVAE_E_UNSUPPORTED, "hmm_seq_plan: (N=%d, S=%d) outside 1 <= S <= N <= %d", N, S, HM_MAX_N);
    RBVAE_CHECK_ARG(lengths_host && plan_dev, "hmm_seq_plan: null pointer");
    RBVAE_CHECK_ARG(block_rows >= 1, "hmm_seq_plan: block_rows=%d", block_rows);
    const int R = block_rows > N ? N : block_rows;
    const size_t ints = hm_plan_ints(N, S, R);
    RBVAE_CHECK_ARG(plan_bytes >= ints * sizeof(int), "hmm_seq_plan: plan of %zu bytes, %zu needed", plan_bytes,
                    ints * sizeof(int));
    long total = 0;
    for (int s = 0; s < S; ++s) {
        RBVAE_CHECK_ARG(lengths_host[s] >= 1, "hmm_seq_plan: lengths[%d]=%d, every sequence needs a row", s, lengths_host[s]);
        total += lengths_host[s];
        RBVAE_CHECK_ARG(total <= N, "hmm_seq_plan: the lengths add to more than N=%d", N);
    }
    RBVAE_CHECK_ARG(total == N, "hmm_seq_plan: the lengths add to %ld, N=%d", total, N);
    std::vector<int> h(ints, 0);
    const HmPlanAt at = hm_plan_at(N, S, R);
    int row = 0, blk = 0;
    for (int s = 0; s < S; ++s) {
        h[at.row + s] = row;
        h[at.blk + s] = blk;
        for (int b = 0; b < cdiv(lengths_host[s], R); ++b) h[at.seq + blk++] = s;
        row += lengths_host[s];
        h[at.end + row - 1] = 1;
    }
    h[at.row + S] = N;
    h[at.blk + S] = blk;
    h[0] = S, h[1] = N, h[2] = R, h[3] = blk;
    // the host copy lives until the transfer has been taken: the stream is waited for (once per fit, not per iteration)
    hipError_t err = hipMemcpyAsync(plan_dev, h.data(), ints * sizeof(int), hipMemcpyHostToDevice, (hipStream_t)stream);
    if (err == hipSuccess) err = hipStreamSynchronize((hipStream_t)stream);
    if (err != hipSuccess) return fail(RBVAE_E_LAUNCH, "hmm_seq_plan: %s", hipGetErrorString(err));
    return RBVAE_OK;
}

extern "C" int rbvae_hmm_seq_forward(const double* e, const double* rowmax, int N, int K, const double* pi, const double* A,
                                     int block_rows, const void* plan, int S, double* alpha, double* ll, int* status, void* ws,
                                     size_t ws_bytes, const int* state, void* stream) {
    HM_CHECK_SEQ("hmm_seq_forward");
    RBVAE_CHECK_ARG(e && rowmax && pi && A && plan && alpha && ll && status, "hmm_seq_forward: null pointer");
    HM_CHECK_SEQ_WS("hmm_seq_forward", block_rows);
    return hm_recurrence<true, true>("hmm_seq_forward", e, rowmax, N, K, pi, A, block_rows, hm_plan(plan, N, S, block_rows),
                                     alpha, ll, status, (double*)ws, state, (hipStream_t)stream);
}

extern "C" int rbvae_hmm_seq_backward(const double* e, int N, int K, const double* A, int block_rows, const void* plan, int S,
                                      double* beta, int* status, void* ws, size_t ws_bytes, const int* state, void* stream) {
    HM_CHECK_SEQ("hmm_seq_backward");
    RBVAE_CHECK_ARG(e && A && plan && beta && status, "hmm_seq_backward: null pointer");
    HM_CHECK_SEQ_WS("hmm_seq_backward", block_rows);
    return hm_recurrence<false, true>("hmm_seq_backward", e, nullptr, N, K, nullptr, A, block_rows,
                                      hm_plan(plan, N, S, block_rows), beta, nullptr, status, (double*)ws, state,
                                      (hipStream_t)stream);
}

extern "C" int rbvae_hmm_seq_posterior(const double* alpha, const double* beta, const double* e, int N, int K, const void* plan,
                                       int S, const double* A, double* gamma, double* xi, double* A_new, double* pi_new,
                                       int* status, void* ws, size_t ws_bytes, const int* state, void* stream) {
    HM_CHECK_SEQ("hmm_seq_posterior");
    RBVAE_CHECK_ARG(alpha && beta && e && plan && A && gamma && xi && A_new && pi_new && status,
                    "hmm_seq_posterior: null pointer");
    RBVAE_CHECK_ARG(ws && ws_bytes >= hm_post_ws_bytes(N, K), "hmm_seq_posterior: workspace of %zu bytes, %zu needed", ws_bytes,
                    hm_post_ws_bytes(N, K));                // its own need: Z and the block partials, whatever block_rows
    return hm_posterior<true>("hmm_seq_posterior", alpha, beta, e, N, K, A, hm_plan(plan, N, S, N), gamma, xi, A_new, pi_new,
                              status, (double*)ws, state, (hipStream_t)stream);
}

extern "C" int rbvae_hmm_seq_viterbi(const double* logb, int N, int K, const void* plan, int S, const double* log_pi,
                                     const double* log_A, unsigned char* back, int* path, double* score, const int* state,
                                     void* stream) {
    HM_CHECK_SEQ("hmm_seq_viterbi");
    RBVAE_CHECK_ARG(logb && plan && log_pi && log_A && back && path && score, "hmm_seq_viterbi: null pointer");
    hipLaunchKernelGGL(hmm_viterbi_k<true>, dim3(S), dim3(64), 0, (hipStream_t)stream, logb, N, K, hm_plan(plan, N, S, N),
                       log_pi, log_A, back, path, score, state);
    RBVAE_CHECK_LAUNCH("hmm_seq_viterbi");
    return RBVAE_OK;
}
