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
#include "common.h"
#include "diag_gauss.h"

#include <limits.h>
#include <math.h>

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

// launch (i).  U f64 [blocks][K][K]: the carried vector of unit start vector `start` of block b; S f64 [blocks][K] its log scale.
// Forward: the last block needs no transfer and block 0 carries the true recursion from pi in slot 0.  Backward: mirrored.
template <bool FWD>
__global__ __launch_bounds__(64) void hmm_carry_k(const double* __restrict__ e, int N, int K, const double* __restrict__ pi,
                                                  const double* __restrict__ A, int R, int blocks, double* __restrict__ U,
                                                  double* __restrict__ S, const int* __restrict__ state) {
    if (state && state[HST_DONE]) return;
    const int b = blockIdx.x, start = blockIdx.y, lane = threadIdx.x;
    const bool own = FWD ? b == 0 : b == blocks - 1;         // the block that holds the recursion's first row
    if ((FWD ? b == blocks - 1 : b == 0) || (own && start != 0)) return;
    const int r0 = b * R, r1 = min(N, r0 + R);
    const bool in = lane < K;
    double a[HM_MAX_K];
    hm_load_a<FWD>(A, K, lane, a);
    double v, s = 0.0, z;
    if (FWD) {
        int t = r0;
        if (own) {
            const double y = in ? pi[lane] * e[lane] : 0.0;
            z = wave_sum_f64(y);
            v = z > 0.0 ? y / z : 0.0;
            t = 1;
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
            t = N - 2;
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
template <bool FWD>
__global__ __launch_bounds__(64) void hmm_chain_k(int K, int blocks, const double* __restrict__ U,
                                                  const double* __restrict__ S, double* __restrict__ VIN,
                                                  const int* __restrict__ state) {
    if (state && state[HST_DONE]) return;
    const int lane = threadIdx.x;
    const bool in = lane < K;
    const int first = FWD ? 0 : blocks - 1, step = FWD ? 1 : -1;
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
template <bool FWD>
__global__ __launch_bounds__(64) void hmm_rows_k(const double* __restrict__ e, const double* __restrict__ rowmax, int N, int K,
                                                 const double* __restrict__ pi, const double* __restrict__ A, int R,
                                                 int blocks, const double* __restrict__ VIN, double* __restrict__ out,
                                                 double* __restrict__ ll, int* __restrict__ status,
                                                 const int* __restrict__ state) {
    if (state && state[HST_DONE]) return;
    const int b = blockIdx.x, lane = threadIdx.x;
    const int r0 = b * R, r1 = min(N, r0 + R);
    const bool in = lane < K;
    double a[HM_MAX_K];
    hm_load_a<FWD>(A, K, lane, a);
    double v, z;
    int bad = 0, first = INT_MAX;
    if (FWD) {
        int t = r0;
        if (b == 0) {
            const double y = in ? pi[lane] * e[lane] : 0.0;
            z = wave_sum_f64(y);
            v = y / z;
            if (in) out[lane] = v;
            if (lane == 0) ll[0] = log(z) + rowmax[0];
            if (hm_bad(z)) { ++bad; first = 0; }
            t = 1;
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
        if (b == blocks - 1) {
            v = in ? 1.0 / (double)K : 0.0;
            if (in) out[(long)(N - 1) * K + lane] = v;
            t = N - 2;
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
__global__ __launch_bounds__(HG_ROWS) void hmm_gamma_k(const double* __restrict__ alpha, const double* __restrict__ beta,
                                                       const double* __restrict__ e, int N, int K,
                                                       const double* __restrict__ A, double* __restrict__ gamma,
                                                       double* __restrict__ Z, int* __restrict__ status,
                                                       const int* __restrict__ state) {
    __shared__ double As[HM_MAX_K * HM_MAX_K];
    __shared__ double ws[HG_ROWS * (HM_MAX_K + 1)];
    if (state && state[HST_DONE]) return;
    const int tid = threadIdx.x, t = blockIdx.x * HG_ROWS + tid;
    const int Kp = K | 1;                                   // an odd stride: the lanes' rows fall on different banks
    for (int c = tid; c < K * K; c += HG_ROWS) As[c] = A[c];
    const bool live = t < N, pair = t < N - 1;
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
__global__ __launch_bounds__(HM_THREADS) void hmm_xi_k(const double* __restrict__ alpha, const double* __restrict__ beta,
                                                       const double* __restrict__ e, int N, int K,
                                                       const double* __restrict__ A, const double* __restrict__ Z, int rows,
                                                       double* __restrict__ part, const int* __restrict__ state) {
    if (state && state[HST_DONE]) return;
    const int c = blockIdx.y * HM_THREADS + threadIdx.x;
    if (c >= K * K) return;
    const int i = c / K, j = c - i * K;
    const int r0 = blockIdx.x * rows, r1 = min(N - 1, r0 + rows);
    const double aij = A[c];
    double acc = 0.0;
    for (int t = r0; t < r1; ++t) {
        const double w = e[(long)(t + 1) * K + j] * beta[(long)(t + 1) * K + j];
        acc += ((alpha[(long)t * K + i] * aij) * w) / Z[t];
    }
    part[(long)blockIdx.x * K * K + c] = acc;
}

__global__ __launch_bounds__(HM_THREADS) void hmm_finish_k(const double* __restrict__ part, int blocks, int N, int K,
                                                           const double* __restrict__ gamma, double* __restrict__ xi,
                                                           double* __restrict__ A_new, double* __restrict__ pi_new,
                                                           const int* __restrict__ state) {
    __shared__ double xs[HM_MAX_K * HM_MAX_K];
    __shared__ double rs[HM_MAX_K];
    if (state && state[HST_DONE]) return;
    const int tid = threadIdx.x;
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
        pi_new[tid] = gamma[(long)tid * N];
    }
    __syncthreads();
    for (int c = tid; c < K * K; c += HM_THREADS) A_new[c] = (xs[c] + DG_NK_EPS / (double)K) / (rs[c / K] + DG_NK_EPS);
}

// ---- Viterbi --------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(64) void hmm_viterbi_k(const double* __restrict__ logb, int N, int K,
                                                    const double* __restrict__ log_pi, const double* __restrict__ log_A,
                                                    unsigned char* __restrict__ back, int* __restrict__ path,
                                                    double* __restrict__ score, const int* __restrict__ state) {
    __shared__ unsigned char bs[HV_ROWS * HM_MAX_K];
    if (state && state[HST_DONE]) return;
    const int lane = threadIdx.x;
    const bool in = lane < K;
    double la[HM_MAX_K];
#pragma unroll
    for (int i = 0; i < HM_MAX_K; ++i) la[i] = (i < K && in) ? log_A[(long)i * K + lane] : -INFINITY;
    double d = in ? log_pi[lane] + logb[(long)lane * N] : -INFINITY;
    if (in) back[lane] = 0;
    double bn = (in && N > 1) ? logb[(long)lane * N + 1] : 0.0;
    for (int t = 1; t < N; ++t) {
        const double bt = bn;
        if (t + 1 < N) bn = in ? logb[(long)lane * N + t + 1] : 0.0;
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
    if (lane == 0) score[0] = best;
    __threadfence_block();
    // the backtrace: chunks of HV_ROWS rows of backpointers pass through LDS, lane 0 walks them
    for (int c1 = N; c1 > 0; c1 -= HV_ROWS) {
        const int c0 = max(0, c1 - HV_ROWS);
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

template <bool FWD>
static int hm_recurrence(const char* name, const double* e, const double* rowmax, int N, int K, const double* pi,
                         const double* A, int R, double* out, double* ll, int* status, double* ws, const int* state,
                         hipStream_t st) {
    if (R > N) R = N;
    const int blocks = cdiv(N, R);
    double* U = ws;
    double* S = U + (size_t)blocks * K * K;
    double* VIN = S + (size_t)blocks * K;
    if (blocks > 1) {
        hipLaunchKernelGGL(hmm_carry_k<FWD>, dim3(blocks, K), dim3(64), 0, st, e, N, K, pi, A, R, blocks, U, S, state);
        RBVAE_CHECK_LAUNCH(name);
        hipLaunchKernelGGL(hmm_chain_k<FWD>, dim3(1), dim3(64), 0, st, K, blocks, (const double*)U, (const double*)S, VIN,
                           state);
        RBVAE_CHECK_LAUNCH(name);
    }
    hipLaunchKernelGGL(hmm_rows_k<FWD>, dim3(blocks), dim3(64), 0, st, e, rowmax, N, K, pi, A, R, blocks, (const double*)VIN,
                       out, ll, status, state);
    RBVAE_CHECK_LAUNCH(name);
    return RBVAE_OK;
}

extern "C" int rbvae_hmm_forward(const double* e, const double* rowmax, int N, int K, const double* pi, const double* A,
                                 int block_rows, double* alpha, double* ll, int* status, void* ws, size_t ws_bytes,
                                 const int* state, void* stream) {
    HM_CHECK_SHAPE("hmm_forward", 1);
    RBVAE_CHECK_ARG(e && rowmax && pi && A && alpha && ll && status, "hmm_forward: null pointer");
    HM_CHECK_WS("hmm_forward", block_rows);
    return hm_recurrence<true>("hmm_forward", e, rowmax, N, K, pi, A, block_rows, alpha, ll, status, (double*)ws, state,
                               (hipStream_t)stream);
}

extern "C" int rbvae_hmm_backward(const double* e, int N, int K, const double* A, int block_rows, double* beta, int* status,
                                  void* ws, size_t ws_bytes, const int* state, void* stream) {
    HM_CHECK_SHAPE("hmm_backward", 1);
    RBVAE_CHECK_ARG(e && A && beta && status, "hmm_backward: null pointer");
    HM_CHECK_WS("hmm_backward", block_rows);
    return hm_recurrence<false>("hmm_backward", e, nullptr, N, K, nullptr, A, block_rows, beta, nullptr, status, (double*)ws,
                                state, (hipStream_t)stream);
}

extern "C" int rbvae_hmm_posterior(const double* alpha, const double* beta, const double* e, int N, int K, const double* A,
                                   double* gamma, double* xi, double* A_new, double* pi_new, int* status, void* ws,
                                   size_t ws_bytes, const int* state, void* stream) {
    HM_CHECK_SHAPE("hmm_posterior", 1);
    RBVAE_CHECK_ARG(alpha && beta && e && A && gamma && xi && A_new && pi_new && status, "hmm_posterior: null pointer");
    HM_CHECK_WS("hmm_posterior", N);
    const int blocks = row_blocks(N), rows = row_block_rows(N);
    double* Z = (double*)ws;
    double* part = Z + N;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(hmm_gamma_k, dim3(cdiv(N, HG_ROWS)), dim3(HG_ROWS), 0, st, alpha, beta, e, N, K, A, gamma, Z, status,
                       state);
    RBVAE_CHECK_LAUNCH("hmm_posterior (gamma)");
    hipLaunchKernelGGL(hmm_xi_k, dim3(blocks, cdiv((long)K * K, HM_THREADS)), dim3(HM_THREADS), 0, st, alpha, beta, e, N, K, A,
                       (const double*)Z, rows, part, state);
    RBVAE_CHECK_LAUNCH("hmm_posterior (transition sums)");
    hipLaunchKernelGGL(hmm_finish_k, dim3(1), dim3(HM_THREADS), 0, st, (const double*)part, blocks, N, K,
                       (const double*)gamma, xi, A_new, pi_new, state);
    RBVAE_CHECK_LAUNCH("hmm_posterior (finish)");
    return RBVAE_OK;
}

extern "C" int rbvae_hmm_viterbi(const double* logb, int N, int K, const double* log_pi, const double* log_A,
                                 unsigned char* back, int* path, double* score, const int* state, void* stream) {
    HM_CHECK_SHAPE("hmm_viterbi", 1);
    RBVAE_CHECK_ARG(logb && log_pi && log_A && back && path && score, "hmm_viterbi: null pointer");
    hipLaunchKernelGGL(hmm_viterbi_k, dim3(1), dim3(64), 0, (hipStream_t)stream, logb, N, K, log_pi, log_A, back, path, score,
                       state);
    RBVAE_CHECK_LAUNCH("hmm_viterbi");
    return RBVAE_OK;
}
