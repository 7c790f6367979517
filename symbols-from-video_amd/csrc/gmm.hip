// Diagonal-covariance Gaussian mixture of the soft latents by EM, as scikit-learn 1.7.2's
// GaussianMixture(covariance_type="diag", n_init=1) runs it (mixture.py drives the iterations and finishes BIC / AIC on the
// host).  DESIGN.md section 7 has the formulation; include/rbvae_hip.h every order.
//   gmm_estep_k     kmeans_assign_k's shape: a workgroup owns 256 rows (one per lane, the row in registers), the components'
//                   means and precision roots pass through LDS as f64 in chunks and every lane reads them at the same
//                   address (broadcast).  The first sweep over the components stores lp into resp's column of the row and
//                   keeps the largest (lp, lowest k); the lane then reads its own values back for the sum of exp(lp - m)
//                   and once more for resp = exp(lp - lognorm).  Without resp the sweep runs twice instead.
//   gmm_partial_k   stage one of the M-step, run twice: a workgroup owns a block of rows (diag_gauss.h's row_blocks) and 256
//                   cells (k, c) of [K][L + 1]; a thread walks the block's rows in ascending order and adds r_ki x_ic
//                   (c = L: r_ki alone).  The centred run first rebuilds nk_k and mu_kc from the first run's partials, in
//                   block order, and adds r_ki (x_ic - mu_kc)^2.
//   gmm_finish_k    stage two: a workgroup per component adds the partials in block order and writes weights, means,
//                   covars, prec_chol and logc
//   gmm_decide_k    one workgroup: the mean of lognorm in sp_dots_k's two-stage order (spectral.hip), the history and the stopping rules
// state int32 [4] = {done, n_iter, why, 0}: every kernel returns at once when done is set, so the host may enqueue
// iterations ahead of the decision.  No floating-point atomics; two runs agree bit for bit.  Contraction is off.
#include "common.h"
#include "diag_gauss.h"

#include <math.h>

#pragma clang fp contract(off)

namespace rbvae {

constexpr int GM_THREADS = 256;
constexpr int GM_MAX_K = 256, GM_MAX_N = 1 << 20;
constexpr int GD_ROWS = 1024;           // rows per block of the lower bound's sum: sp_dots_k's blocks (spectral.hip)
constexpr int GST_DONE = 0, GST_ITER = 1, GST_WHY = 2;

// lp = logc - q / 2
__device__ __forceinline__ double gm_lp(const float* xi, const double* p, int L, int Lp, double logc) {
    return logc - 0.5 * diag_gauss_q(xi, p, L, Lp);
}

__global__ __launch_bounds__(GM_THREADS) void gmm_estep_k(const float* __restrict__ X, int N, int L,
                                                          const double* __restrict__ means,
                                                          const double* __restrict__ prec,
                                                          const double* __restrict__ logc, int K, double* resp,
                                                          double* __restrict__ lognorm, int* __restrict__ label,
                                                          const int* __restrict__ state) {
    __shared__ __attribute__((aligned(16))) double ps[DG_CHUNK];
    __shared__ double lc[DG_CHUNK / 16];
    if (state && state[GST_DONE]) return;                   // the same in every workgroup: only gmm_decide_k writes it
    const int tid = threadIdx.x;
    const int i = blockIdx.x * GM_THREADS + tid;
    const bool live = i < N;
    const int Lp = (L + 7) & ~7;                            // the row stride in LDS; the padding holds zeros
    const int KC = DG_CHUNK / (2 * Lp);
    float xi[DG_MAX_L];                                     // zeros beyond L
#pragma unroll
    for (int l = 0; l < DG_MAX_L; ++l) xi[l] = (live && l < L) ? X[(long)i * L + l] : 0.f;
    double m = -INFINITY, s = 0.0;
    int bk = 0;
    // with resp: one sweep that stores lp; without: a second sweep computes the same lp again for the sum
    const int sweeps = resp ? 1 : 2;
    for (int sweep = 0; sweep < sweeps; ++sweep) {
        for (int k0 = 0; k0 < K; k0 += KC) {
            const int n = min(KC, K - k0);
            __syncthreads();                                // the previous chunk's reads are done
            for (int e = tid; e < n * 2 * Lp; e += GM_THREADS) {
                const int r = e / (2 * Lp), c = e - r * 2 * Lp, l = c < Lp ? c : c - Lp;
                const double* src = c < Lp ? means : prec;
                ps[e] = l < L ? src[(long)(k0 + r) * L + l] : 0.0;
            }
            if (tid < n) lc[tid] = logc[k0 + tid];
            __syncthreads();
            for (int r = 0; r < n; ++r) {
                const double lp = gm_lp(xi, ps + r * 2 * Lp, L, Lp, lc[r]);
                if (sweep == 0) {
                    if (resp && live) resp[(long)(k0 + r) * N + i] = lp;
                    if (lp > m) {                           // k ascends: a tie stays with the lower component
                        m = lp;
                        bk = k0 + r;
                    }
                } else {
                    s += exp(lp - m);
                }
            }
        }
    }
    if (!live) return;
    if (resp)
        for (int k = 0; k < K; ++k) s += exp(resp[(long)k * N + i] - m);
    const double ln = m + log(s);
    lognorm[i] = ln;
    if (label) label[i] = bk;
    if (resp)
        for (int k = 0; k < K; ++k) resp[(long)k * N + i] = exp(resp[(long)k * N + i] - ln);
}

// nk_k and the sum behind mu_kc from the uncentred partials ws1 f64 [blocks][K][L + 1], in block order from zero
__device__ __forceinline__ void gm_block_sums(const double* __restrict__ ws1, int blocks, int K, int LS, int k, int c,
                                              double& nk, double& sx) {
    double a = 0.0, b = 0.0;
    for (int blk = 0; blk < blocks; ++blk) {
        const double* p = ws1 + ((long)blk * K + k) * LS;
        a += p[LS - 1];
        b += p[c];
    }
    nk = a + DG_NK_EPS;
    sx = b;
}

// out f64 [blocks][K][L + 1]; grid (blocks, ceil(K (L + 1) / 256)).  CENTRED: ws1 holds the uncentred run's partials.
template <bool CENTRED>
__global__ __launch_bounds__(GM_THREADS) void gmm_partial_k(const float* __restrict__ X, int N, int L,
                                                            const double* __restrict__ resp, int K, int rows,
                                                            const double* __restrict__ ws1, int blocks,
                                                            double* __restrict__ out, const int* __restrict__ state) {
    if (state && state[GST_DONE]) return;
    const int LS = L + 1;
    const int e = blockIdx.y * GM_THREADS + threadIdx.x;
    if (e >= K * LS) return;
    const int k = e / LS, c = e - k * LS;
    const int r0 = blockIdx.x * rows, r1 = min(N, r0 + rows);
    const double* rk = resp + (long)k * N;
    double acc = 0.0;
    if (CENTRED) {
        if (c < L) {
            double nk, sx;
            gm_block_sums(ws1, blocks, K, LS, k, c, nk, sx);
            const double mu = sx / nk;
            for (int r = r0; r < r1; ++r) {
                const double d = (double)X[(long)r * L + c] - mu;
                const double d2 = d * d;
                acc += rk[r] * d2;
            }
        }
    } else if (c < L) {
        for (int r = r0; r < r1; ++r) acc += rk[r] * (double)X[(long)r * L + c];
    } else {
        for (int r = r0; r < r1; ++r) acc += rk[r];
    }
    out[((long)blockIdx.x * K + k) * LS + c] = acc;
}

__global__ __launch_bounds__(GM_THREADS) void gmm_finish_k(const double* __restrict__ ws1, const double* __restrict__ ws2,
                                                           int blocks, int L, int K, double reg_covar,
                                                           double* __restrict__ weights, double* __restrict__ means,
                                                           double* __restrict__ covars, double* __restrict__ prec,
                                                           double* __restrict__ logc, const int* __restrict__ state) {
    __shared__ double nks[GM_MAX_K];
    __shared__ double logs[DG_MAX_L];
    __shared__ double total;
    if (state && state[GST_DONE]) return;
    const int c = threadIdx.x, k = blockIdx.x, LS = L + 1;
    if (c < K) {                                            // every component's nk: the weights' denominator
        double a = 0.0;
        for (int blk = 0; blk < blocks; ++blk) a += ws1[((long)blk * K + c) * LS + L];
        nks[c] = a + DG_NK_EPS;
    }
    __syncthreads();
    if (c == 0) {
        double t = 0.0;
        for (int j = 0; j < K; ++j) t += nks[j];
        total = t;
    }
    if (c < L) {
        double nk, sx, v = 0.0;
        gm_block_sums(ws1, blocks, K, LS, k, c, nk, sx);
        for (int blk = 0; blk < blocks; ++blk) v += ws2[((long)blk * K + k) * LS + c];
        const double var = v / nk + reg_covar;
        const double s = 1.0 / sqrt(var);
        means[(long)k * L + c] = sx / nk;
        covars[(long)k * L + c] = var;
        prec[(long)k * L + c] = s;
        logs[c] = log(s);
    }
    __syncthreads();
    if (c == 0) {
        const double w = nks[k] / total;
        double t = 0.0;
        for (int l = 0; l < L; ++l) t += logs[l];
        weights[k] = w;
        logc[k] = (log(w) + t) - 0.5 * L * DG_LOG_2PI;
    }
}

// lb f64 [1]: the previous lower bound on entry (-inf before the first iteration), this one on return
__global__ __launch_bounds__(GM_THREADS) void gmm_decide_k(const double* __restrict__ lognorm, int N, double tol,
                                                           int max_iter, double* __restrict__ lb,
                                                           double* __restrict__ history, int* __restrict__ state) {
    __shared__ double wsum[(GM_MAX_N / GD_ROWS) * 4];
    if (state[GST_DONE]) return;                            // read by every thread before thread 0 writes it below
    const int tid = threadIdx.x, blocks = (N + GD_ROWS - 1) / GD_ROWS;
    for (int b = 0; b < blocks; ++b) {
        double v = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = b * GD_ROWS + tid + GM_THREADS * j;
            v += i < N ? lognorm[i] : 0.0;
        }
        v = wave_sum_f64(v);
        if ((tid & 63) == 0) wsum[b * 4 + (tid >> 6)] = v;
    }
    __syncthreads();
    for (int b = tid; b < blocks; b += GM_THREADS) {
        double t = 0.0;
        for (int w = 0; w < 4; ++w) t += wsum[b * 4 + w];
        wsum[b * 4] = t;
    }
    __syncthreads();
    if (tid != 0) return;
    double t = 0.0;
    for (int b = 0; b < blocks; ++b) t += wsum[b * 4];
    const double now = t / (double)N, prev = lb[0];
    const int it = state[GST_ITER] + 1;
    lb[0] = now;
    if (it <= max_iter) history[it - 1] = now;
    state[GST_ITER] = it;
    int why = 0;
    if (fabs(now - prev) < tol) why = 1;
    else if (it >= max_iter) why = 2;
    if (why) {
        state[GST_WHY] = why;
        state[GST_DONE] = 1;
    }
}

static bool gm_ok(int N, int L, int K) {
    return L >= 1 && L <= DG_MAX_L && K >= 1 && K <= GM_MAX_K && N >= K && N <= GM_MAX_N && (long)N * K <= DG_MAX_NK;
}

}  // namespace rbvae

using namespace rbvae;

#define GM_CHECK_SHAPE(name)                                                                                          \
    do {                                                                                                              \
        if (!gm_ok(N, L, K))                                                                                          \
            return fail(RBVAE_E_UNSUPPORTED,                                                                          \
                        name ": (N=%d, L=%d, K=%d) outside 1 <= L <= %d, 1 <= K <= %d, K <= N <= %d, N K <= %ld", N, L, K, \
                        DG_MAX_L, GM_MAX_K, GM_MAX_N, DG_MAX_NK);                                                     \
    } while (0)

extern "C" int rbvae_gmm_ok(int N, int L, int K) { return gm_ok(N, L, K) ? 1 : 0; }

extern "C" int rbvae_gmm_chunk_components(int L) {
    return L >= 1 && L <= DG_MAX_L ? DG_CHUNK / (2 * ((L + 7) & ~7)) : 0;
}

extern "C" size_t rbvae_gmm_ws_bytes(int N, int L, int K) {
    if (!gm_ok(N, L, K)) return 0;
    return sizeof(double) * 2 * (size_t)row_blocks(N) * K * (L + 1);
}

extern "C" int rbvae_gmm_estep(const float* X, int N, int L, const double* means, const double* prec_chol,
                               const double* logc, int K, double* resp, double* lognorm, int* label, const int* state,
                               void* stream) {
    GM_CHECK_SHAPE("gmm_estep");
    RBVAE_CHECK_ARG(X && means && prec_chol && logc && lognorm, "gmm_estep: null pointer");
    hipLaunchKernelGGL(gmm_estep_k, dim3(cdiv(N, GM_THREADS)), dim3(GM_THREADS), 0, (hipStream_t)stream, X, N, L, means,
                       prec_chol, logc, K, resp, lognorm, label, state);
    RBVAE_CHECK_LAUNCH("gmm_estep");
    return RBVAE_OK;
}

extern "C" int rbvae_gmm_mstep(const float* X, int N, int L, const double* resp, int K, double reg_covar, double* weights,
                               double* means, double* covars, double* prec_chol, double* logc, double* ws,
                               const int* state, void* stream) {
    GM_CHECK_SHAPE("gmm_mstep");
    RBVAE_CHECK_ARG(X && resp && weights && means && covars && prec_chol && logc && ws, "gmm_mstep: null pointer");
    RBVAE_CHECK_ARG(reg_covar >= 0.0, "gmm_mstep: reg_covar=%g", reg_covar);
    const int blocks = row_blocks(N), rows = row_block_rows(N);
    const dim3 grid(blocks, cdiv((long)K * (L + 1), GM_THREADS));
    double* ws2 = ws + (size_t)blocks * K * (L + 1);
    hipLaunchKernelGGL(gmm_partial_k<false>, grid, dim3(GM_THREADS), 0, (hipStream_t)stream, X, N, L, resp, K, rows,
                       (const double*)nullptr, blocks, ws, state);
    RBVAE_CHECK_LAUNCH("gmm_mstep (sums)");
    hipLaunchKernelGGL(gmm_partial_k<true>, grid, dim3(GM_THREADS), 0, (hipStream_t)stream, X, N, L, resp, K, rows,
                       (const double*)ws, blocks, ws2, state);
    RBVAE_CHECK_LAUNCH("gmm_mstep (centred sums)");
    hipLaunchKernelGGL(gmm_finish_k, dim3(K), dim3(GM_THREADS), 0, (hipStream_t)stream, (const double*)ws,
                       (const double*)ws2, blocks, L, K, reg_covar, weights, means, covars, prec_chol, logc, state);
    RBVAE_CHECK_LAUNCH("gmm_mstep (finish)");
    return RBVAE_OK;
}

extern "C" int rbvae_gmm_decide(const double* lognorm, int N, double tol, int max_iter, double* lb, double* history,
                                int* state, void* stream) {
    if (N < 1 || N > GM_MAX_N) return fail(RBVAE_E_UNSUPPORTED, "gmm_decide: N=%d outside 1..%d", N, GM_MAX_N);
    RBVAE_CHECK_ARG(lognorm && lb && history && state, "gmm_decide: null pointer");
    RBVAE_CHECK_ARG(max_iter >= 1 && tol >= 0.0, "gmm_decide: max_iter=%d, tol=%g", max_iter, tol);
    hipLaunchKernelGGL(gmm_decide_k, dim3(1), dim3(GM_THREADS), 0, (hipStream_t)stream, lognorm, N, tol, max_iter, lb,
                       history, state);
    RBVAE_CHECK_LAUNCH("gmm_decide");
    return RBVAE_OK;
}
