// Lloyd's k-means with k-means++ seeding on the soft latents, and the per-cluster sums behind the Davies-Bouldin and
// Calinski-Harabasz indices.  DESIGN.md section 7 has the formulation; scikit-learn 1.7.2's KMeans(algorithm="lloyd") is
// the behaviour restated (symbols.py keeps its RandomState draws and finishes the scores on the host).
//   kmeans_assign_k     label_dist_sums_k's shape: a workgroup owns 256 rows (one per lane, the row in registers), the
//                       centres pass through LDS as f64 in chunks of KM_CHUNK values and every lane reads them at the same
//                       address (broadcast); the lane keeps the smallest (d2, k).  With `own` it keeps d2 to the row's own
//                       centre instead.  The rows whose label moved are counted with one integer atomic per workgroup.
//   kmeans_partial_k    stage one of the update: a workgroup owns a block of rows (diag_gauss.h's row_blocks) and a chunk of
//                       clusters; thread c owns column c of an LDS slab [clusters][L + 3] (the L coordinates, d2, sqrt(d2)
//                       and a count of ones) and walks the block's rows in ascending order, so no two threads touch one
//                       cell and every cell has one order
//   kmeans_finish_k     stage two: a workgroup per cluster, thread c adds column c of the block partials in block order,
//                       divides by the count and leaves an empty cluster's centre as it was
//   kmeans_decide_k     one wave: adds shift2 in k order and applies scikit-learn's two stopping rules to state
//   kmeans_pp_k, kmeans_pp_pot_k   the k-means++ trials: min(closest, d2 to the candidate row) and its fixed-order sum
// state int32 [4] = {done, n_iter, why, changed}: every kernel of an iteration returns at once when done is set, so the
// host may enqueue iterations ahead of the decision.  No floating-point atomics; two runs agree bit for bit.  Contraction
// is off.
#include "common.h"
#include "diag_gauss.h"
#include "pairdist.h"

#include <math.h>

#pragma clang fp contract(off)

namespace rbvae {

constexpr int KM_THREADS = 256;
constexpr int KM_MAX_L = 128, KM_MAX_K = 256, KM_MAX_N = 1 << 20, KM_MAX_T = 8;
constexpr int KM_CHUNK = 4096;          // f64 values of centres per LDS chunk (32 KB): KM_CHUNK / round_up(L, 8) centres
constexpr int KU_SLAB = 8192;           // f64 values of the update's LDS slab (64 KB): KU_SLAB / (L + 3) clusters
constexpr int KU_THREADS = 192;         // >= KM_MAX_L + 3 columns
constexpr int ST_DONE = 0, ST_ITER = 1, ST_WHY = 2, ST_CHANGED = 3;

__global__ __launch_bounds__(KM_THREADS) void kmeans_assign_k(const float* __restrict__ X, int N, int L,
                                                              const double* __restrict__ C, int K,
                                                              const int* __restrict__ prev, const int* __restrict__ own,
                                                              int* __restrict__ label, double* __restrict__ d2out,
                                                              int* __restrict__ state) {
    __shared__ __attribute__((aligned(16))) double cs[KM_CHUNK];
    __shared__ int moved[KM_THREADS / 64];
    if (state && state[ST_DONE]) return;                    // the same in every workgroup: only kmeans_decide_k writes it
    const int tid = threadIdx.x;
    const int i = blockIdx.x * KM_THREADS + tid;
    const bool live = i < N;
    const int Lp = (L + 7) & ~7;                            // the row stride in LDS; the padding holds zeros
    const int KC = KM_CHUNK / Lp;
    float xi[KM_MAX_L];                                     // zeros beyond L: a padded coordinate adds an exact +0
#pragma unroll
    for (int l = 0; l < KM_MAX_L; ++l) xi[l] = (live && l < L) ? X[(long)i * L + l] : 0.f;
    const int mine = (own && live) ? own[i] : -1;
    double best = INFINITY;
    int bk = -1;
    for (int k0 = 0; k0 < K; k0 += KC) {
        const int n = min(KC, K - k0);
        __syncthreads();                                    // the previous chunk's reads are done
        for (int e = tid; e < n * Lp; e += KM_THREADS) {
            const int r = e / Lp, l = e - r * Lp;
            cs[e] = l < L ? C[(long)(k0 + r) * L + l] : 0.0;
        }
        __syncthreads();
        for (int r = 0; r < n; ++r) {
            const double* p = cs + r * Lp;                  // the same address in every lane: broadcast reads
            double d = 0.0;
#pragma unroll
            for (int l0 = 0; l0 < KM_MAX_L; l0 += 8) {
                if (l0 < L) {
#pragma unroll
                    for (int l = l0; l < l0 + 8; ++l) d2_step(d, (double)xi[l], p[l]);
                }
            }
            const bool take = own ? (k0 + r == mine) : (d < best);     // k ascends: a tie stays with the lower centre
            if (take) {
                best = d;
                bk = k0 + r;
            }
        }
    }
    if (live) {
        label[i] = bk;
        d2out[i] = best;
    }
    if (state) {
        const bool ch = live && bk != (prev ? prev[i] : -1);
        const int c = __popcll(__ballot(ch));
        if ((tid & 63) == 0) moved[tid >> 6] = c;
        __syncthreads();
        if (tid == 0) {
            const int t = moved[0] + moved[1] + moved[2] + moved[3];
            if (t) atomicAdd(state + ST_CHANGED, t);
        }
    }
}

// ws f64 [blocks][K][L + 3]; grid (blocks, cluster chunks)
__global__ __launch_bounds__(KU_THREADS) void kmeans_partial_k(const float* __restrict__ X, int N, int L,
                                                               const int* __restrict__ label,
                                                               const double* __restrict__ d2, int K, int rows,
                                                               double* __restrict__ ws, const int* __restrict__ state) {
    __shared__ __attribute__((aligned(16))) double slab[KU_SLAB];
    if (state && state[ST_DONE]) return;
    const int c = threadIdx.x, LS = L + 3;
    const int KC = KU_SLAB / LS;
    const int k0 = blockIdx.y * KC, n = min(KC, K - k0);
    const int r0 = blockIdx.x * rows, r1 = min(N, r0 + rows);
    for (int e = c; e < n * LS; e += KU_THREADS) slab[e] = 0.0;
    __syncthreads();
    if (c < LS) {
        for (int r = r0; r < r1; ++r) {
            const int k = label[r] - k0;                    // the same in every thread
            if (k < 0 || k >= n) continue;                  // another chunk's cluster, or no cluster at all
            double v;
            if (c < L) v = (double)X[(long)r * L + c];
            else if (c == L) v = d2 ? d2[r] : 0.0;
            else if (c == L + 1) v = d2 ? sqrt(d2[r]) : 0.0;
            else v = 1.0;                                   // the count: exact in f64
            slab[k * LS + c] += v;
        }
    }
    __syncthreads();
    double* out = ws + ((long)blockIdx.x * K + k0) * LS;
    for (int e = c; e < n * LS; e += KU_THREADS) out[e] = slab[e];
}

__global__ __launch_bounds__(KU_THREADS) void kmeans_finish_k(const double* __restrict__ ws, int blocks, int L, int K,
                                                              double* __restrict__ C, int* __restrict__ count,
                                                              double* __restrict__ shift2, double* __restrict__ within,
                                                              double* __restrict__ spread, const int* __restrict__ state) {
    __shared__ double df2[KM_MAX_L];
    __shared__ double cnt;
    if (state && state[ST_DONE]) return;
    const int c = threadIdx.x, k = blockIdx.x, LS = L + 3;
    double s = 0.0;
    if (c < LS)
        for (int b = 0; b < blocks; ++b) s += ws[((long)b * K + k) * LS + c];
    if (c == L + 2) cnt = s;
    __syncthreads();
    const double n = cnt;
    if (c < L) {
        double q = 0.0;
        if (n > 0.0) {
            const double nw = s / n, df = nw - C[(long)k * L + c];
            q = df * df;
            C[(long)k * L + c] = nw;
        }                                                   // an empty cluster keeps its centre
        df2[c] = q;
    } else if (c == L) {
        within[k] = s;
    } else if (c == L + 1) {
        spread[k] = s;
    } else if (c == L + 2) {
        count[k] = (int)s;
    }
    __syncthreads();
    if (c == 0) {
        double t = 0.0;
        for (int l = 0; l < L; ++l) t += df2[l];
        shift2[k] = t;
    }
}

__global__ void kmeans_decide_k(const double* __restrict__ shift2, int K, double tol_abs, int max_iter,
                                int* __restrict__ state) {
    if (threadIdx.x != 0 || state[ST_DONE]) return;
    double t = 0.0;
    for (int k = 0; k < K; ++k) t += shift2[k];
    const int it = state[ST_ITER] + 1, changed = state[ST_CHANGED];
    state[ST_ITER] = it;
    state[ST_CHANGED] = 0;
    int why = 0;
    if (changed == 0) why = 1;                              // strict convergence
    else if (t <= tol_abs) why = 2;
    else if (it >= max_iter) why = 3;
    if (why) {
        state[ST_WHY] = why;
        state[ST_DONE] = 1;
    }
}

// out f64 [T][N], part f64 [T][gridDim.x]
__global__ __launch_bounds__(KM_THREADS) void kmeans_pp_k(const float* __restrict__ X, int N, int L,
                                                          const int* __restrict__ cand, int T,
                                                          const double* __restrict__ closest, double* __restrict__ out,
                                                          double* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) double cx[KM_MAX_T * KM_MAX_L];
    __shared__ int okc[KM_MAX_T];
    __shared__ double red[KM_THREADS];
    const int tid = threadIdx.x;
    const int i = blockIdx.x * KM_THREADS + tid;
    const bool live = i < N;
    const int Lp = (L + 7) & ~7;
    for (int e = tid; e < T * Lp; e += KM_THREADS) {
        const int t = e / Lp, l = e - t * Lp;
        const int j = cand[t];
        const bool ok = j >= 0 && j < N;
        cx[e] = (ok && l < L) ? (double)X[(long)j * L + l] : 0.0;
        if (l == 0) okc[t] = ok ? 1 : 0;
    }
    float xi[KM_MAX_L];
#pragma unroll
    for (int l = 0; l < KM_MAX_L; ++l) xi[l] = (live && l < L) ? X[(long)i * L + l] : 0.f;
    const double cl = live ? closest[i] : 0.0;
    __syncthreads();
    for (int t = 0; t < T; ++t) {
        const double* p = cx + t * Lp;
        double d = 0.0;
#pragma unroll
        for (int l0 = 0; l0 < KM_MAX_L; l0 += 8) {
            if (l0 < L) {
#pragma unroll
                for (int l = l0; l < l0 + 8; ++l) d2_step(d, (double)xi[l], p[l]);
            }
        }
        const double m = (okc[t] && d < cl) ? d : cl;       // a candidate that is no row changes nothing
        if (live) out[(long)t * N + i] = m;
        const double s = block_tree_sum<KM_THREADS>(live ? m : 0.0, red);
        if (tid == 0) part[(long)t * gridDim.x + blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(KM_THREADS) void kmeans_pp_pot_k(const double* __restrict__ part, int blocks,
                                                              double* __restrict__ pot) {
    __shared__ double red[KM_THREADS];
    const int t = blockIdx.x;
    double s = 0.0;
    for (int b = threadIdx.x; b < blocks; b += KM_THREADS) s += part[(long)t * blocks + b];
    s = block_tree_sum<KM_THREADS>(s, red);
    if (threadIdx.x == 0) pot[t] = s;
}

static bool km_ok(int N, int L, int K) {
    return L >= 1 && L <= KM_MAX_L && K >= 1 && K <= KM_MAX_K && N >= K && N <= KM_MAX_N;
}

}  // namespace rbvae

using namespace rbvae;

#define KM_CHECK_SHAPE(name)                                                                                          \
    do {                                                                                                              \
        if (!km_ok(N, L, K))                                                                                          \
            return fail(RBVAE_E_UNSUPPORTED, name ": (N=%d, L=%d, K=%d) outside 1 <= L <= %d, 1 <= K <= %d, K <= N <= %d", \
                        N, L, K, KM_MAX_L, KM_MAX_K, KM_MAX_N);                                                       \
    } while (0)

extern "C" int rbvae_kmeans_ok(int N, int L, int K) { return km_ok(N, L, K) ? 1 : 0; }

extern "C" int rbvae_kmeans_chunk_centres(int L) { return L >= 1 && L <= KM_MAX_L ? KM_CHUNK / ((L + 7) & ~7) : 0; }

extern "C" size_t rbvae_kmeans_ws_bytes(int N, int L, int K) {
    if (!km_ok(N, L, K)) return 0;
    const size_t upd = (size_t)row_blocks(N) * K * (L + 3), pp = (size_t)KM_MAX_T * cdiv(N, KM_THREADS);
    return sizeof(double) * (upd > pp ? upd : pp);
}

extern "C" int rbvae_kmeans_assign(const float* X, int N, int L, const double* centres, int K, const int* label_prev,
                                   const int* own, int* label, double* d2, int* state, void* stream) {
    KM_CHECK_SHAPE("kmeans_assign");
    RBVAE_CHECK_ARG(X && centres && label && d2, "kmeans_assign: null pointer");
    hipLaunchKernelGGL(kmeans_assign_k, dim3(cdiv(N, KM_THREADS)), dim3(KM_THREADS), 0, (hipStream_t)stream, X, N, L, centres,
                       K, label_prev, own, label, d2, state);
    RBVAE_CHECK_LAUNCH("kmeans_assign");
    return RBVAE_OK;
}

extern "C" int rbvae_kmeans_update(const float* X, int N, int L, const int* label, const double* d2, int K, double* centres,
                                   int* count, double* shift2, double* within, double* spread, double* ws, const int* state,
                                   void* stream) {
    KM_CHECK_SHAPE("kmeans_update");
    RBVAE_CHECK_ARG(X && label && centres && count && shift2 && within && spread && ws, "kmeans_update: null pointer");
    const int blocks = row_blocks(N), chunks = cdiv(K, KU_SLAB / (L + 3));
    hipLaunchKernelGGL(kmeans_partial_k, dim3(blocks, chunks), dim3(KU_THREADS), 0, (hipStream_t)stream, X, N, L, label, d2, K,
                       row_block_rows(N), ws, state);
    RBVAE_CHECK_LAUNCH("kmeans_update (partials)");
    hipLaunchKernelGGL(kmeans_finish_k, dim3(K), dim3(KU_THREADS), 0, (hipStream_t)stream, ws, blocks, L, K, centres, count,
                       shift2, within, spread, state);
    RBVAE_CHECK_LAUNCH("kmeans_update (finish)");
    return RBVAE_OK;
}

extern "C" int rbvae_kmeans_decide(const double* shift2, int K, double tol_abs, int max_iter, int* state, void* stream) {
    if (K < 1 || K > KM_MAX_K) return fail(RBVAE_E_UNSUPPORTED, "kmeans_decide: K=%d outside 1..%d", K, KM_MAX_K);
    RBVAE_CHECK_ARG(shift2 && state, "kmeans_decide: null pointer");
    RBVAE_CHECK_ARG(max_iter >= 1 && tol_abs >= 0.0, "kmeans_decide: max_iter=%d, tol=%g", max_iter, tol_abs);
    hipLaunchKernelGGL(kmeans_decide_k, dim3(1), dim3(64), 0, (hipStream_t)stream, shift2, K, tol_abs, max_iter, state);
    RBVAE_CHECK_LAUNCH("kmeans_decide");
    return RBVAE_OK;
}

extern "C" int rbvae_kmeans_pp_trials(const float* X, int N, int L, const int* cand, int T, const double* closest,
                                      double* out, double* pot, double* ws, void* stream) {
    const int K = 1;
    KM_CHECK_SHAPE("kmeans_pp_trials");
    if (T < 1 || T > KM_MAX_T) return fail(RBVAE_E_UNSUPPORTED, "kmeans_pp_trials: T=%d outside 1..%d", T, KM_MAX_T);
    RBVAE_CHECK_ARG(X && cand && closest && out && pot && ws, "kmeans_pp_trials: null pointer");
    const int blocks = cdiv(N, KM_THREADS);
    hipLaunchKernelGGL(kmeans_pp_k, dim3(blocks), dim3(KM_THREADS), 0, (hipStream_t)stream, X, N, L, cand, T, closest, out, ws);
    RBVAE_CHECK_LAUNCH("kmeans_pp_trials");
    hipLaunchKernelGGL(kmeans_pp_pot_k, dim3(T), dim3(KM_THREADS), 0, (hipStream_t)stream, ws, blocks, pot);
    RBVAE_CHECK_LAUNCH("kmeans_pp_trials (potentials)");
    return RBVAE_OK;
}
