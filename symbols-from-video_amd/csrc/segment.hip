// State boundaries without the labels: the optimal partition of the N rows of X (in time order) into K contiguous
// segments with the least within-segment sum of squared deviations, by the exact dynamic programme over (segments, end).
// DESIGN.md section 7 has the formulation; tests/_segment_ref.py restates it operation for operation.
//   seg_scan_local_k    a workgroup owns SEG_SCAN = 256 rows: r_i = sum_l x_il^2 per row into LDS, then thread c adds
//                       column c of the block (column L: the r_i) one row at a time and leaves the local running sums in
//                       P and Q
//   seg_scan_offsets_k  one workgroup, thread c: off_{b+1} = off_b + local_last_b along the blocks, written where it
//                       belongs (the last row of a full block is off_b + local_255 = off_{b+1})
//   seg_scan_add_k      every other row: P = off_b + local, off_b read from the row before the block
//   seg_layer_k         a workgroup takes a 64 x 64 tile of (end t, start s) pairs, for a run of `span` start tiles of one
//                       end block.  Both sets of P rows pass through LDS in chunks of SG_LC coordinates as [l][row] images,
//                       a thread holds a 4 x 4 tile of d2 accumulators (two 16-byte LDS reads per side feed 16 d2_steps),
//                       turns them into candidates prev[s] + cost(s, t) after the last chunk and keeps the smallest
//                       (value, s) per end; the 16 threads that share an end are reduced with shuffles.  A start tile with
//                       no finite prev, or wholly beyond t - min_size, is skipped, so only the triangle is visited.
//   seg_combine_k       a thread per end: the smallest (value, s) over the end block's runs
//   seg_trace_k         a thread per k: the walk t <- arg[j][t] from t = N
// The minimum under key_less is exact and order-free, so the result does not depend on `span`.  No floating-point
// atomics; two runs agree bit for bit.  Contraction is off.
#include "common.h"
#include "pairdist.h"

#include <math.h>

#pragma clang fp contract(off)

namespace rbvae {

constexpr int SEG_SCAN = 256;           // rows per block of the prefix scan
constexpr int SEG_MAX_N = 65536, SEG_MAX_L = 128, SEG_MAX_K = 256;
constexpr int SG_THREADS = 256;
constexpr int SG_T = 64;                // tile edge: ends and starts per tile
constexpr int SG_LC = 16;               // coordinates per LDS chunk
constexpr int SG_LD = SG_T + 2;         // f64 stride of an [l][row] image: 528 B keeps 16-byte reads aligned
constexpr int SG_MIN_SPAN = 8;          // start tiles per workgroup at least
constexpr int SG_MAX_RUNS = 32;         // runs per end block at most: bounds the workspace

static int seg_span(int N) {
    const int s = cdiv(cdiv(N, SG_T), SG_MAX_RUNS);
    return s > SG_MIN_SPAN ? s : SG_MIN_SPAN;
}
static int seg_runs(int N) { return cdiv(cdiv(N, SG_T), seg_span(N)); }

__global__ __launch_bounds__(SEG_SCAN) void seg_scan_local_k(const float* __restrict__ X, int N, int L,
                                                             double* __restrict__ P, double* __restrict__ Q) {
    __shared__ double rr[SEG_SCAN];
    const int c = threadIdx.x;
    const int r0 = blockIdx.x * SEG_SCAN, n = min(SEG_SCAN, N - r0);
    if (c < n) {
        const float* x = X + (long)(r0 + c) * L;
        double r = 0.0;
        for (int l = 0; l < L; ++l) {
            const double v = (double)x[l];
            r += v * v;                                     // the product of two f32 values is exact in f64
        }
        rr[c] = r;
    }
    __syncthreads();
    if (blockIdx.x == 0) {
        if (c < L) P[c] = 0.0;
        if (c == L) Q[0] = 0.0;
    }
    if (c < L) {
        double s = (double)X[(long)r0 * L + c];
        P[(long)(r0 + 1) * L + c] = s;
        for (int i = 1; i < n; ++i) {
            s += (double)X[(long)(r0 + i) * L + c];
            P[(long)(r0 + i + 1) * L + c] = s;
        }
    } else if (c == L) {
        double s = rr[0];
        Q[r0 + 1] = s;
        for (int i = 1; i < n; ++i) {
            s += rr[i];
            Q[r0 + i + 1] = s;
        }
    }
}

__global__ __launch_bounds__(SEG_SCAN) void seg_scan_offsets_k(int N, int L, double* __restrict__ P,
                                                               double* __restrict__ Q) {
    const int c = threadIdx.x;
    if (c > L) return;
    double off = 0.0;
    for (int t = SEG_SCAN; t <= N; t += SEG_SCAN) {         // the last rows of the full blocks
        double* p = c < L ? P + (long)t * L + c : Q + t;
        off = off + *p;
        *p = off;
    }
}

__global__ __launch_bounds__(SEG_SCAN) void seg_scan_add_k(int N, int L, double* __restrict__ P, double* __restrict__ Q) {
    const int b = blockIdx.x, r0 = b * SEG_SCAN;
    const int n = min(SEG_SCAN - 1, N - r0);                // row SEG_SCAN - 1 of a full block is final already
    const int LS = L + 1;
    for (int e = threadIdx.x; e < n * LS; e += SEG_SCAN) {
        const int i = e / LS, c = e - i * LS;
        const int t = r0 + i + 1;
        if (c < L) {
            const double off = b ? P[(long)r0 * L + c] : 0.0;
            P[(long)t * L + c] = off + P[(long)t * L + c];
        } else {
            const double off = b ? Q[r0] : 0.0;
            Q[t] = off + Q[t];
        }
    }
}

// a beats b in the order (value, s) ascending; s < 0 marks "no candidate"
__device__ __forceinline__ bool cand_less(double va, int sa, double vb, int sb) {
    return sa >= 0 && (sb < 0 || key_less(va, sa, vb, sb));
}

// grid (runs, end blocks); wv f64 [runs][N + 1], wi int32 [runs][N + 1]
__global__ __launch_bounds__(SG_THREADS) void seg_layer_k(const double* __restrict__ P, const double* __restrict__ Q,
                                                          int N, int L, const double* __restrict__ prev, int m, int span,
                                                          double* __restrict__ wv, int* __restrict__ wi) {
    __shared__ __attribute__((aligned(16))) double pe[SG_LC * SG_LD];
    __shared__ __attribute__((aligned(16))) double ps[SG_LC * SG_LD];
    __shared__ double qe[SG_T], qs[SG_T], pv[SG_T];
    const int eb = blockIdx.y, run = blockIdx.x;
    const int sb0 = run * span;
    if (sb0 > eb) return;                                   // beyond the diagonal: the same in every thread
    const int sb1 = min(eb, sb0 + span - 1);
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int t0 = eb * SG_T + 1;                           // the tile's ends are t0 .. t0 + 63, its starts s0 .. s0 + 63
    const int tmax = min(t0 + SG_T - 1, N);
    if (tid < SG_T) qe[tid] = t0 + tid <= N ? Q[t0 + tid] : 0.0;
    double bv[4];
    int bs[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        bv[i] = INFINITY;
        bs[i] = -1;
    }
    for (int sb = sb0; sb <= sb1; ++sb) {
        const int s0 = sb * SG_T;
        __syncthreads();                                    // the previous tile's reads of qs and pv are done
        int live = 0;
        if (tid < SG_T) {
            const int s = s0 + tid;
            const double v = s < N ? prev[s] : INFINITY;
            const bool fin = isfinite(v);
            pv[tid] = fin ? v : INFINITY;                   // +inf: no candidate from this start
            qs[tid] = s < N ? Q[s] : 0.0;
            live = fin && s <= tmax - m;
        }
        if (!__syncthreads_or(live)) continue;              // the same in every thread
        double acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
        for (int l0 = 0; l0 < L; l0 += SG_LC) {
            const int lc = min(SG_LC, L - l0);
            if (l0) __syncthreads();                        // the previous chunk's reads are done
            for (int e = tid; e < 2 * SG_T * SG_LC; e += SG_THREADS) {
                const int side = e / (SG_T * SG_LC), f = e - side * (SG_T * SG_LC);
                const int r = f / SG_LC, l = f - r * SG_LC;
                const int row = (side ? s0 : t0) + r;
                const double v = (row <= N && l < lc) ? P[(long)row * L + l0 + l] : 0.0;
                (side ? ps : pe)[l * SG_LD + r] = v;
            }
            __syncthreads();
#pragma unroll 2
            for (int l = 0; l < lc; ++l) {
                const double2 a0 = *reinterpret_cast<const double2*>(pe + l * SG_LD + 2 * ty);
                const double2 a1 = *reinterpret_cast<const double2*>(pe + l * SG_LD + 32 + 2 * ty);
                const double2 b0 = *reinterpret_cast<const double2*>(ps + l * SG_LD + 2 * tx);
                const double2 b1 = *reinterpret_cast<const double2*>(ps + l * SG_LD + 32 + 2 * tx);
                const double a[4] = {a0.x, a0.y, a1.x, a1.y}, b[4] = {b0.x, b0.y, b1.x, b1.y};
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) d2_step(acc[i][j], a[i], b[j]);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int ei = (i >> 1) * 32 + 2 * ty + (i & 1);
            const int t = t0 + ei;
            const double qt = qe[ei];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int sj = (j >> 1) * 32 + 2 * tx + (j & 1);
                const int s = s0 + sj;
                const double p = pv[sj];
                const bool ok = t <= N && s <= t - m && p < INFINITY;
                const double len = (double)(ok ? t - s : 1);
                const double cost = (qt - qs[sj]) - acc[i][j] / len;
                const double cand = p + cost;
                if (ok && cand_less(cand, s, bv[i], bs[i])) {
                    bv[i] = cand;
                    bs[i] = s;
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {                  // the 16 lanes tx = 0 .. 15 share the end
            const double ov = __shfl_xor(bv[i], o, 64);
            const int os = __shfl_xor(bs[i], o, 64);
            if (cand_less(ov, os, bv[i], bs[i])) {
                bv[i] = ov;
                bs[i] = os;
            }
        }
        const int t = t0 + (i >> 1) * 32 + 2 * ty + (i & 1);
        if (tx == 0 && t <= N) {
            wv[(long)run * (N + 1) + t] = bv[i];
            wi[(long)run * (N + 1) + t] = bs[i];
        }
    }
}

__global__ __launch_bounds__(SG_THREADS) void seg_combine_k(const double* __restrict__ wv, const int* __restrict__ wi, int N,
                                                            int span, double* __restrict__ out, int* __restrict__ arg) {
    const int t = blockIdx.x * SG_THREADS + threadIdx.x;
    if (t > N) return;
    double v = INFINITY;
    int s = -1;
    if (t > 0) {
        const int runs = ((t - 1) / SG_T) / span + 1;
        for (int r = 0; r < runs; ++r) {
            const double ov = wv[(long)r * (N + 1) + t];
            const int os = wi[(long)r * (N + 1) + t];
            if (cand_less(ov, os, v, s)) {
                v = ov;
                s = os;
            }
        }
    }
    out[t] = s < 0 ? INFINITY : v;
    arg[t] = s;
}

// cuts int32 [K][K]: row k - 1 = the k - 1 interior boundaries of the best k-segmentation ascending, then -1
__global__ __launch_bounds__(SG_THREADS) void seg_trace_k(const int* __restrict__ arg, int N, int K,
                                                          const double* __restrict__ cost, int* __restrict__ cuts) {
    const int k = threadIdx.x + 1;
    if (k > K) return;
    int* row = cuts + (long)(k - 1) * K;
    for (int j = 0; j < K; ++j) row[j] = -1;
    if (!isfinite(cost[(long)(k - 1) * (N + 1) + N])) return;
    int t = N;
    for (int j = k; j >= 2; --j) {
        t = arg[(long)(j - 1) * (N + 1) + t];
        if (t < 0 || t > N) {                               // a table that is no layer output: no segmentation
            for (int q = 0; q < K; ++q) row[q] = -1;
            return;
        }
        row[j - 2] = t;
    }
}

static bool seg_ok(int N, int L, int K, long m) {
    return N >= 2 && N <= SEG_MAX_N && L >= 1 && L <= SEG_MAX_L && K >= 1 && K <= SEG_MAX_K && m >= 1 && (long)K * m <= N;
}

}  // namespace rbvae

using namespace rbvae;

#define SEG_CHECK_SHAPE(name, K, m)                                                                                    \
    do {                                                                                                              \
        if (!seg_ok(N, L, K, m))                                                                                      \
            return fail(RBVAE_E_UNSUPPORTED,                                                                          \
                        name ": (N=%d, L=%d, K=%d, min_size=%d) outside 2 <= N <= %d, 1 <= L <= %d, 1 <= K <= %d, "   \
                             "min_size >= 1, K min_size <= N",                                                       \
                        N, L, K, m, SEG_MAX_N, SEG_MAX_L, SEG_MAX_K);                                                 \
    } while (0)

extern "C" int rbvae_segment_ok(int N, int L, int K, int min_size) { return seg_ok(N, L, K, min_size) ? 1 : 0; }

extern "C" size_t rbvae_segment_ws_bytes(int N, int L) {
    if (!seg_ok(N, L, 1, 1)) return 0;
    const size_t cells = (size_t)seg_runs(N) * (N + 1);
    return (cells * (sizeof(double) + sizeof(int)) + 7) & ~(size_t)7;
}

extern "C" int rbvae_segment_prefix(const float* X, int N, int L, double* P, double* Q, void* stream) {
    SEG_CHECK_SHAPE("segment_prefix", 1, 1);
    RBVAE_CHECK_ARG(X && P && Q, "segment_prefix: null pointer");
    const int blocks = cdiv(N, SEG_SCAN);
    hipLaunchKernelGGL(seg_scan_local_k, dim3(blocks), dim3(SEG_SCAN), 0, (hipStream_t)stream, X, N, L, P, Q);
    RBVAE_CHECK_LAUNCH("segment_prefix (local sums)");
    hipLaunchKernelGGL(seg_scan_offsets_k, dim3(1), dim3(SEG_SCAN), 0, (hipStream_t)stream, N, L, P, Q);
    RBVAE_CHECK_LAUNCH("segment_prefix (offsets)");
    hipLaunchKernelGGL(seg_scan_add_k, dim3(blocks), dim3(SEG_SCAN), 0, (hipStream_t)stream, N, L, P, Q);
    RBVAE_CHECK_LAUNCH("segment_prefix (add)");
    return RBVAE_OK;
}

extern "C" int rbvae_segment_layer(const double* P, const double* Q, int N, int L, const double* prev, int min_size,
                                   double* out, int* arg, void* ws, void* stream) {
    SEG_CHECK_SHAPE("segment_layer", 1, min_size);
    RBVAE_CHECK_ARG(P && Q && prev && out && arg && ws, "segment_layer: null pointer");
    const int span = seg_span(N), runs = seg_runs(N);
    double* wv = (double*)ws;
    int* wi = (int*)(wv + (size_t)runs * (N + 1));
    hipLaunchKernelGGL(seg_layer_k, dim3(runs, cdiv(N, SG_T)), dim3(SG_THREADS), 0, (hipStream_t)stream, P, Q, N, L, prev,
                       min_size, span, wv, wi);
    RBVAE_CHECK_LAUNCH("segment_layer");
    hipLaunchKernelGGL(seg_combine_k, dim3(cdiv(N + 1, SG_THREADS)), dim3(SG_THREADS), 0, (hipStream_t)stream, wv, wi, N, span,
                       out, arg);
    RBVAE_CHECK_LAUNCH("segment_layer (combine)");
    return RBVAE_OK;
}

extern "C" int rbvae_segment_trace(const int* arg, int N, int K, const double* cost, int* cuts, void* stream) {
    const int L = 1;
    SEG_CHECK_SHAPE("segment_trace", K, 1);
    RBVAE_CHECK_ARG(arg && cost && cuts, "segment_trace: null pointer");
    hipLaunchKernelGGL(seg_trace_k, dim3(1), dim3(SG_THREADS), 0, (hipStream_t)stream, arg, N, K, cost, cuts);
    RBVAE_CHECK_LAUNCH("segment_trace");
    return RBVAE_OK;
}
