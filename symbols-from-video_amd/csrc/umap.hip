// UMAP (scripts/evaluation/clustering_eval/embedding_umap.py:63-64) after the exact neighbour graph of project.hip: the
// smooth kNN distances of the fuzzy simplicial set and one synchronous epoch of the layout optimiser (McInnes, Healy,
// Melville 2018, Algorithms 2-5; umap-learn's defaults).  DESIGN.md section 7 has the formulation.
//   umap_dsum_k      the sum of every d = (double)(float)sqrt(d2) in f64, one workgroup of 1024 threads, fixed order
//   umap_smooth_k    rho, the bisection on sigma and the memberships, one wave per row, two neighbours per lane
//   umap_epoch_k     one wave per vertex: the lanes own the CSR row's edges in chunks of 64; a lane evaluates its edge's
//                    attraction (counted twice: the mirror edge moves this end by the same vector) and that edge's negative
//                    samples, a butterfly adds the chunk.  Every vertex moves from the epoch-start map (Y read, Y_out
//                    written) and an edge's schedule state belongs to one lane: no race, no atomic
//   umap_samples_k   the same schedule arithmetic and draws, written out instead of used (what the tests compare)
// Every sum has one fixed order: two runs agree bit for bit.  Contraction is off: sums round where the text says they do.
#include "common.h"

#include <math.h>

#pragma clang fp contract(off)

namespace rbvae {

constexpr int UM_THREADS = 256;
constexpr int UM_MAX_K1 = 127, UM_MAX_N = 16384, UM_MAX_SAMPLES = 32, UM_SMOOTH_ITERS = 64;
constexpr int UM_SUM_THREADS = 1024;

__device__ __forceinline__ double um_dist(double d2) { return (double)(float)sqrt(d2); }

// thread t adds the elements t, t + 1024, ... in ascending order, then a halving tree
__global__ __launch_bounds__(UM_SUM_THREADS) void umap_dsum_k(const double* __restrict__ d2, long n, double* __restrict__ out) {
    __shared__ double red[UM_SUM_THREADS];
    double acc = 0.0;
    for (long e = threadIdx.x; e < n; e += UM_SUM_THREADS) acc += um_dist(d2[e]);
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = UM_SUM_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = red[0];
}

// lane l holds neighbours l and l + 64 of the wave's row (K1 <= 127)
__global__ __launch_bounds__(UM_THREADS) void umap_smooth_k(const double* __restrict__ d2, int N, int K1, double target,
                                                            const double* __restrict__ dsum, float* __restrict__ rho_out,
                                                            float* __restrict__ sigma_out, float* __restrict__ w,
                                                            int* __restrict__ steps) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * (UM_THREADS / 64) + (threadIdx.x >> 6);
    if (i >= N) return;
    const double inf = __builtin_huge_val();
    const bool h0 = lane < K1, h1 = lane + 64 < K1;
    const double d0 = h0 ? um_dist(d2[(long)i * K1 + lane]) : 0.0;
    const double d1 = h1 ? um_dist(d2[(long)i * K1 + lane + 64]) : 0.0;
    double rho = inf;
    if (h0 && d0 > 0.0) rho = d0;
    if (h1 && d1 > 0.0 && d1 < rho) rho = d1;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) rho = fmin(rho, __shfl_xor(rho, o, 64));
    if (rho == inf) rho = 0.0;
    const double e0 = d0 - rho, e1 = d1 - rho;
    double lo = 0.0, hi = inf, mid = 1.0;
    int n = 0;
    for (int it = 0; it < UM_SMOOTH_ITERS; ++it) {
        const double t0 = h0 ? (e0 > 0.0 ? exp(-e0 / mid) : 1.0) : 0.0;
        const double t1 = h1 ? (e1 > 0.0 ? exp(-e1 / mid) : 1.0) : 0.0;
        const double psum = wave_sum_f64(t0 + t1);
        n = it + 1;
        if (fabs(psum - target) < 1e-5) break;
        if (psum > target) {
            hi = mid;
            mid = (lo + hi) / 2.0;
        } else {
            lo = mid;
            mid = hi == inf ? 2.0 * mid : (lo + hi) / 2.0;
        }
    }
    const double k = (double)(K1 + 1);                      // the self distance 0 is one of the k entries
    const double row = wave_sum_f64(d0 + d1);
    const double mean = rho > 0.0 ? row / k : dsum[0] / ((double)N * k);
    const double sigma = fmax(mid, 1e-3 * mean);
    if (h0) w[(long)i * K1 + lane] = (e0 <= 0.0 || sigma == 0.0) ? 1.0f : (float)exp(-e0 / sigma);
    if (h1) w[(long)i * K1 + lane + 64] = (e1 <= 0.0 || sigma == 0.0) ? 1.0f : (float)exp(-e1 / sigma);
    if (lane == 0) { rho_out[i] = (float)rho; sigma_out[i] = (float)sigma; steps[i] = n; }
}

__device__ __forceinline__ int um_neg_count(float nf, float next_neg, float neg_period) {
    const float x = (nf - next_neg) / neg_period;
    return (int)fminf(fmaxf(x, 0.0f), (float)UM_MAX_SAMPLES);      // a NaN counts as 0
}

__device__ __forceinline__ int um_sample(unsigned long long seed, int epoch, int e, int p, int N) {
    const unsigned long long key = ((unsigned long long)epoch << 40) | ((unsigned long long)(unsigned)e << 8) | (unsigned)p;
    return (int)(((unsigned long long)hash_u32(seed, key) * (unsigned long long)N) >> 32);
}

__device__ __forceinline__ float um_clip(float x) { return fminf(fmaxf(x, -4.0f), 4.0f); }

__global__ __launch_bounds__(UM_THREADS) void umap_epoch_k(const float* __restrict__ Y, float* __restrict__ Y_out,
                                                           const int* __restrict__ indptr, const int* __restrict__ indices,
                                                           const float* __restrict__ period, float* __restrict__ next,
                                                           float* __restrict__ next_neg, int N, int epoch, float alpha,
                                                           float a, float b, float gamma, float neg_rate,
                                                           unsigned long long seed) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * (UM_THREADS / 64) + (threadIdx.x >> 6);
    if (i >= N) return;
    const float2 me = ((const float2*)Y)[i];
    const float nf = (float)epoch;
    const float m2ab = (-2.0f * a) * b, g2b = (2.0f * gamma) * b, bm1 = b - 1.0f;
    const int beg = indptr[i], end = indptr[i + 1];
    float tx = 0.f, ty = 0.f;
    for (int e0 = beg; e0 < end; e0 += 64) {                // wave-uniform bounds: the butterfly runs with every lane
        const int e = e0 + lane;
        float sx = 0.f, sy = 0.f;
        if (e < end) {
            const float nx = next[e];
            const int j = indices[e];
            if (nx <= nf && (unsigned)j < (unsigned)N) {
                const float per = period[e];
                const float2 p = ((const float2*)Y)[j];
                float dx = me.x - p.x, dy = me.y - p.y;
                float r2 = fmaf(dy, dy, dx * dx);
                float c = 0.f;
                if (r2 > 0.f) c = (m2ab * powf(r2, bm1)) / (a * powf(r2, b) + 1.0f);
                sx = 2.0f * um_clip(c * dx);
                sy = 2.0f * um_clip(c * dy);
                next[e] = nx + per;
                const float negp = per / neg_rate;
                const float nn = next_neg[e];
                const int q = um_neg_count(nf, nn, negp);
                for (int s = 0; s < q; ++s) {
                    const int m = um_sample(seed, epoch, e, s, N);
                    if (m == i) continue;
                    const float2 o = ((const float2*)Y)[m];
                    dx = me.x - o.x;
                    dy = me.y - o.y;
                    r2 = fmaf(dy, dy, dx * dx);
                    c = 0.f;
                    if (r2 > 0.f) c = g2b / ((0.001f + r2) * (a * powf(r2, b) + 1.0f));
                    sx += um_clip(c * dx);
                    sy += um_clip(c * dy);
                }
                next_neg[e] = nn + (float)q * negp;
            }
        }
        tx += wave_sum(sx);
        ty += wave_sum(sy);
    }
    if (lane == 0) ((float2*)Y_out)[i] = float2{me.x + alpha * tx, me.y + alpha * ty};
}

// count [E] and samples [E][32] of the epoch the state stands before: -1 in a slot that is not drawn or drew the vertex itself
__global__ __launch_bounds__(UM_THREADS) void umap_samples_k(const int* __restrict__ indptr, const float* __restrict__ period,
                                                             const float* __restrict__ next,
                                                             const float* __restrict__ next_neg, int N, int epoch,
                                                             float neg_rate, unsigned long long seed, int* __restrict__ count,
                                                             int* __restrict__ samples) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * (UM_THREADS / 64) + (threadIdx.x >> 6);
    if (i >= N) return;
    const float nf = (float)epoch;
    for (int e = indptr[i] + lane; e < indptr[i + 1]; e += 64) {
        int q = 0;
        if (next[e] <= nf) q = um_neg_count(nf, next_neg[e], period[e] / neg_rate);
        count[e] = q;
        for (int s = 0; s < UM_MAX_SAMPLES; ++s) {
            const int m = s < q ? um_sample(seed, epoch, e, s, N) : -1;
            samples[(long)e * UM_MAX_SAMPLES + s] = m == i ? -1 : m;
        }
    }
}

}  // namespace rbvae

using namespace rbvae;

extern "C" int rbvae_umap_smooth_knn_ok(int N, int K1) { return N >= 1 && K1 >= 1 && K1 <= UM_MAX_K1; }

extern "C" int rbvae_umap_smooth_knn(const double* d2, int N, int K1, double* dsum, float* rho, float* sigma, float* w,
                                     int* steps, void* stream) {
    RBVAE_CHECK_ARG(d2 && dsum && rho && sigma && w && steps, "umap_smooth_knn: null pointer");
    RBVAE_CHECK_ARG(N >= 1, "umap_smooth_knn: N=%d, need at least one row", N);
    RBVAE_CHECK_ARG(K1 >= 1 && K1 <= UM_MAX_K1, "umap_smooth_knn: K1=%d outside 1..%d (n_neighbors - 1, two per lane)", K1,
                    UM_MAX_K1);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(umap_dsum_k, dim3(1), dim3(UM_SUM_THREADS), 0, st, d2, (long)N * K1, dsum);
    RBVAE_CHECK_LAUNCH("umap_smooth_knn (distance sum)");
    hipLaunchKernelGGL(umap_smooth_k, dim3(cdiv(N, UM_THREADS / 64)), dim3(UM_THREADS), 0, st, d2, N, K1,
                       log2((double)(K1 + 1)), (const double*)dsum, rho, sigma, w, steps);
    RBVAE_CHECK_LAUNCH("umap_smooth_knn");
    return RBVAE_OK;
}

extern "C" int rbvae_umap_epoch_ok(int N, int n_epochs, int neg_rate) {
    return N >= 2 && N <= UM_MAX_N && n_epochs >= 1 && n_epochs <= (1 << 20) && neg_rate >= 1 && neg_rate <= 64;
}

static int umap_epoch_args(const char* who, int N, int epoch, int n_epochs, int neg_rate) {
    RBVAE_CHECK_ARG(N >= 2 && N <= UM_MAX_N, "%s: N=%d outside 2..%d", who, N, UM_MAX_N);
    RBVAE_CHECK_ARG(n_epochs >= 1 && n_epochs <= (1 << 20), "%s: n_epochs=%d outside 1..%d", who, n_epochs, 1 << 20);
    RBVAE_CHECK_ARG(epoch >= 0 && epoch < n_epochs, "%s: epoch=%d outside 0..n_epochs - 1 = %d", who, epoch, n_epochs - 1);
    RBVAE_CHECK_ARG(neg_rate >= 1 && neg_rate <= 64, "%s: neg_rate=%d outside 1..64", who, neg_rate);
    return RBVAE_OK;
}

extern "C" int rbvae_umap_epoch(const float* Y, float* Y_out, const int* indptr, const int* indices, const float* period,
                                float* next, float* next_neg, int N, int epoch, int n_epochs, float a, float b, float gamma,
                                int neg_rate, unsigned long long seed, void* stream) {
    RBVAE_CHECK_ARG(Y && Y_out && indptr && indices && period && next && next_neg, "umap_epoch: null pointer");
    RBVAE_CHECK_ARG(Y != Y_out, "umap_epoch: Y_out must not be Y (vertices read the epoch-start map)");
    if (int rc = umap_epoch_args("umap_epoch", N, epoch, n_epochs, neg_rate)) return rc;
    RBVAE_CHECK_ARG(a > 0.f && b > 0.f && a <= 1e6f && b <= 16.f, "umap_epoch: a=%g, b=%g outside (0, 1e6] x (0, 16]",
                    (double)a, (double)b);
    RBVAE_CHECK_ARG(gamma >= 0.f && gamma <= 1e6f, "umap_epoch: gamma=%g outside 0..1e6", (double)gamma);
    RBVAE_CHECK_ARG((uintptr_t)Y % 8 == 0 && (uintptr_t)Y_out % 8 == 0, "umap_epoch: Y and Y_out must be 8-byte aligned");
    const float alpha = 1.0f - (float)epoch / (float)n_epochs;
    hipLaunchKernelGGL(umap_epoch_k, dim3(cdiv(N, UM_THREADS / 64)), dim3(UM_THREADS), 0, (hipStream_t)stream, Y, Y_out,
                       indptr, indices, period, next, next_neg, N, epoch, alpha, a, b, gamma, (float)neg_rate, seed);
    RBVAE_CHECK_LAUNCH("umap_epoch");
    return RBVAE_OK;
}

extern "C" int rbvae_umap_epoch_samples(const int* indptr, const float* period, const float* next, const float* next_neg,
                                        int N, int epoch, int n_epochs, int neg_rate, unsigned long long seed, int* count,
                                        int* samples, void* stream) {
    RBVAE_CHECK_ARG(indptr && period && next && next_neg && count && samples, "umap_epoch_samples: null pointer");
    if (int rc = umap_epoch_args("umap_epoch_samples", N, epoch, n_epochs, neg_rate)) return rc;
    hipLaunchKernelGGL(umap_samples_k, dim3(cdiv(N, UM_THREADS / 64)), dim3(UM_THREADS), 0, (hipStream_t)stream, indptr,
                       period, next, next_neg, N, epoch, (float)neg_rate, seed, count, samples);
    RBVAE_CHECK_LAUNCH("umap_epoch_samples");
    return RBVAE_OK;
}
