// Latent-space projections (scripts/evaluation/clustering_eval/embedding_umap.py:58-128): the exact k-nearest-neighbour
// graph t-SNE and UMAP start from, t-SNE's perplexity search and gradient iteration, and the moments / projection of an
// exact PCA.  DESIGN.md section 7 has the formulation; scikit-learn 1.7.2 is the behaviour restated.
//   knn_k            one workgroup per query row: all N squared distances in LDS as f64, then k rounds of a block-wide
//                    minimum over the keys (d2, j); a thread owns the candidates j = t (mod 256) and rescans only after
//                    one of its own was taken
//   tsne_perp_k      sklearn.manifold._utils._binary_search_perplexity, one wave per row, two neighbours per lane
//   tsne_repulse_k   R_i = sum_j q^2 (y_i - y_j), Z_i = sum_j q over one slice of j, q = 1 / (1 + |y_i - y_j|^2): a lane
//                    keeps one i, the j points come from LDS at a wave-uniform address (broadcast)
//   tsne_zsum_k      Z = the sum of every part[s][i][2] in f64, one workgroup of 1024 threads, fixed order
//   tsne_step_k      one wave per CSR row: attraction, gradient, scikit-learn's _gradient_descent update, and the
//                    workgroup's f64 partials of |g|^2, |gains g|^2 and the sparse KL
//   pca_mean_k / pca_cov_k / pca_project_k   f64 moments of centred rows and (X - mean) V^T
// No float atomics: every sum has a fixed order, two runs agree bit for bit.  Contraction is off: sums round where the
// text says they do, fused products are explicit fma calls.
#include "common.h"
#include "pairdist.h"

#include <float.h>
#include <math.h>

#pragma clang fp contract(off)

namespace rbvae {

constexpr int PJ_THREADS = 256;
constexpr int PJ_MAX_L = 128, PJ_MAX_K = 128, PJ_MAX_N = 16384, PJ_MAX_COMP = 8;
constexpr int RP_TI = 256;              // i rows per workgroup of the repulsion, one per lane
constexpr int RP_JC = 256;              // j points per LDS chunk; a chunk's sums start from zero

// Dynamic LDS: dist f64 [N] | xq f64 [L] | wave minima d [2][4] | out_d f64 [k] | wave minima j [2][4] | out_j [k]
__global__ __launch_bounds__(PJ_THREADS) void knn_k(const float* __restrict__ X, int N, int L, int k,
                                                    int* __restrict__ idx, double* __restrict__ d2) {
    extern __shared__ __attribute__((aligned(16))) double kn_lds[];
    double* dist = kn_lds;
    double* xq = dist + N;
    double* wd = xq + L;
    double* out_d = wd + 8;
    int* wj = (int*)(out_d + k);
    int* out_j = wj + 8;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = blockIdx.x;
    for (int l = tid; l < L; l += PJ_THREADS) xq[l] = (double)X[(long)i * L + l];
    __syncthreads();
    const double inf = __builtin_huge_val();
    double ld = inf;
    int lj = 0x7fffffff;
    for (int j = tid; j < N; j += PJ_THREADS) {             // ascending j: the first minimum is the lowest index
        double s = row_d2(xq, X + (long)j * L, L);
        if (j == i) s = inf;
        dist[j] = s;
        if (s < ld) { ld = s; lj = j; }
    }
    for (int r = 0; r < k; ++r) {
        double bd = ld;
        int bj = lj;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double od = __shfl_xor(bd, o, 64);
            const int oj = __shfl_xor(bj, o, 64);
            if (key_less(od, oj, bd, bj)) { bd = od; bj = oj; }
        }
        const int slot = (r & 1) * 4;
        if (lane == 0) { wd[slot + wave] = bd; wj[slot + wave] = bj; }
        __syncthreads();
        bd = wd[slot];
        bj = wj[slot];
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (key_less(wd[slot + w], wj[slot + w], bd, bj)) { bd = wd[slot + w]; bj = wj[slot + w]; }
        if (tid == 0) { out_d[r] = bd; out_j[r] = bj; }
        // the owner takes it out and finds the next of its own.  bj < N: with non-finite rows fewer than k finite keys
        // can remain; the minimum is then (inf, 0x7fffffff), which every thread holds and none may store through
        if (bj < N && bj == lj && bd == ld) {
            dist[bj] = inf;
            ld = inf;
            lj = 0x7fffffff;
            for (int j = tid; j < N; j += PJ_THREADS) {
                const double s = dist[j];
                if (s < ld) { ld = s; lj = j; }
            }
        }
    }
    __syncthreads();
    for (int r = tid; r < k; r += PJ_THREADS) {
        idx[(long)i * k + r] = out_j[r];
        d2[(long)i * k + r] = out_d[r];
    }
}

// _binary_search_perplexity on one row per wave: lane l holds neighbours l and l + 64.
__global__ __launch_bounds__(PJ_THREADS) void tsne_perp_k(const double* __restrict__ d2, int N, int k, double want_entropy,
                                                          double* __restrict__ P, double* __restrict__ beta_out,
                                                          int* __restrict__ steps) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * (PJ_THREADS / 64) + (threadIdx.x >> 6);
    if (i >= N) return;
    const double eps_dbl = (double)1e-8f, tol = (double)1e-5f;  // the .pyx declares both as C floats
    const double inf = __builtin_huge_val();
    const bool h0 = lane < k, h1 = lane + 64 < k;
    const double d0 = h0 ? (double)(float)d2[(long)i * k + lane] : 0.0;
    const double d1 = h1 ? (double)(float)d2[(long)i * k + lane + 64] : 0.0;
    double beta = 1.0, bmin = -inf, bmax = inf, p0 = 0.0, p1 = 0.0, used = 1.0;
    int n = 0;
    for (int l = 0; l < 100; ++l) {
        p0 = h0 ? exp(-d0 * beta) : 0.0;
        p1 = h1 ? exp(-d1 * beta) : 0.0;
        double sum = wave_sum_f64(p0 + p1);
        if (sum == 0.0) sum = eps_dbl;
        p0 /= sum;
        p1 /= sum;
        const double sdp = wave_sum_f64(d0 * p0 + d1 * p1);
        const double diff = (log(sum) + beta * sdp) - want_entropy;
        used = beta;
        n = l + 1;
        if (fabs(diff) <= tol) break;
        if (diff > 0.0) {
            bmin = beta;
            beta = bmax == inf ? beta * 2.0 : (beta + bmax) / 2.0;
        } else {
            bmax = beta;
            beta = bmin == -inf ? beta / 2.0 : (beta + bmin) / 2.0;
        }
    }
    if (h0) P[(long)i * k + lane] = p0;
    if (h1) P[(long)i * k + lane + 64] = p1;
    if (lane == 0) { beta_out[i] = used; steps[i] = n; }
}

// j points ys[0..n) against the lane's point; MASK: the chunk holds the lane's own index i = j0 + t for some t
template <bool MASK>
__device__ __forceinline__ void repulse_chunk(const float2* ys, int n, int self, float xi, float yi, float& rx, float& ry,
                                              float& z) {
#pragma unroll 8
    for (int t = 0; t < n; ++t) {
        const float2 p = ys[t];                             // the same address in every lane: one broadcast read
        const float dx = xi - p.x, dy = yi - p.y;
        const float den = 1.0f + fmaf(dy, dy, dx * dx);
        float q = __builtin_amdgcn_rcpf(den);
        if (MASK) q = t == self ? 0.0f : q;
        z += q;
        const float q2 = q * q;
        rx = fmaf(q2, dx, rx);
        ry = fmaf(q2, dy, ry);
    }
}

__global__ __launch_bounds__(PJ_THREADS) void tsne_repulse_k(const float* __restrict__ Y, int N, float* __restrict__ part,
                                                             int slice) {
    __shared__ float2 ys[RP_JC];
    const int tid = threadIdx.x;
    const int i0 = blockIdx.x * RP_TI, i = i0 + tid;
    const bool live = i < N;
    const float2 me = live ? ((const float2*)Y)[i] : float2{0.f, 0.f};
    const int jb = blockIdx.y * slice, je = min(N, jb + slice);
    float Rx = 0.f, Ry = 0.f, Z = 0.f;
    for (int j0 = jb; j0 < je; j0 += RP_JC) {
        const int n = min(RP_JC, je - j0);
        __syncthreads();                                    // the previous chunk's reads are done
        if (tid < n) ys[tid] = ((const float2*)Y)[j0 + tid];
        __syncthreads();
        float rx = 0.f, ry = 0.f, z = 0.f;
        if (j0 < i0 + RP_TI && j0 + n > i0) repulse_chunk<true>(ys, n, i - j0, me.x, me.y, rx, ry, z);
        else repulse_chunk<false>(ys, n, 0, me.x, me.y, rx, ry, z);
        Rx += rx;
        Ry += ry;
        Z += z;
    }
    if (live) {
        float* o = part + ((long)blockIdx.y * N + i) * 3;
        o[0] = Rx;
        o[1] = Ry;
        o[2] = Z;
    }
}

// One workgroup of 1024 threads over the n = splits x N partial sums in memory order: thread t adds the elements t,
// t + 1024, ... in ascending order (eight loads in flight), then the tree.
constexpr int ZS_THREADS = 1024, ZS_UNROLL = 8;
__global__ __launch_bounds__(ZS_THREADS) void tsne_zsum_k(const float* __restrict__ part, long n, double* __restrict__ Z) {
    __shared__ double red[ZS_THREADS];
    double acc = 0.0;
    for (long e0 = threadIdx.x; e0 < n; e0 += (long)ZS_THREADS * ZS_UNROLL) {
        float v[ZS_UNROLL];
#pragma unroll
        for (int u = 0; u < ZS_UNROLL; ++u) {
            const long e = e0 + (long)u * ZS_THREADS;
            v[u] = e < n ? part[e * 3 + 2] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < ZS_UNROLL; ++u) acc += (double)v[u];
    }
    const double tot = block_tree_sum<ZS_THREADS>(acc, red);
    if (threadIdx.x == 0) Z[0] = tot;
}

// sched = (exaggeration, momentum, learning rate) on the device.  Y is read, Y_out written: a neighbour's row may belong
// to another workgroup.
__global__ __launch_bounds__(PJ_THREADS) void tsne_step_k(const float* __restrict__ Y, float* __restrict__ Y_out,
                                                          float* __restrict__ update, float* __restrict__ gains,
                                                          const int* __restrict__ indptr, const int* __restrict__ indices,
                                                          const float* __restrict__ data, const float* __restrict__ part,
                                                          int splits, const double* __restrict__ Zp,
                                                          const float* __restrict__ sched, int N,
                                                          double* __restrict__ stats) {
    __shared__ double wst[4][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * (PJ_THREADS / 64) + wave;
    const float exag = sched[0], mom = sched[1], lr = sched[2];
    const double Z = Zp[0];
    double gg = 0.0, sgg = 0.0, kl = 0.0;
    if (i < N) {
        const float2 me = ((const float2*)Y)[i];
        float ax = 0.f, ay = 0.f;
        for (int e = indptr[i] + lane; e < indptr[i + 1]; e += 64) {
            const float2 p = ((const float2*)Y)[indices[e]];
            const float pe = exag * data[e];
            const float dx = me.x - p.x, dy = me.y - p.y;
            const float q = 1.0f / (1.0f + fmaf(dy, dy, dx * dx));
            const float w = pe * q;
            ax = fmaf(w, dx, ax);
            ay = fmaf(w, dy, ay);
            kl += (double)pe * log(fmax((double)pe, (double)FLT_MIN) / fmax((double)q / Z, (double)FLT_MIN));
        }
        ax = wave_sum(ax);
        ay = wave_sum(ay);
        kl = wave_sum_f64(kl);
        if (lane < 2) {                                     // lane c owns coordinate c
            float r = 0.f;
            for (int s = 0; s < splits; ++s) r += part[((long)s * N + i) * 3 + lane];
            const float a = lane ? ay : ax;
            const float g = 4.0f * (float)((double)a - (double)r / Z);
            float u = update[2 * i + lane], gn = gains[2 * i + lane];
            gn = u * g < 0.0f ? gn + 0.2f : gn * 0.8f;
            gn = fmaxf(gn, 0.01f);
            const float sg = gn * g;
            u = mom * u - lr * sg;
            gains[2 * i + lane] = gn;
            update[2 * i + lane] = u;
            Y_out[2 * i + lane] = (lane ? me.y : me.x) + u;
            gg = (double)g * (double)g;
            sgg = (double)sg * (double)sg;
        }
        gg += __shfl_xor(gg, 1, 64);                        // lanes 0 and 1: x + y
        sgg += __shfl_xor(sgg, 1, 64);
    }
    if (lane == 0) { wst[wave][0] = gg; wst[wave][1] = sgg; wst[wave][2] = kl; }
    __syncthreads();
    if (threadIdx.x < 3) {
        double s = wst[0][threadIdx.x];
        for (int w = 1; w < 4; ++w) s += wst[w][threadIdx.x];
        stats[(long)blockIdx.x * 3 + threadIdx.x] = s;
    }
}

// mean[l] = (sum_rows x) / N: one workgroup per column, thread t adds rows t, t + 256, ... in order, then the tree
__global__ __launch_bounds__(PJ_THREADS) void pca_mean_k(const float* __restrict__ X, int N, int L, double* __restrict__ mean) {
    __shared__ double red[PJ_THREADS];
    const int l = blockIdx.x;
    double s = 0.0;
    for (int r = threadIdx.x; r < N; r += PJ_THREADS) s += (double)X[(long)r * L + l];
    const double tot = block_tree_sum<PJ_THREADS>(s, red);
    if (threadIdx.x == 0) mean[l] = tot / (double)N;
}

// cov[a][b] = cov[b][a] = sum_rows (x_a - mean_a)(x_b - mean_b) / (N - 1), a <= b: one workgroup per pair
__global__ __launch_bounds__(PJ_THREADS) void pca_cov_k(const float* __restrict__ X, int N, int L,
                                                        const double* __restrict__ mean, double* __restrict__ cov) {
    __shared__ double red[PJ_THREADS];
    const int a = blockIdx.x, b = blockIdx.y;
    if (a > b) return;
    const double ma = mean[a], mb = mean[b];
    double s = 0.0;
    for (int r = threadIdx.x; r < N; r += PJ_THREADS) {
        const double ca = (double)X[(long)r * L + a] - ma, cb = (double)X[(long)r * L + b] - mb;
        s += ca * cb;
    }
    const double tot = block_tree_sum<PJ_THREADS>(s, red);
    if (threadIdx.x == 0) {
        const double v = tot / (double)(N - 1);
        cov[(long)a * L + b] = v;
        cov[(long)b * L + a] = v;
    }
}

// out[i][c] = sum_l (x_il - mean_l) V[c][l], l ascending, products and sums rounded separately
__global__ __launch_bounds__(PJ_THREADS) void pca_project_k(const float* __restrict__ X, int N, int L,
                                                            const double* __restrict__ mean, const double* __restrict__ V,
                                                            int nc, double* __restrict__ out) {
    __shared__ double vs[PJ_MAX_COMP * PJ_MAX_L];
    __shared__ double ms[PJ_MAX_L];
    for (int t = threadIdx.x; t < nc * L; t += PJ_THREADS) vs[t] = V[t];
    for (int t = threadIdx.x; t < L; t += PJ_THREADS) ms[t] = mean[t];
    __syncthreads();
    const int i = blockIdx.x * PJ_THREADS + threadIdx.x;
    if (i >= N) return;
    double acc[PJ_MAX_COMP];
#pragma unroll
    for (int c = 0; c < PJ_MAX_COMP; ++c) acc[c] = 0.0;
    for (int l = 0; l < L; ++l) {
        const double x = (double)X[(long)i * L + l] - ms[l];
#pragma unroll
        for (int c = 0; c < PJ_MAX_COMP; ++c)
            if (c < nc) acc[c] += x * vs[c * L + l];
    }
#pragma unroll
    for (int c = 0; c < PJ_MAX_COMP; ++c)
        if (c < nc) out[(long)i * nc + c] = acc[c];
}

// j slices of the repulsion: none while the i tiles alone give ~1024 workgroups, else whole chunks of RP_JC points
static void repulse_shape(int N, int* splits, int* slice) {
    const int tiles = cdiv(N, RP_TI), chunks = cdiv(N, RP_JC);
    int s = cdiv(1024, tiles);
    if (s > chunks) s = chunks;
    const int per = cdiv(chunks, s);
    *slice = per * RP_JC;
    *splits = cdiv(chunks, per);
}

static size_t knn_lds_bytes(int N, int L, int k) {
    return ((size_t)N + L + 8 + k) * sizeof(double) + ((size_t)8 + k) * sizeof(int);
}

}  // namespace rbvae

using namespace rbvae;

extern "C" int rbvae_knn_ok(int N, int L, int k) {
    return N >= 2 && N <= PJ_MAX_N && L >= 1 && L <= PJ_MAX_L && k >= 1 && k <= PJ_MAX_K && k <= N - 1;
}

extern "C" int rbvae_knn(const float* X, int N, int L, int k, int* idx, double* d2, void* stream) {
    RBVAE_CHECK_ARG(X && idx && d2, "knn: null pointer");
    RBVAE_CHECK_ARG(N >= 2 && N <= PJ_MAX_N, "knn: N=%d outside 2..%d (all N distances of a row stay in LDS)", N, PJ_MAX_N);
    RBVAE_CHECK_ARG(L >= 1 && L <= PJ_MAX_L, "knn: L=%d outside 1..%d", L, PJ_MAX_L);
    RBVAE_CHECK_ARG(k >= 1 && k <= PJ_MAX_K && k <= N - 1, "knn: k=%d outside 1..min(N - 1, %d), N=%d", k, PJ_MAX_K, N);
    const size_t lds = knn_lds_bytes(N, L, k);
    // process-wide like the other kernels' opt-in flags: one device per process, entry points called from one thread
    static size_t reserved = 0;
    if (lds > reserved) {
        if (hipFuncSetAttribute((const void*)knn_k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return fail(RBVAE_E_LAUNCH, "knn: cannot reserve %zu bytes of LDS", lds);
        reserved = lds;
    }
    hipLaunchKernelGGL(knn_k, dim3(N), dim3(PJ_THREADS), lds, (hipStream_t)stream, X, N, L, k, idx, d2);
    RBVAE_CHECK_LAUNCH("knn");
    return RBVAE_OK;
}

extern "C" int rbvae_tsne_perplexity(const double* d2, int N, int k, float perplexity, double* P, double* beta, int* steps,
                                     void* stream) {
    RBVAE_CHECK_ARG(d2 && P && beta && steps, "tsne_perplexity: null pointer");
    RBVAE_CHECK_ARG(N >= 1, "tsne_perplexity: N=%d, need at least one row", N);
    RBVAE_CHECK_ARG(k >= 1 && k <= PJ_MAX_K, "tsne_perplexity: k=%d outside 1..%d", k, PJ_MAX_K);
    RBVAE_CHECK_ARG(perplexity > 0.f && perplexity < (float)k,
                    "tsne_perplexity: perplexity %g must be positive and below the k=%d neighbours", (double)perplexity, k);
    hipLaunchKernelGGL(tsne_perp_k, dim3(cdiv(N, PJ_THREADS / 64)), dim3(PJ_THREADS), 0, (hipStream_t)stream, d2, N, k,
                       log((double)perplexity), P, beta, steps);
    RBVAE_CHECK_LAUNCH("tsne_perplexity");
    return RBVAE_OK;
}

extern "C" int rbvae_tsne_repulse_splits(int N) {
    if (N < 1) return 0;
    int splits, slice;
    repulse_shape(N, &splits, &slice);
    return splits;
}

extern "C" int rbvae_tsne_repulse(const float* Y, int N, float* part, void* stream) {
    RBVAE_CHECK_ARG(Y && part, "tsne_repulse: null pointer");
    RBVAE_CHECK_ARG(N >= 1, "tsne_repulse: N=%d, need at least one point", N);
    RBVAE_CHECK_ARG((uintptr_t)Y % 8 == 0, "tsne_repulse: Y must be 8-byte aligned");
    int splits, slice;
    repulse_shape(N, &splits, &slice);
    RBVAE_CHECK_ARG(splits <= 65535, "tsne_repulse: N=%d too large", N);
    hipLaunchKernelGGL(tsne_repulse_k, dim3(cdiv(N, RP_TI), splits), dim3(PJ_THREADS), 0, (hipStream_t)stream, Y, N, part,
                       slice);
    RBVAE_CHECK_LAUNCH("tsne_repulse");
    return RBVAE_OK;
}

extern "C" int rbvae_tsne_zsum(const float* part, int N, double* Z, void* stream) {
    RBVAE_CHECK_ARG(part && Z, "tsne_zsum: null pointer");
    RBVAE_CHECK_ARG(N >= 1, "tsne_zsum: N=%d, need at least one point", N);
    int splits, slice;
    repulse_shape(N, &splits, &slice);
    hipLaunchKernelGGL(tsne_zsum_k, dim3(1), dim3(ZS_THREADS), 0, (hipStream_t)stream, part, (long)splits * N, Z);
    RBVAE_CHECK_LAUNCH("tsne_zsum");
    return RBVAE_OK;
}

extern "C" int rbvae_tsne_step_parts(int N) { return N >= 1 ? cdiv(N, PJ_THREADS / 64) : 0; }

extern "C" int rbvae_tsne_step(const float* Y, float* Y_out, float* update, float* gains, const int* indptr,
                               const int* indices, const float* data, const float* part, const double* Z,
                               const float* sched, int N, double* stats, void* stream) {
    RBVAE_CHECK_ARG(Y && Y_out && update && gains && indptr && indices && data && part && Z && sched && stats,
                    "tsne_step: null pointer");
    RBVAE_CHECK_ARG(Y != Y_out, "tsne_step: Y_out must not be Y (rows read their neighbours)");
    RBVAE_CHECK_ARG(N >= 2, "tsne_step: N=%d, need at least two points", N);
    RBVAE_CHECK_ARG((uintptr_t)Y % 8 == 0, "tsne_step: Y must be 8-byte aligned");
    int splits, slice;
    repulse_shape(N, &splits, &slice);
    hipLaunchKernelGGL(tsne_step_k, dim3(cdiv(N, PJ_THREADS / 64)), dim3(PJ_THREADS), 0, (hipStream_t)stream, Y, Y_out,
                       update, gains, indptr, indices, data, part, splits, Z, sched, N, stats);
    RBVAE_CHECK_LAUNCH("tsne_step");
    return RBVAE_OK;
}

extern "C" int rbvae_pca_moments(const float* X, int N, int L, double* mean, double* cov, void* stream) {
    RBVAE_CHECK_ARG(X && mean && cov, "pca_moments: null pointer");
    RBVAE_CHECK_ARG(N >= 2, "pca_moments: N=%d, need at least two rows", N);
    RBVAE_CHECK_ARG(L >= 1 && L <= PJ_MAX_L, "pca_moments: L=%d outside 1..%d", L, PJ_MAX_L);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(pca_mean_k, dim3(L), dim3(PJ_THREADS), 0, st, X, N, L, mean);
    RBVAE_CHECK_LAUNCH("pca_moments (mean)");
    hipLaunchKernelGGL(pca_cov_k, dim3(L, L), dim3(PJ_THREADS), 0, st, X, N, L, mean, cov);
    RBVAE_CHECK_LAUNCH("pca_moments (covariance)");
    return RBVAE_OK;
}

extern "C" int rbvae_pca_project(const float* X, int N, int L, const double* mean, const double* V, int n_components,
                                 double* out, void* stream) {
    RBVAE_CHECK_ARG(X && mean && V && out, "pca_project: null pointer");
    RBVAE_CHECK_ARG(N >= 1, "pca_project: N=%d, need at least one row", N);
    RBVAE_CHECK_ARG(L >= 1 && L <= PJ_MAX_L, "pca_project: L=%d outside 1..%d", L, PJ_MAX_L);
    RBVAE_CHECK_ARG(n_components >= 1 && n_components <= PJ_MAX_COMP && n_components <= L,
                    "pca_project: n_components=%d outside 1..min(L, %d)", n_components, PJ_MAX_COMP);
    hipLaunchKernelGGL(pca_project_k, dim3(cdiv(N, PJ_THREADS)), dim3(PJ_THREADS), 0, (hipStream_t)stream, X, N, L, mean, V,
                       n_components, out);
    RBVAE_CHECK_LAUNCH("pca_project");
    return RBVAE_OK;
}
