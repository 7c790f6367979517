// Latent scores (what scripts/evaluation/clustering_eval/embedding_umap.py leaves to the eye): the all-pairs reductions
// behind trustworthiness / continuity of a 2-D map and the silhouette of the labelled latents.  DESIGN.md section 7 has
// the formulation; scikit-learn 1.7.2 is the behaviour restated (scores.py finishes both on the host).
//   nbr_ranks_k            one workgroup per row i: its N squared distances in LDS as f64 (knn_k's row_d2, so the two
//                          kernels order a row identically), then a wave takes up to four of the row's given neighbours at
//                          a time and counts, a lane per m = lane (mod 64), the rows that come before each of them in the
//                          (d2, index) order
//   label_dist_sums_k      a workgroup owns 256 rows i (one per lane, the row in registers) and one state's segment of
//                          `order`: the segment's rows j pass through LDS as f64 in chunks, every lane reads them at the
//                          same address (broadcast) and adds sqrt(d2(i, j)) to its one accumulator in segment order
//   label_hamming_sums_k   the same walk over 128-bit code keys (bit = value > 0.5, as rbvae_state_vote packs them):
//                          popcount(key_i xor key_j) in int32
// No atomics: counts are integers, every f64 sum has one fixed order, two runs agree bit for bit.  Contraction is off.
#include "common.h"
#include "pairdist.h"

#include <math.h>

#pragma clang fp contract(off)

namespace rbvae {

constexpr int SC_THREADS = 256;
constexpr int SC_MAX_L = 128, SC_MAX_K = 128, SC_MAX_N = 16384, SC_MAX_S = 256;    // the first three are rbvae_knn's
constexpr int NR_GROUP = 4;             // neighbours a wave counts for in one pass over the row's distances
constexpr int LS_TI = 256;              // i rows per workgroup of the sums, one per lane
constexpr int LS_CHUNK = 4096;          // f64 values of j rows per LDS chunk (32 KB): LS_CHUNK / round_up(L, 8) rows
constexpr int LH_JC = 256;              // j keys per LDS chunk of the Hamming sums

// Dynamic LDS: dist f64 [N] | xq f64 [L] | the waves' excess [4]
__global__ __launch_bounds__(SC_THREADS) void nbr_ranks_k(const float* __restrict__ X, int N, int L,
                                                          const int* __restrict__ nbr, int k, int* __restrict__ rank,
                                                          int* __restrict__ excess) {
    extern __shared__ __attribute__((aligned(16))) double nr_lds[];
    double* dist = nr_lds;
    double* xq = dist + N;
    int* wex = (int*)(xq + L);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = blockIdx.x;
    for (int l = tid; l < L; l += SC_THREADS) xq[l] = (double)X[(long)i * L + l];
    __syncthreads();
    for (int j = tid; j < N; j += SC_THREADS) dist[j] = row_d2(xq, X + (long)j * L, L);
    __syncthreads();
    int ex = 0;                                             // the wave's share of excess[i]; every lane holds the same
    for (int r0 = wave; r0 < k; r0 += 4 * NR_GROUP) {       // this wave: r = r0, r0 + 4, r0 + 8, r0 + 12
        double dj[NR_GROUP];
        int jj[NR_GROUP], cnt[NR_GROUP];
        bool ok[NR_GROUP];
#pragma unroll
        for (int u = 0; u < NR_GROUP; ++u) {
            const int r = r0 + 4 * u;
            const int j = r < k ? nbr[(long)i * k + r] : -1;
            ok[u] = j >= 0 && j < N && j != i;              // rbvae_knn's 0x7fffffff, a negative entry, the row itself
            jj[u] = ok[u] ? j : 0;
            dj[u] = dist[jj[u]];
            cnt[u] = 0;
        }
        for (int m = lane; m < N; m += 64) {
            const double d = dist[m];
            const bool other = m != i;
#pragma unroll
            for (int u = 0; u < NR_GROUP; ++u) cnt[u] += (other && key_less(d, m, dj[u], jj[u])) ? 1 : 0;
        }
#pragma unroll
        for (int u = 0; u < NR_GROUP; ++u) {
            int c = cnt[u];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
            const int r = r0 + 4 * u;
            if (r < k) {
                const int rk = ok[u] ? c + 1 : -1;
                if (lane == 0) rank[(long)i * k + r] = rk;
                if (rk > k) ex += rk - k;
            }
        }
    }
    if (lane == 0) wex[wave] = ex;
    __syncthreads();
    if (tid == 0) excess[i] = wex[0] + wex[1] + wex[2] + wex[3];
}

// Static LDS only: xj f64 [LS_CHUNK] | okj [LS_CHUNK / 8]
__global__ __launch_bounds__(SC_THREADS) void label_dist_sums_k(const float* __restrict__ X, int N, int L,
                                                                const int* __restrict__ order,
                                                                const int* __restrict__ seg, int S,
                                                                double* __restrict__ sums) {
    __shared__ __attribute__((aligned(16))) double xj[LS_CHUNK];
    __shared__ int okj[LS_CHUNK / 8];
    const int tid = threadIdx.x;
    const int i = blockIdx.x * LS_TI + tid, s = blockIdx.y;
    const bool live = i < N;
    const int Lp = (L + 7) & ~7;                            // the row stride in LDS; the padding holds zeros
    const int JC = LS_CHUNK / Lp;
    float xi[SC_MAX_L];                                     // zeros beyond L: a padded coordinate adds an exact +0
#pragma unroll
    for (int l = 0; l < SC_MAX_L; ++l) xi[l] = (live && l < L) ? X[(long)i * L + l] : 0.f;
    const int jb = max(seg[s], 0), je = min(seg[s + 1], N);
    double acc = 0.0;
    for (int j0 = jb; j0 < je; j0 += JC) {
        const int n = min(JC, je - j0);
        __syncthreads();                                    // the previous chunk's reads are done
        for (int e = tid; e < n * Lp; e += SC_THREADS) {
            const int r = e / Lp, l = e - r * Lp;
            const int j = order[j0 + r];
            const bool ok = j >= 0 && j < N;
            xj[e] = (ok && l < L) ? (double)X[(long)j * L + l] : 0.0;
            if (l == 0) okj[r] = ok ? 1 : 0;
        }
        __syncthreads();
        for (int r = 0; r < n; ++r) {
            if (!okj[r]) continue;                          // the same in every lane
            const double* p = xj + r * Lp;                  // the same address in every lane: broadcast reads
            double d = 0.0;
#pragma unroll
            for (int l0 = 0; l0 < SC_MAX_L; l0 += 8) {
                if (l0 < L) {
#pragma unroll
                    for (int l = l0; l < l0 + 8; ++l) d2_step(d, (double)xi[l], p[l]);
                }
            }
            acc += sqrt(d);                                 // j == i: an exact 0
        }
    }
    if (live) sums[(long)i * S + s] = acc;
}

// the key of rbvae_state_vote's vote_pack_k: bit l of the code, first value in the highest bit of word 0
__device__ __forceinline__ uint4 code_key(const float* __restrict__ row, int L) {
    unsigned w[4] = {0u, 0u, 0u, 0u};
    for (int l = 0; l < L; ++l)
        if (row[l] > 0.5f) w[l >> 5] |= 1u << (31 - (l & 31));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

__global__ __launch_bounds__(SC_THREADS) void label_hamming_sums_k(const float* __restrict__ codes, int N, int L,
                                                                   const int* __restrict__ order,
                                                                   const int* __restrict__ seg, int S,
                                                                   int* __restrict__ sums) {
    __shared__ uint4 kj[LH_JC];
    __shared__ int okj[LH_JC];
    const int tid = threadIdx.x;
    const int i = blockIdx.x * LS_TI + tid, s = blockIdx.y;
    const bool live = i < N;
    const uint4 me = live ? code_key(codes + (long)i * L, L) : make_uint4(0u, 0u, 0u, 0u);
    const int jb = max(seg[s], 0), je = min(seg[s + 1], N);
    int acc = 0;
    for (int j0 = jb; j0 < je; j0 += LH_JC) {
        const int n = min(LH_JC, je - j0);
        __syncthreads();
        if (tid < n) {
            const int j = order[j0 + tid];
            const bool ok = j >= 0 && j < N;
            kj[tid] = ok ? code_key(codes + (long)j * L, L) : make_uint4(0u, 0u, 0u, 0u);
            okj[tid] = ok ? 1 : 0;
        }
        __syncthreads();
        for (int t = 0; t < n; ++t) {
            if (!okj[t]) continue;
            const uint4 q = kj[t];
            acc += __popc(me.x ^ q.x) + __popc(me.y ^ q.y) + __popc(me.z ^ q.z) + __popc(me.w ^ q.w);
        }
    }
    if (live) sums[(long)i * S + s] = acc;
}

static size_t ranks_lds_bytes(int N, int L) { return ((size_t)N + L) * sizeof(double) + 4 * sizeof(int); }

}  // namespace rbvae

using namespace rbvae;

extern "C" int rbvae_nbr_ranks_ok(int N, int L, int k) {
    return N >= 2 && N <= SC_MAX_N && L >= 1 && L <= SC_MAX_L && k >= 1 && k <= SC_MAX_K && k <= N - 1;
}

extern "C" int rbvae_nbr_ranks(const float* X, int N, int L, const int* nbr, int k, int* rank, int* excess, void* stream) {
    RBVAE_CHECK_ARG(X && nbr && rank && excess, "nbr_ranks: null pointer");
    RBVAE_CHECK_ARG(N >= 2 && N <= SC_MAX_N, "nbr_ranks: N=%d outside 2..%d (all N distances of a row stay in LDS)", N,
                    SC_MAX_N);
    RBVAE_CHECK_ARG(L >= 1 && L <= SC_MAX_L, "nbr_ranks: L=%d outside 1..%d", L, SC_MAX_L);
    RBVAE_CHECK_ARG(k >= 1 && k <= SC_MAX_K && k <= N - 1, "nbr_ranks: k=%d outside 1..min(N - 1, %d), N=%d", k, SC_MAX_K, N);
    const size_t lds = ranks_lds_bytes(N, L);
    static size_t reserved = 0;                             // process-wide, as rbvae_knn's
    if (lds > reserved) {
        if (hipFuncSetAttribute((const void*)nbr_ranks_k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return fail(RBVAE_E_LAUNCH, "nbr_ranks: cannot reserve %zu bytes of LDS", lds);
        reserved = lds;
    }
    hipLaunchKernelGGL(nbr_ranks_k, dim3(N), dim3(SC_THREADS), lds, (hipStream_t)stream, X, N, L, nbr, k, rank, excess);
    RBVAE_CHECK_LAUNCH("nbr_ranks");
    return RBVAE_OK;
}

extern "C" int rbvae_label_sums_ok(int N, int L, int S) {
    return N >= 1 && N <= SC_MAX_N && L >= 1 && L <= SC_MAX_L && S >= 1 && S <= SC_MAX_S;
}

#define LABEL_SUMS_CHECK(name, X, sums)                                                                               \
    RBVAE_CHECK_ARG(X && order && seg && sums, name ": null pointer");                                                \
    RBVAE_CHECK_ARG(N >= 1 && N <= SC_MAX_N, name ": N=%d outside 1..%d", N, SC_MAX_N);                               \
    RBVAE_CHECK_ARG(L >= 1 && L <= SC_MAX_L, name ": L=%d outside 1..%d", L, SC_MAX_L);                               \
    RBVAE_CHECK_ARG(S >= 1 && S <= SC_MAX_S, name ": S=%d states outside 1..%d", S, SC_MAX_S)

extern "C" int rbvae_label_dist_sums(const float* X, int N, int L, const int* order, const int* seg, int S, double* sums,
                                     void* stream) {
    LABEL_SUMS_CHECK("label_dist_sums", X, sums);
    hipLaunchKernelGGL(label_dist_sums_k, dim3(cdiv(N, LS_TI), S), dim3(SC_THREADS), 0, (hipStream_t)stream, X, N, L, order,
                       seg, S, sums);
    RBVAE_CHECK_LAUNCH("label_dist_sums");
    return RBVAE_OK;
}

extern "C" int rbvae_label_hamming_sums(const float* codes, int N, int L, const int* order, const int* seg, int S, int* sums,
                                        void* stream) {
    LABEL_SUMS_CHECK("label_hamming_sums", codes, sums);
    hipLaunchKernelGGL(label_hamming_sums_k, dim3(cdiv(N, LS_TI), S), dim3(SC_THREADS), 0, (hipStream_t)stream, codes, N, L,
                       order, seg, S, sums);
    RBVAE_CHECK_LAUNCH("label_hamming_sums");
    return RBVAE_OK;
}
