// Linear probe evaluation (scripts/evaluation/linear_projection_eval/linear_regression_eval.py:123-144): the
// multi-output least-squares fit from an embedding (L <= 128 values) to the flattened frame (P targets) and its
// held-out metrics, in f64, on targets that stay resident as u8 [N][H][W][3] (or f32 [N][P]).
//   probe_xty_k        C[M][P] = B^T (Y[rows] - y0) on v_mfma_f64_16x16x4_f64; B [n_rows][M] is the host's fit factor
//                      (M = L + 1: the minimum-norm operator's transpose and the column 1 / n_rows), y0 = Y[row0]
//   probe_slab_sum_k   the split-K slabs of C summed in slab order (bitwise reproducible)
//   probe_intercept_k  intercept = (C[L] - sum_l mean_x[l] C[l]) + y0, l ascending
//   probe_residual_k   per target, over the test rows: sum e, sum e^2, sum |e| (e = y - (intercept + x W)) and
//                      sum d, sum d^2 (d = y - Y[row0])
//   probe_scores_k / probe_means_k   r2 and explained variance per target (scikit-learn's force_finite rule), then
//                      their uniform means, mse, mae and the number of constant targets, reduced in a fixed order
// A u8 target is ToTensor's (float)v / 255.0f (the expression of u8_to_input_k in frames.hip) widened to f64; every
// difference y - y0 of two such values is exact in f64, so a target that is constant over the rows gives C = 0, a zero
// residual and SStot == 0 exactly.  Rows are addressed through an int32 list; an index outside [0, N) contributes zero.
// Contraction is off: the sums round where the text above says they do; the dot product of the prediction is an
// explicit fma chain.
#include "common.h"

#pragma clang fp contract(off)

namespace rbvae {

typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr int PB_THREADS = 256;
constexpr int PB_TP = 256;              // targets per workgroup: 4 waves x 4 n-tiles of 16
constexpr int PB_KB = 16;               // rows per K block: 4 MFMA k-steps
constexpr int PB_MG = 3;                // m-tiles (of 16 rows of C) per workgroup; blockIdx.y walks the groups
constexpr int PB_YLD = PB_TP + 16;      // f32 row stride of the staged target tile: the 4 rows of a k-step hit distinct banks
constexpr int PB_FLD = 16 * PB_MG;      // f64 row stride of the staged factor block
constexpr int PB_RT = 64;               // targets per workgroup of the residual pass (4 row groups x 64 lanes)

template <typename T> struct Tgt;
template <> struct Tgt<unsigned char> {
    static constexpr int PIECE = 16;    // elements per 16-byte piece
    static __device__ __forceinline__ float val(unsigned char v) { return (float)v / 255.0f; }
    static __device__ __forceinline__ void unpack(const uint4& q, float* f) {
        const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int i = 0; i < 16; ++i) f[i] = (float)((w[i >> 2] >> (8 * (i & 3))) & 0xffu) / 255.0f;
    }
};
template <> struct Tgt<float> {
    static constexpr int PIECE = 4;
    static __device__ __forceinline__ float val(float v) { return v; }
    static __device__ __forceinline__ void unpack(const uint4& q, float* f) {
        f[0] = __uint_as_float(q.x); f[1] = __uint_as_float(q.y); f[2] = __uint_as_float(q.z); f[3] = __uint_as_float(q.w);
    }
};

// One workgroup: 256 targets x up to 48 rows of C over one slab of the row list.  Per K block of 16 rows the target
// tile is staged as f32 in LDS with 16-byte global loads (whole pieces per lane; element loads when P or the base
// pointer breaks the 16-byte alignment of the rows) and the factor block as f64; a row past the list's end or with an
// index outside [0, N) is staged as zeros in both, so it adds 0 * (0 - y0) = 0.  MFMA operands (f64 16x16x4): lane l
// holds A[row l & 15][k l >> 4] = B[k][m] and B[k l >> 4][col l & 15] = y - y0 of target l & 15; result register i of
// lane l is C[row (l >> 4) + 4 i][col l & 15].
template <typename T>
__global__ __launch_bounds__(PB_THREADS) void probe_xty_k(const T* __restrict__ Y, long N, long P,
                                                          const int* __restrict__ rows, int n_rows, int row0,
                                                          const double* __restrict__ Bf, int M, double* __restrict__ out,
                                                          int blocks_per_slab, int vec) {
    __shared__ __attribute__((aligned(16))) float ys[PB_KB][PB_YLD];
    __shared__ double fb[PB_KB][PB_FLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long p0 = (long)blockIdx.x * PB_TP;
    const int m0 = blockIdx.y * PB_FLD;
    const int mtiles = min(PB_MG, (M - m0 + 15) >> 4);
    const int nblocks = (n_rows + PB_KB - 1) / PB_KB;
    const int kb0 = blockIdx.z * blocks_per_slab, kb1 = min(nblocks, kb0 + blocks_per_slab);
    const int lc = lane & 15, lk = lane >> 4;

    double y0v[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        const long p = p0 + wave * 64 + nt * 16 + lc;
        y0v[nt] = p < P ? (double)Tgt<T>::val(Y[(long)row0 * P + p]) : 0.0;
    }
    double4_t acc[PB_MG][4];
#pragma unroll
    for (int mt = 0; mt < PB_MG; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = double4_t{0.0, 0.0, 0.0, 0.0};

    for (int kb = kb0; kb < kb1; ++kb) {
        const int k0 = kb * PB_KB;
        __syncthreads();                                    // the previous block's fragment reads are done
        for (int i = tid; i < PB_KB * PB_FLD; i += PB_THREADS) {
            const int r = i / PB_FLD, j = i - r * PB_FLD;
            double v = 0.0;
            if (k0 + r < n_rows && m0 + j < M) {
                const int ri = rows[k0 + r];
                if (ri >= 0 && ri < N) v = Bf[(long)(k0 + r) * M + m0 + j];
            }
            fb[r][j] = v;
        }
        if (vec) {
            constexpr int PC = Tgt<T>::PIECE, PPR = PB_TP / PC;
            for (int i = tid; i < PB_KB * PPR; i += PB_THREADS) {
                const int r = i / PPR, c = (i - r * PPR) * PC;
                float f[PC];
#pragma unroll
                for (int e = 0; e < PC; ++e) f[e] = 0.f;
                if (k0 + r < n_rows && p0 + c < P) {        // P % PC == 0: a piece is inside the row or outside it
                    const int ri = rows[k0 + r];
                    if (ri >= 0 && ri < N) Tgt<T>::unpack(*(const uint4*)(Y + (long)ri * P + p0 + c), f);
                }
#pragma unroll
                for (int e = 0; e < PC; e += 4) *(float4*)&ys[r][c + e] = float4{f[e], f[e + 1], f[e + 2], f[e + 3]};
            }
        } else {
            for (int i = tid; i < PB_KB * PB_TP; i += PB_THREADS) {
                const int r = i / PB_TP, c = i - r * PB_TP;
                float v = 0.f;
                if (k0 + r < n_rows && p0 + c < P) {
                    const int ri = rows[k0 + r];
                    if (ri >= 0 && ri < N) v = Tgt<T>::val(Y[(long)ri * P + p0 + c]);
                }
                ys[r][c] = v;
            }
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < PB_KB / 4; ++ks) {
            const int kr = ks * 4 + lk;
            double a[PB_MG];
#pragma unroll
            for (int mt = 0; mt < PB_MG; ++mt) a[mt] = fb[kr][mt * 16 + lc];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const double b = (double)ys[kr][wave * 64 + nt * 16 + lc] - y0v[nt];
#pragma unroll
                for (int mt = 0; mt < PB_MG; ++mt)
                    if (mt < mtiles) acc[mt][nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mt], b, acc[mt][nt], 0, 0, 0);
            }
        }
    }

    double* dst = out + (long)blockIdx.z * M * P;
#pragma unroll
    for (int mt = 0; mt < PB_MG; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            const long p = p0 + wave * 64 + nt * 16 + lc;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int m = m0 + mt * 16 + lk + 4 * i;
                if (mt < mtiles && m < M && p < P) dst[(long)m * P + p] = acc[mt][nt][i];
            }
        }
}

// C[i] = ws[0][i] + ws[1][i] + ... in slab order
__global__ __launch_bounds__(PB_THREADS) void probe_slab_sum_k(const double* __restrict__ ws, double* __restrict__ C,
                                                               long n, int slabs) {
    for (long i = (long)blockIdx.x * PB_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * PB_THREADS) {
        double s = ws[i];
        for (int z = 1; z < slabs; ++z) s += ws[(long)z * n + i];
        C[i] = s;
    }
}

template <typename T>
__global__ __launch_bounds__(PB_THREADS) void probe_intercept_k(const T* __restrict__ Y, long P, int row0,
                                                                const double* __restrict__ C,
                                                                const double* __restrict__ mean_x, int L,
                                                                double* __restrict__ icpt) {
    for (long p = (long)blockIdx.x * PB_THREADS + threadIdx.x; p < P; p += (long)gridDim.x * PB_THREADS) {
        double s = 0.0;
        for (int l = 0; l < L; ++l) s += mean_x[l] * C[(long)l * P + p];
        icpt[p] = (C[(long)L * P + p] - s) + (double)Tgt<T>::val(Y[(long)row0 * P + p]);
    }
}

// One workgroup: 64 targets; wave g takes the row quads g, g + 4, ... of the list, four rows at a time and in list order
// (a row's index and embedding are uniform across the wave: scalar loads), the W tile [L][64] sits in LDS, and the four
// waves' sums are added in wave order.  Y[rows] and W are
// read once.  sums [5][P]: sum e, sum e^2, sum |e|, sum d, sum d^2.
template <typename T>
__global__ __launch_bounds__(PB_THREADS) void probe_residual_k(const T* __restrict__ Y, long N, long P,
                                                               const int* __restrict__ rows, int n_rows, int row0,
                                                               const double* __restrict__ Xr, const double* __restrict__ C,
                                                               const double* __restrict__ icpt, int L,
                                                               double* __restrict__ sums) {
    extern __shared__ double pb_lds[];                      // W tile [L][64], then the waves' sums [5][4][64]
    const int tid = threadIdx.x, t = tid & 63, g = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long p0 = (long)blockIdx.x * PB_RT, p = p0 + t;
    const bool live = p < P;
    for (int i = tid; i < L * PB_RT; i += PB_THREADS) {
        const int l = i / PB_RT, c = i - l * PB_RT;
        pb_lds[i] = p0 + c < P ? C[(long)l * P + p0 + c] : 0.0;
    }
    __syncthreads();
    const double ic = live ? icpt[p] : 0.0;
    const double yref = live ? (double)Tgt<T>::val(Y[(long)row0 * P + p]) : 0.0;
    double se = 0.0, see = 0.0, sae = 0.0, sd = 0.0, sdd = 0.0;
    for (int rb = 4 * g; rb < n_rows; rb += 4 * (PB_THREADS / 64)) {
        const double* x[4];
        long ri[4];
        double dot[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = min(rb + j, n_rows - 1);          // past the end: a valid address, the row is skipped below
            ri[j] = rb + j < n_rows ? (long)rows[r] : -1;
            x[j] = Xr + (long)r * L;
            dot[j] = 0.0;
        }
        for (int l = 0; l < L; ++l) {                       // one LDS read of W serves the four rows
            const double w = pb_lds[l * PB_RT + t];
#pragma unroll
            for (int j = 0; j < 4; ++j) dot[j] = fma(x[j][l], w, dot[j]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (ri[j] < 0 || ri[j] >= N) continue;
            const double y = live ? (double)Tgt<T>::val(Y[ri[j] * P + p]) : 0.0;
            const double e = y - (ic + dot[j]), d = y - yref;
            se += e;
            see += e * e;
            sae += fabs(e);
            sd += d;
            sdd += d * d;
        }
    }
    __syncthreads();                                        // every wave is done with the W tile
    const double v[5] = {se, see, sae, sd, sdd};
#pragma unroll
    for (int j = 0; j < 5; ++j) pb_lds[(j * 4 + g) * PB_RT + t] = v[j];
    __syncthreads();
    if (g == 0 && live) {
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            double s = pb_lds[(j * 4) * PB_RT + t];
            for (int w = 1; w < 4; ++w) s += pb_lds[(j * 4 + w) * PB_RT + t];
            sums[(long)j * P + p] = s;
        }
    }
}

// r2_score / explained_variance_score per target (sklearn.metrics._regression, force_finite=True: a zero denominator
// scores 1 with a zero numerator and 0 otherwise) and the block's partial sums part[block][5] = (r2, evs, sum e^2,
// sum |e|, constant targets).
__global__ __launch_bounds__(PB_THREADS) void probe_scores_k(const double* __restrict__ sums, long P, double m,
                                                             double* __restrict__ r2, double* __restrict__ evs,
                                                             double* __restrict__ part) {
    __shared__ double red[PB_THREADS];
    const long p = (long)blockIdx.x * PB_THREADS + threadIdx.x;
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (p < P) {
        const double se = sums[p], see = sums[P + p], sae = sums[2 * P + p], sd = sums[3 * P + p], sdd = sums[4 * P + p];
        const double sstot = sdd - (sd * sd) / m;
        const double r = sstot != 0.0 ? 1.0 - see / sstot : (see != 0.0 ? 0.0 : 1.0);
        const double me = se / m;
        const double num = see / m - me * me, den = sstot / m;
        const double ev = den != 0.0 ? 1.0 - num / den : (num != 0.0 ? 0.0 : 1.0);
        r2[p] = r;
        evs[p] = ev;
        v[0] = r; v[1] = ev; v[2] = see; v[3] = sae; v[4] = sstot == 0.0 ? 1.0 : 0.0;
    }
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const double s = block_tree_sum<PB_THREADS>(v[j], red);
        if (threadIdx.x == 0) part[(long)blockIdx.x * 5 + j] = s;
    }
}

// metrics = (mean r2, mse, mae, mean evs), n_constant: one workgroup; thread t adds the blocks t, t + 256, ... in
// order, then the halving tree
__global__ __launch_bounds__(PB_THREADS) void probe_means_k(const double* __restrict__ part, int nparts, long P, double m,
                                                            double* __restrict__ metrics, int* __restrict__ n_constant) {
    __shared__ double red[PB_THREADS];
    double tot[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        double s = 0.0;
        for (int b = threadIdx.x; b < nparts; b += PB_THREADS) s += part[(long)b * 5 + j];
        tot[j] = block_tree_sum<PB_THREADS>(s, red);
    }
    if (threadIdx.x == 0) {
        metrics[0] = tot[0] / (double)P;
        metrics[1] = tot[2] / (m * (double)P);
        metrics[2] = tot[3] / (m * (double)P);
        metrics[3] = tot[1] / (double)P;
        n_constant[0] = (int)tot[4];
    }
}

static int grid_1d(long n) {
    const long b = (n + PB_THREADS - 1) / PB_THREADS;
    return (int)(b < 65536 ? b : 65536);
}

// K slabs of the product: none while the target tiles alone fill the device, else enough to reach ~1024 workgroups,
// at least 16 K blocks (256 rows) each
static void xty_slabs(int n_rows, int M, long P, int* slabs, int* blocks_per_slab) {
    const long nblocks = cdiv(n_rows, PB_KB);
    const long wgs = (long)cdiv(P, PB_TP) * cdiv(cdiv(M, 16), PB_MG);
    long s = 1024 / wgs;
    if (s > nblocks / 16) s = nblocks / 16;
    if (s < 1) s = 1;
    const long bps = (nblocks + s - 1) / s;
    *blocks_per_slab = (int)bps;
    *slabs = (int)((nblocks + bps - 1) / bps);
}

template <typename T> static bool rows_aligned(const void* Y, long P) {
    return P % Tgt<T>::PIECE == 0 && (uintptr_t)Y % 16 == 0;
}

}  // namespace rbvae

using namespace rbvae;

#define PROBE_CHECK_SHAPE(name)                                                                                       \
    RBVAE_CHECK_ARG(y_dtype == RBVAE_PROBE_U8 || y_dtype == RBVAE_PROBE_F32,                                          \
                    name ": y_dtype %d is neither RBVAE_PROBE_U8 nor RBVAE_PROBE_F32", y_dtype);                      \
    RBVAE_CHECK_ARG(N >= 1 && N <= 2147483647L, name ": N=%ld outside 1..2^31-1", N);                                 \
    RBVAE_CHECK_ARG(P >= 1, name ": P=%ld, need at least one target", P);                                             \
    RBVAE_CHECK_ARG(row0 >= 0 && row0 < N, name ": the shift row %d is outside the %ld rows", row0, N)

extern "C" int rbvae_probe_xty_slabs(int n_rows, int M, long P) {
    if (n_rows < 1 || M < 2 || M > 129 || P < 1) return 0;
    int s, bps;
    xty_slabs(n_rows, M, P, &s, &bps);
    return s;
}

extern "C" size_t rbvae_probe_xty_ws_bytes(int n_rows, int M, long P) {
    const int s = rbvae_probe_xty_slabs(n_rows, M, P);
    return s > 1 ? (size_t)s * (size_t)M * (size_t)P * sizeof(double) : 0;
}

extern "C" int rbvae_probe_xty(int y_dtype, const void* Y, long N, long P, const int* rows, int n_rows, int row0,
                               const double* B, int M, double* C, double* ws, void* stream) {
    RBVAE_CHECK_ARG(Y && rows && B && C, "probe_xty: null pointer");
    PROBE_CHECK_SHAPE("probe_xty");
    RBVAE_CHECK_ARG(M >= 2 && M <= 129, "probe_xty: M=%d outside 2..129 (L = M - 1 in 1..128)", M);
    RBVAE_CHECK_ARG(n_rows >= 1, "probe_xty: empty row list");
    int slabs, bps;
    xty_slabs(n_rows, M, P, &slabs, &bps);
    RBVAE_CHECK_ARG(slabs == 1 || ws, "probe_xty: %d K slabs need the workspace (rbvae_probe_xty_ws_bytes)", slabs);
    const long tiles = cdiv(P, PB_TP);
    RBVAE_CHECK_ARG(tiles <= 2147483647L, "probe_xty: P=%ld too large", P);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)tiles, cdiv(cdiv(M, 16), PB_MG), slabs);
    double* out = slabs > 1 ? ws : C;
    if (y_dtype == RBVAE_PROBE_U8)
        hipLaunchKernelGGL(probe_xty_k<unsigned char>, grid, dim3(PB_THREADS), 0, st, (const unsigned char*)Y, N, P, rows,
                           n_rows, row0, B, M, out, bps, (int)rows_aligned<unsigned char>(Y, P));
    else
        hipLaunchKernelGGL(probe_xty_k<float>, grid, dim3(PB_THREADS), 0, st, (const float*)Y, N, P, rows, n_rows, row0,
                           B, M, out, bps, (int)rows_aligned<float>(Y, P));
    RBVAE_CHECK_LAUNCH("probe_xty");
    if (slabs > 1) {
        const long n = (long)M * P;
        hipLaunchKernelGGL(probe_slab_sum_k, dim3(grid_1d(n)), dim3(PB_THREADS), 0, st, ws, C, n, slabs);
        RBVAE_CHECK_LAUNCH("probe_xty (slab sum)");
    }
    return RBVAE_OK;
}

extern "C" int rbvae_probe_intercept(int y_dtype, const void* Y, long N, long P, int row0, const double* C,
                                     const double* mean_x, int L, double* intercept, void* stream) {
    RBVAE_CHECK_ARG(Y && C && mean_x && intercept, "probe_intercept: null pointer");
    PROBE_CHECK_SHAPE("probe_intercept");
    RBVAE_CHECK_ARG(L >= 1 && L <= 128, "probe_intercept: L=%d outside 1..128", L);
    hipStream_t st = (hipStream_t)stream;
    if (y_dtype == RBVAE_PROBE_U8)
        hipLaunchKernelGGL(probe_intercept_k<unsigned char>, dim3(grid_1d(P)), dim3(PB_THREADS), 0, st,
                           (const unsigned char*)Y, P, row0, C, mean_x, L, intercept);
    else
        hipLaunchKernelGGL(probe_intercept_k<float>, dim3(grid_1d(P)), dim3(PB_THREADS), 0, st, (const float*)Y, P, row0,
                           C, mean_x, L, intercept);
    RBVAE_CHECK_LAUNCH("probe_intercept");
    return RBVAE_OK;
}

extern "C" int rbvae_probe_residual_sums(int y_dtype, const void* Y, long N, long P, const int* rows, int n_rows,
                                         int row0, const double* Xr, const double* C, const double* intercept, int L,
                                         double* sums, void* stream) {
    RBVAE_CHECK_ARG(Y && rows && Xr && C && intercept && sums, "probe_residual_sums: null pointer");
    PROBE_CHECK_SHAPE("probe_residual_sums");
    RBVAE_CHECK_ARG(L >= 1 && L <= 128, "probe_residual_sums: L=%d outside 1..128", L);
    RBVAE_CHECK_ARG(n_rows >= 1, "probe_residual_sums: empty row list");
    const long tiles = cdiv(P, PB_RT);
    RBVAE_CHECK_ARG(tiles <= 2147483647L, "probe_residual_sums: P=%ld too large", P);
    const size_t w_bytes = (size_t)L * PB_RT * sizeof(double), red_bytes = (size_t)5 * 4 * PB_RT * sizeof(double);
    const size_t lds = w_bytes > red_bytes ? w_bytes : red_bytes;       // <= 64 KB at L = 128
    hipStream_t st = (hipStream_t)stream;
    if (y_dtype == RBVAE_PROBE_U8)
        hipLaunchKernelGGL(probe_residual_k<unsigned char>, dim3((unsigned)tiles), dim3(PB_THREADS), lds, st,
                           (const unsigned char*)Y, N, P, rows, n_rows, row0, Xr, C, intercept, L, sums);
    else
        hipLaunchKernelGGL(probe_residual_k<float>, dim3((unsigned)tiles), dim3(PB_THREADS), lds, st, (const float*)Y, N,
                           P, rows, n_rows, row0, Xr, C, intercept, L, sums);
    RBVAE_CHECK_LAUNCH("probe_residual_sums");
    return RBVAE_OK;
}

extern "C" int rbvae_probe_finish_parts(long P) { return P >= 1 ? cdiv(P, PB_THREADS) : 0; }

extern "C" int rbvae_probe_finish(const double* sums, long P, int m, double* r2, double* evs, double* part,
                                  double* metrics, int* n_constant, void* stream) {
    RBVAE_CHECK_ARG(sums && r2 && evs && part && metrics && n_constant, "probe_finish: null pointer");
    RBVAE_CHECK_ARG(P >= 1, "probe_finish: P=%ld, need at least one target", P);
    RBVAE_CHECK_ARG(m >= 1, "probe_finish: m=%d, need at least one test row", m);
    const long nparts = cdiv(P, PB_THREADS);
    RBVAE_CHECK_ARG(nparts <= 2147483647L, "probe_finish: P=%ld too large", P);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(probe_scores_k, dim3((unsigned)nparts), dim3(PB_THREADS), 0, st, sums, P, (double)m, r2, evs, part);
    RBVAE_CHECK_LAUNCH("probe_finish (scores)");
    hipLaunchKernelGGL(probe_means_k, dim3(1), dim3(PB_THREADS), 0, st, part, (int)nparts, P, (double)m, metrics,
                       n_constant);
    RBVAE_CHECK_LAUNCH("probe_finish (means)");
    return RBVAE_OK;
}
