// Lowest eigenvectors of the symmetric-normalised Laplacian L = I - S, S = D^-1/2 W D^-1/2, of a symmetric CSR graph (the
// fuzzy graph of umap.hip): Lanczos with full reorthogonalisation against a basis that lives on the device.  spectral.py
// drives it and solves the tridiagonal problem on the host; DESIGN.md section 7 has the formulation.
//   sp_degree_k     a thread per row: deg = the row's weights added in ascending order, isd = 1 / sqrt(deg) (0 at deg = 0)
//   sp_matvec_k     umap_epoch_k's shape: a wave per row, the row's edges in chunks of 64, one per lane; a butterfly adds a
//                   chunk and the chunks are added in order
//   sp_dots_k       stage one of c = V^T w: a workgroup owns SP_ROWS = 1024 consecutive rows and 8 vectors; thread t adds
//                   its rows t, t + 256, t + 512, t + 768 in that order, a butterfly adds the wave's 64 lanes and the four
//                   waves' sums are added in wave order
//   sp_coef_k       stage two: a thread per vector adds the row blocks' partials in block order
//   sp_update_k     w_i -= sum_k c_k V_k[i], k ascending from zero, a thread per row
//   sp_beta_k       one thread: beta_j = sqrt(sum of the norm's partials), alpha_j and the state word
//   sp_scale_k      v_{j+1} = w / beta_j
//   sp_ritz_k       Y_c[i] = sum_j V[q + j][i] s[j][c], j ascending, a thread per row, up to 32 columns in registers
//   sp_resid_k, sp_norm_k   r = S y - theta y and its 2-norm through sp_matvec_k and sp_dots_k
// state int32 [2] = {broken, steps}: sp_beta_k alone writes it, every kernel of a step returns at once when broken is set, so
// the host may enqueue steps ahead of the read.  No floating-point atomics; two runs agree bit for bit.  Contraction is off.
#include "common.h"

#include <math.h>

#pragma clang fp contract(off)

namespace rbvae {

constexpr int SP_THREADS = 256;
constexpr int SP_ROWS = 1024;               // rows of one block of the dot products' first stage
constexpr int SP_VECS = 8;                  // vectors per workgroup there
constexpr int SP_UPD_THREADS = 64;
constexpr int SP_MAX_N = 1 << 20, SP_MAX_M = 1024, SP_MAX_Q = 8, SP_MAX_COLS = 32;
constexpr int ST_BROKEN = 0, ST_STEPS = 1;
constexpr double SP_BREAKDOWN = 0x1p-40;

__global__ __launch_bounds__(SP_THREADS) void sp_degree_k(const int* __restrict__ indptr, const int* __restrict__ indices,
                                                          const float* __restrict__ data, int N, double* __restrict__ deg,
                                                          double* __restrict__ isd) {
    const int i = blockIdx.x * SP_THREADS + threadIdx.x;
    if (i >= N) return;
    double d = 0.0;
    for (int e = indptr[i]; e < indptr[i + 1]; ++e)
        if ((unsigned)indices[e] < (unsigned)N) d += (double)data[e];
    deg[i] = d;
    isd[i] = d == 0.0 ? 0.0 : 1.0 / sqrt(d);
}

// y_i = isd_i * sum_e (double)w_e * (isd_j * x_j)
__global__ __launch_bounds__(SP_THREADS) void sp_matvec_k(const int* __restrict__ indptr, const int* __restrict__ indices,
                                                          const float* __restrict__ data, const double* __restrict__ isd,
                                                          int N, const double* __restrict__ x, double* __restrict__ y,
                                                          const int* __restrict__ state) {
    if (state && state[ST_BROKEN]) return;
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * (SP_THREADS / 64) + (threadIdx.x >> 6);
    if (i >= N) return;
    const int beg = indptr[i], end = indptr[i + 1];
    double acc = 0.0;
    for (int e0 = beg; e0 < end; e0 += 64) {                // wave-uniform bounds: the butterfly runs with every lane
        const int e = e0 + lane;
        double t = 0.0;
        if (e < end) {
            const int j = indices[e];
            if ((unsigned)j < (unsigned)N) t = (double)data[e] * (isd[j] * x[j]);
        }
        acc += wave_sum_f64(t);
    }
    if (lane == 0) y[i] = isd[i] * acc;
}

// part f64 [blocks][nv]: part[b][k] = the dot product of V_k and w over the rows of block b; grid (blocks, ceil(nv / 8))
__global__ __launch_bounds__(SP_THREADS) void sp_dots_k(const double* __restrict__ V, int nv, int N,
                                                        const double* __restrict__ w, double* __restrict__ part,
                                                        const int* __restrict__ state) {
    __shared__ double red[SP_VECS][SP_THREADS / 64];
    if (state && state[ST_BROKEN]) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r0 = blockIdx.x * SP_ROWS + tid, k0 = blockIdx.y * SP_VECS;
    double wv[SP_ROWS / SP_THREADS];
#pragma unroll
    for (int s = 0; s < SP_ROWS / SP_THREADS; ++s) {
        const int r = r0 + s * SP_THREADS;
        wv[s] = r < N ? w[r] : 0.0;
    }
    for (int kk = 0; kk < SP_VECS; ++kk) {
        const int k = k0 + kk;
        if (k >= nv) break;                                 // the same in every thread
        const double* v = V + (long)k * N;
        double acc = 0.0;
#pragma unroll
        for (int s = 0; s < SP_ROWS / SP_THREADS; ++s) {
            const int r = r0 + s * SP_THREADS;
            acc += (r < N ? v[r] : 0.0) * wv[s];
        }
        acc = wave_sum_f64(acc);
        if (lane == 0) red[kk][wave] = acc;
    }
    __syncthreads();
    if (tid < SP_VECS && k0 + tid < nv)
        part[(long)blockIdx.x * nv + k0 + tid] = ((red[tid][0] + red[tid][1]) + red[tid][2]) + red[tid][3];
}

// c[k] = sum_b part[b][k], b ascending.  diag >= 0: acc[0] = c[diag] (first) or acc[0] += c[diag]
__global__ __launch_bounds__(SP_THREADS) void sp_coef_k(const double* __restrict__ part, int blocks, int nv,
                                                        double* __restrict__ c, int diag, int first,
                                                        double* __restrict__ acc, const int* __restrict__ state) {
    if (state && state[ST_BROKEN]) return;
    const int k = blockIdx.x * SP_THREADS + threadIdx.x;
    if (k >= nv) return;
    double s = 0.0;
    for (int b = 0; b < blocks; ++b) s += part[(long)b * nv + k];
    c[k] = s;
    if (k == diag) acc[0] = first ? s : acc[0] + s;
}

__global__ __launch_bounds__(SP_UPD_THREADS) void sp_update_k(const double* __restrict__ V, int nv, int N,
                                                              const double* __restrict__ c, double* __restrict__ w,
                                                              const int* __restrict__ state) {
    if (state && state[ST_BROKEN]) return;
    const int i = blockIdx.x * SP_UPD_THREADS + threadIdx.x;
    if (i >= N) return;
    double s = 0.0;
    for (int k = 0; k < nv; ++k) s += c[k] * V[(long)k * N + i];
    w[i] = w[i] - s;
}

// part f64 [blocks]: the partials of w . w
__global__ void sp_beta_k(const double* __restrict__ part, int blocks, int j, const double* __restrict__ acc,
                          double* __restrict__ alpha, double* __restrict__ beta, int* __restrict__ state) {
    if (threadIdx.x != 0 || state[ST_BROKEN]) return;
    double s = 0.0;
    for (int b = 0; b < blocks; ++b) s += part[b];
    const double bt = sqrt(s);
    alpha[j] = acc[0];
    beta[j] = bt;
    state[ST_STEPS] = j + 1;
    if (!(bt > SP_BREAKDOWN)) state[ST_BROKEN] = 1;        // a NaN breaks the run down as well
}

__global__ __launch_bounds__(SP_THREADS) void sp_scale_k(double* __restrict__ w, int N, const double* __restrict__ beta,
                                                         const int* __restrict__ state) {
    if (state[ST_BROKEN]) return;                           // this step's breakdown included: w stays unnormalised
    const int i = blockIdx.x * SP_THREADS + threadIdx.x;
    if (i < N) w[i] = w[i] / beta[0];
}

// Y f64 [cols][N]; s f64 [m][cols]
__global__ __launch_bounds__(SP_UPD_THREADS) void sp_ritz_k(const double* __restrict__ V, int m, int N,
                                                            const double* __restrict__ s, int cols,
                                                            double* __restrict__ Y) {
    const int i = blockIdx.x * SP_UPD_THREADS + threadIdx.x;
    if (i >= N) return;
    double acc[SP_MAX_COLS];
#pragma unroll
    for (int c = 0; c < SP_MAX_COLS; ++c) acc[c] = 0.0;
    for (int j = 0; j < m; ++j) {
        const double v = V[(long)j * N + i];
        const double* sj = s + (long)j * cols;              // the same address in every lane
#pragma unroll
        for (int c = 0; c < SP_MAX_COLS; ++c)
            if (c < cols) acc[c] += v * sj[c];
    }
#pragma unroll
    for (int c = 0; c < SP_MAX_COLS; ++c)
        if (c < cols) Y[(long)c * N + i] = acc[c];
}

__global__ __launch_bounds__(SP_THREADS) void sp_resid_k(double* __restrict__ r, const double* __restrict__ y, int N,
                                                         const double* __restrict__ theta) {
    const int i = blockIdx.x * SP_THREADS + threadIdx.x;
    if (i < N) r[i] = r[i] - theta[0] * y[i];
}

__global__ void sp_norm_k(const double* __restrict__ part, int blocks, double* __restrict__ out) {
    if (threadIdx.x != 0) return;
    double s = 0.0;
    for (int b = 0; b < blocks; ++b) s += part[b];
    out[0] = sqrt(s);
}

static bool sp_ok(int N, int m_max, int q) {
    return N >= 2 && N <= SP_MAX_N && m_max >= 1 && m_max <= SP_MAX_M && q >= 0 && q <= SP_MAX_Q;
}
static int sp_blocks(int N) { return cdiv(N, SP_ROWS); }
// ws f64: partials [blocks][q + m_max + 1] | c [q + m_max + 1] | acc [2] | r [N]
static size_t sp_ws_doubles(int N, int m_max, int q) {
    const size_t nv = (size_t)q + m_max + 1;
    return (size_t)sp_blocks(N) * nv + nv + 2 + (size_t)N;
}

struct SpWs {
    double *part, *c, *acc, *r;
};
static SpWs sp_carve(void* ws, int N, int m_max, int q) {
    const size_t nv = (size_t)q + m_max + 1;
    SpWs s;
    s.part = (double*)ws;
    s.c = s.part + (size_t)sp_blocks(N) * nv;
    s.acc = s.c + nv;
    s.r = s.acc + 2;
    return s;
}

static int sp_launch_dots(const double* V, int nv, int N, const double* w, const SpWs& s, double* c, int diag, int first,
                          const int* state, hipStream_t st) {
    const int blocks = sp_blocks(N);
    hipLaunchKernelGGL(sp_dots_k, dim3(blocks, cdiv(nv, SP_VECS)), dim3(SP_THREADS), 0, st, V, nv, N, w, s.part, state);
    RBVAE_CHECK_LAUNCH("spectral (dot products)");
    if (c) {
        hipLaunchKernelGGL(sp_coef_k, dim3(cdiv(nv, SP_THREADS)), dim3(SP_THREADS), 0, st, (const double*)s.part, blocks, nv, c,
                           diag, first, s.acc, state);
        RBVAE_CHECK_LAUNCH("spectral (coefficients)");
    }
    return RBVAE_OK;
}

}  // namespace rbvae

using namespace rbvae;

#define SP_CHECK_SHAPE(name)                                                                                          \
    do {                                                                                                              \
        if (!sp_ok(N, m_max, q))                                                                                      \
            return fail(RBVAE_E_UNSUPPORTED, name ": (N=%d, m_max=%d, q=%d) outside 2 <= N <= %d, 1 <= m_max <= %d, " \
                        "0 <= q <= %d", N, m_max, q, SP_MAX_N, SP_MAX_M, SP_MAX_Q);                                   \
    } while (0)

#define SP_CHECK_WS(name)                                                                                             \
    do {                                                                                                              \
        RBVAE_CHECK_ARG(ws, name ": null pointer");                                                                   \
        RBVAE_CHECK_ARG(ws_bytes >= sizeof(double) * sp_ws_doubles(N, m_max, q), name ": workspace of %zu bytes, "    \
                        "rbvae_spectral_ws_bytes asks for %zu", ws_bytes, sizeof(double) * sp_ws_doubles(N, m_max, q)); \
    } while (0)

extern "C" int rbvae_spectral_ok(int N, int m_max, int q) { return sp_ok(N, m_max, q) ? 1 : 0; }

extern "C" int rbvae_spectral_block_rows(void) { return SP_ROWS; }

extern "C" size_t rbvae_spectral_ws_bytes(int N, int m_max, int q) {
    return sp_ok(N, m_max, q) ? sizeof(double) * sp_ws_doubles(N, m_max, q) : 0;
}

extern "C" int rbvae_spectral_degree(const int* indptr, const int* indices, const float* data, int N, double* deg,
                                     double* isd, void* stream) {
    const int m_max = 1, q = 0;
    SP_CHECK_SHAPE("spectral_degree");
    RBVAE_CHECK_ARG(indptr && indices && data && deg && isd, "spectral_degree: null pointer");
    hipLaunchKernelGGL(sp_degree_k, dim3(cdiv(N, SP_THREADS)), dim3(SP_THREADS), 0, (hipStream_t)stream, indptr, indices,
                       data, N, deg, isd);
    RBVAE_CHECK_LAUNCH("spectral_degree");
    return RBVAE_OK;
}

extern "C" int rbvae_spectral_matvec(const int* indptr, const int* indices, const float* data, const double* isd, int N,
                                     const double* x, double* y, void* stream) {
    const int m_max = 1, q = 0;
    SP_CHECK_SHAPE("spectral_matvec");
    RBVAE_CHECK_ARG(indptr && indices && data && isd && x && y, "spectral_matvec: null pointer");
    RBVAE_CHECK_ARG(x != y, "spectral_matvec: y must not be x");
    hipLaunchKernelGGL(sp_matvec_k, dim3(cdiv(N, SP_THREADS / 64)), dim3(SP_THREADS), 0, (hipStream_t)stream, indptr,
                       indices, data, isd, N, x, y, (const int*)nullptr);
    RBVAE_CHECK_LAUNCH("spectral_matvec");
    return RBVAE_OK;
}

extern "C" int rbvae_spectral_dots(const double* V, int nv, int N, const double* w, double* c, void* ws, size_t ws_bytes,
                                   void* stream) {
    const int q = 0, m_max = nv - 1 < 1 ? 1 : nv - 1;
    RBVAE_CHECK_ARG(nv >= 1, "spectral_dots: nv=%d, need at least one vector", nv);
    if (nv > SP_MAX_M + 1) return fail(RBVAE_E_UNSUPPORTED, "spectral_dots: nv=%d above %d", nv, SP_MAX_M + 1);
    SP_CHECK_SHAPE("spectral_dots");
    RBVAE_CHECK_ARG(V && w && c, "spectral_dots: null pointer");
    SP_CHECK_WS("spectral_dots");
    return sp_launch_dots(V, nv, N, w, sp_carve(ws, N, m_max, q), c, -1, 0, nullptr, (hipStream_t)stream);
}

extern "C" int rbvae_spectral_update(const double* V, int nv, int N, const double* c, double* w, void* stream) {
    const int q = 0, m_max = 1;
    RBVAE_CHECK_ARG(nv >= 1, "spectral_update: nv=%d, need at least one vector", nv);
    if (nv > SP_MAX_M + 1) return fail(RBVAE_E_UNSUPPORTED, "spectral_update: nv=%d above %d", nv, SP_MAX_M + 1);
    SP_CHECK_SHAPE("spectral_update");
    RBVAE_CHECK_ARG(V && c && w, "spectral_update: null pointer");
    hipLaunchKernelGGL(sp_update_k, dim3(cdiv(N, SP_UPD_THREADS)), dim3(SP_UPD_THREADS), 0, (hipStream_t)stream, V, nv, N, c,
                       w, (const int*)nullptr);
    RBVAE_CHECK_LAUNCH("spectral_update");
    return RBVAE_OK;
}

extern "C" int rbvae_spectral_step(const int* indptr, const int* indices, const float* data, const double* isd, int N,
                                   double* V, int q, int j, int m_max, double* alpha, double* beta, int* state, void* ws,
                                   size_t ws_bytes, void* stream) {
    SP_CHECK_SHAPE("spectral_step");
    RBVAE_CHECK_ARG(indptr && indices && data && isd && V && alpha && beta && state, "spectral_step: null pointer");
    RBVAE_CHECK_ARG(j >= 0 && j < m_max, "spectral_step: j=%d outside 0..m_max - 1 = %d", j, m_max - 1);
    SP_CHECK_WS("spectral_step");
    hipStream_t st = (hipStream_t)stream;
    const SpWs s = sp_carve(ws, N, m_max, q);
    const int nv = q + j + 1;
    const double* vj = V + (long)(q + j) * N;
    double* w = V + (long)(q + j + 1) * N;
    hipLaunchKernelGGL(sp_matvec_k, dim3(cdiv(N, SP_THREADS / 64)), dim3(SP_THREADS), 0, st, indptr, indices, data, isd, N,
                       vj, w, (const int*)state);
    RBVAE_CHECK_LAUNCH("spectral_step (product)");
    for (int pass = 0; pass < 2; ++pass) {
        if (int rc = sp_launch_dots(V, nv, N, w, s, s.c, q + j, pass == 0, state, st)) return rc;
        hipLaunchKernelGGL(sp_update_k, dim3(cdiv(N, SP_UPD_THREADS)), dim3(SP_UPD_THREADS), 0, st, (const double*)V, nv, N,
                           (const double*)s.c, w, (const int*)state);
        RBVAE_CHECK_LAUNCH("spectral_step (update)");
    }
    if (int rc = sp_launch_dots(w, 1, N, w, s, nullptr, -1, 0, state, st)) return rc;
    hipLaunchKernelGGL(sp_beta_k, dim3(1), dim3(64), 0, st, (const double*)s.part, sp_blocks(N), j, (const double*)s.acc,
                       alpha, beta, state);
    RBVAE_CHECK_LAUNCH("spectral_step (beta)");
    hipLaunchKernelGGL(sp_scale_k, dim3(cdiv(N, SP_THREADS)), dim3(SP_THREADS), 0, st, w, N, (const double*)(beta + j),
                       (const int*)state);
    RBVAE_CHECK_LAUNCH("spectral_step (scale)");
    return RBVAE_OK;
}

extern "C" int rbvae_spectral_ritz(const double* V, int q, int m, int N, const double* s, int cols, double* Y,
                                   void* stream) {
    const int m_max = m;
    if (cols < 1 || cols > SP_MAX_COLS)
        return fail(RBVAE_E_UNSUPPORTED, "spectral_ritz: cols=%d outside 1..%d", cols, SP_MAX_COLS);
    SP_CHECK_SHAPE("spectral_ritz");
    RBVAE_CHECK_ARG(V && s && Y, "spectral_ritz: null pointer");
    hipLaunchKernelGGL(sp_ritz_k, dim3(cdiv(N, SP_UPD_THREADS)), dim3(SP_UPD_THREADS), 0, (hipStream_t)stream,
                       V + (long)q * N, m, N, s, cols, Y);
    RBVAE_CHECK_LAUNCH("spectral_ritz");
    return RBVAE_OK;
}

extern "C" int rbvae_spectral_residuals(const int* indptr, const int* indices, const float* data, const double* isd, int N,
                                        const double* Y, int cols, const double* theta, double* res, void* ws,
                                        size_t ws_bytes, void* stream) {
    const int m_max = 1, q = 0;
    if (cols < 1 || cols > SP_MAX_COLS)
        return fail(RBVAE_E_UNSUPPORTED, "spectral_residuals: cols=%d outside 1..%d", cols, SP_MAX_COLS);
    SP_CHECK_SHAPE("spectral_residuals");
    RBVAE_CHECK_ARG(indptr && indices && data && isd && Y && theta && res, "spectral_residuals: null pointer");
    SP_CHECK_WS("spectral_residuals");
    hipStream_t st = (hipStream_t)stream;
    const SpWs s = sp_carve(ws, N, m_max, q);
    for (int c = 0; c < cols; ++c) {
        const double* y = Y + (long)c * N;
        hipLaunchKernelGGL(sp_matvec_k, dim3(cdiv(N, SP_THREADS / 64)), dim3(SP_THREADS), 0, st, indptr, indices, data, isd,
                           N, y, s.r, (const int*)nullptr);
        RBVAE_CHECK_LAUNCH("spectral_residuals (product)");
        hipLaunchKernelGGL(sp_resid_k, dim3(cdiv(N, SP_THREADS)), dim3(SP_THREADS), 0, st, s.r, y, N, theta + c);
        RBVAE_CHECK_LAUNCH("spectral_residuals (difference)");
        if (int rc = sp_launch_dots(s.r, 1, N, s.r, s, nullptr, -1, 0, nullptr, st)) return rc;
        hipLaunchKernelGGL(sp_norm_k, dim3(1), dim3(64), 0, st, (const double*)s.part, sp_blocks(N), res + c);
        RBVAE_CHECK_LAUNCH("spectral_residuals (norm)");
    }
    return RBVAE_OK;
}
