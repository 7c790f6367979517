// Bernoulli models of the hard codes: a state is a vector of bit probabilities theta_kl.  The emissions and the M-step of a
// Bernoulli mixture and of a hidden Markov model with Bernoulli emissions, on bit-packed codes (bernoulli.py drives the fits
// with rbvae_gmm_decide and rbvae_hmm_forward / _backward / _posterior / _viterbi, which take any emissions).  DESIGN.md
// section 7 has the formulation; include/rbvae_hip.h every order.
//   bern_pack_k     a wave per row: lane l reads codes[i][l] and codes[i][64 + l] (coalesced), two ballots of `> 0.5` are the
//                   row's four words, lane 0 stores them as 16 bytes
//   bern_emit_k     hmm_emit_k's shape: a lane per row, the row's four words in registers.  log theta and log(1 - theta) pass
//                   through LDS in chunks, interleaved [k][l][2] = {logf, logt}: the lane's bit selects one of two adjacent f64,
//                   one LDS read and one addition per (row, k, l); four components run side by side, each a chain in l
//   bern_estep_k    gmm_estep_k's shape and sweeps with the same sum and log w_k added last
//   bern_partial_k  stage one of the M-step, gmm_partial_k's blocks: a workgroup owns a block of rows and 256 cells (k, c) of
//                   [K][L + 1]; it stages 256 rows' words in LDS at a time and a thread walks them in ascending order, adding
//                   r_ki where bit c of the row is set (c = L: always)
//   bern_finish_k   stage two: a workgroup per component adds the partials in block order and writes theta, the two log tables,
//                   the weights and their logs
// state int32 [4] is the mixture's {done, n_iter, why, 0}: every kernel returns at once when done is set.  No floating-point
// atomics; two runs agree bit for bit.  Contraction is off.
#include "common.h"
#include "diag_gauss.h"

#include <math.h>

#pragma clang fp contract(off)

namespace rbvae {

constexpr int BN_THREADS = 256;
constexpr int BN_MAX_K = 256, BN_MAX_N = 1 << 20;
constexpr int BN_CHUNK = DG_CHUNK;      // f64 values of the interleaved log tables per LDS chunk (32 KB)
constexpr int BN_UNROLL = 4;            // components summed side by side
constexpr int BN_ROWS = 256;            // rows of packed words staged per pass of bern_partial_k
constexpr int BST_DONE = 0;

__global__ __launch_bounds__(BN_THREADS) void bern_pack_k(const float* __restrict__ codes, int N, int L,
                                                          uint4* __restrict__ bits) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * (BN_THREADS / 64) + (threadIdx.x >> 6);
    if (i >= N) return;                                     // the same in every lane of a wave
    const float* row = codes + (long)i * L;
    const float a = lane < L ? row[lane] : 0.f;
    const float b = 64 + lane < L ? row[64 + lane] : 0.f;
    const unsigned long long lo = __ballot(a > 0.5f), hi = __ballot(b > 0.5f);
    if (lane == 0) bits[i] = make_uint4((unsigned)lo, (unsigned)(lo >> 32), (unsigned)hi, (unsigned)(hi >> 32));
}

// ts f64 [n][L][2] = {logf_kl, logt_kl} of the components k0 .. k0 + n
__device__ __forceinline__ void bn_stage(double* ts, const double* __restrict__ logt, const double* __restrict__ logf,
                                         int L, int k0, int n, int tid) {
    const double* t = logt + (long)k0 * L;
    const double* f = logf + (long)k0 * L;
    for (int c = tid; c < n * L; c += BN_THREADS) reinterpret_cast<double2*>(ts)[c] = make_double2(f[c], t[c]);
}

// s_u = sum_l (bit_l ? logt : logf) of component u of t [U][L][2], l ascending from zero: selections and additions only
template <int U>
__device__ __forceinline__ void bn_row_sums(const uint4 w, const double* t, int L, double (&s)[U]) {
    const unsigned ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int u = 0; u < U; ++u) s[u] = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = min(32, L - 32 * j);
        unsigned b = ws[j];
        const double* p = t + 64 * j;
        for (int l = 0; l < n; ++l) {
            const int o = 2 * l + (int)(b & 1u);
#pragma unroll
            for (int u = 0; u < U; ++u) s[u] += p[u * 2 * L + o];
            b >>= 1;
        }
    }
}

__global__ __launch_bounds__(BN_THREADS) void bern_emit_k(const uint4* __restrict__ bits, int N, int L,
                                                          const double* __restrict__ logt,
                                                          const double* __restrict__ logf, int K, double* logb,
                                                          double* __restrict__ rowmax, double* __restrict__ e,
                                                          const int* __restrict__ state) {
    __shared__ __attribute__((aligned(16))) double ts[BN_CHUNK];
    if (state && state[BST_DONE]) return;
    const int tid = threadIdx.x;
    const int i = blockIdx.x * BN_THREADS + tid;
    const bool live = i < N;
    const int KC = BN_CHUNK / (2 * L);
    const uint4 w = live ? bits[i] : make_uint4(0u, 0u, 0u, 0u);
    double m = -INFINITY;
    for (int k0 = 0; k0 < K; k0 += KC) {
        const int n = min(KC, K - k0);
        __syncthreads();                                    // the previous chunk's reads are done
        bn_stage(ts, logt, logf, L, k0, n, tid);
        __syncthreads();
        int r = 0;
        for (; r + BN_UNROLL <= n; r += BN_UNROLL) {
            double s[BN_UNROLL];
            bn_row_sums<BN_UNROLL>(w, ts + r * 2 * L, L, s);
#pragma unroll
            for (int u = 0; u < BN_UNROLL; ++u) {
                if (live) logb[(long)(k0 + r + u) * N + i] = s[u];
                if (s[u] > m) m = s[u];
            }
        }
        for (; r < n; ++r) {
            double s[1];
            bn_row_sums<1>(w, ts + r * 2 * L, L, s);
            if (live) logb[(long)(k0 + r) * N + i] = s[0];
            if (s[0] > m) m = s[0];
        }
    }
    if (!live) return;
    rowmax[i] = m;
    for (int k = 0; k < K; ++k) e[(long)i * K + k] = exp(logb[(long)k * N + i] - m);
}

__global__ __launch_bounds__(BN_THREADS) void bern_estep_k(const uint4* __restrict__ bits, int N, int L,
                                                           const double* __restrict__ logt,
                                                           const double* __restrict__ logf,
                                                           const double* __restrict__ logw, int K, double* resp,
                                                           double* __restrict__ lognorm, int* __restrict__ label,
                                                           const int* __restrict__ state) {
    __shared__ __attribute__((aligned(16))) double ts[BN_CHUNK];
    __shared__ double lw[BN_MAX_K];
    if (state && state[BST_DONE]) return;
    const int tid = threadIdx.x;
    const int i = blockIdx.x * BN_THREADS + tid;
    const bool live = i < N;
    const int KC = BN_CHUNK / (2 * L);
    const uint4 w = live ? bits[i] : make_uint4(0u, 0u, 0u, 0u);
    if (tid < K) lw[tid] = logw[tid];                       // K <= 256: one value per thread, visible after the first barrier
    double m = -INFINITY, s = 0.0;
    int bk = 0;
    // with resp: one sweep that stores lp; without: a second sweep computes the same lp again for the sum
    const int sweeps = resp ? 1 : 2;
    for (int sweep = 0; sweep < sweeps; ++sweep) {
        for (int k0 = 0; k0 < K; k0 += KC) {
            const int n = min(KC, K - k0);
            __syncthreads();
            bn_stage(ts, logt, logf, L, k0, n, tid);
            __syncthreads();
            for (int r = 0; r < n; r += BN_UNROLL) {
                double q[BN_UNROLL];
                const int nu = min(BN_UNROLL, n - r);
                if (nu == BN_UNROLL) {
                    bn_row_sums<BN_UNROLL>(w, ts + r * 2 * L, L, q);
                } else {
                    for (int u = 0; u < nu; ++u) {
                        double q1[1];
                        bn_row_sums<1>(w, ts + (r + u) * 2 * L, L, q1);
                        q[u] = q1[0];
                    }
                }
                for (int u = 0; u < nu; ++u) {
                    const int k = k0 + r + u;
                    const double lp = q[u] + lw[k];
                    if (sweep == 0) {
                        if (resp && live) resp[(long)k * N + i] = lp;
                        if (lp > m) {                       // k ascends: a tie stays with the lower component
                            m = lp;
                            bk = k;
                        }
                    } else {
                        s += exp(lp - m);
                    }
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

// out f64 [blocks][K][L + 1]; grid (blocks, ceil(K (L + 1) / 256)): cell (k, l) the block's sum of r_ki over the rows whose
// bit l is set, cell (k, L) that of r_ki
__global__ __launch_bounds__(BN_THREADS) void bern_partial_k(const uint4* __restrict__ bits, int N, int L,
                                                             const double* __restrict__ resp, int K, int rows,
                                                             double* __restrict__ out, const int* __restrict__ state) {
    __shared__ __attribute__((aligned(16))) unsigned wsm[BN_ROWS * 4];
    if (state && state[BST_DONE]) return;
    const int tid = threadIdx.x, LS = L + 1;
    const int e = blockIdx.y * BN_THREADS + tid;
    const bool cell = e < K * LS;                           // a thread without a cell still stages rows
    const int k = cell ? e / LS : 0, c = cell ? e - k * LS : 0;
    const bool all = c == L;
    const int wi = all ? 0 : c >> 5, sh = c & 31;
    const int r0 = blockIdx.x * rows, r1 = min(N, r0 + rows);
    const double* rk = resp + (long)k * N;
    double acc = 0.0;
    for (int base = r0; base < r1; base += BN_ROWS) {
        const int nr = min(BN_ROWS, r1 - base);
        __syncthreads();                                    // the previous pass's reads are done
        if (tid < nr) reinterpret_cast<uint4*>(wsm)[tid] = bits[base + tid];
        __syncthreads();
        if (!cell) continue;
        if (all) {
            for (int r = 0; r < nr; ++r) acc += rk[base + r];
        } else {
            for (int r = 0; r < nr; ++r) {
                const double v = rk[base + r];
                if ((wsm[r * 4 + wi] >> sh) & 1u) acc += v;
            }
        }
    }
    if (cell) out[((long)blockIdx.x * K + k) * LS + c] = acc;
}

__global__ __launch_bounds__(BN_THREADS) void bern_finish_k(const double* __restrict__ ws, int blocks, int L, int K,
                                                            double prior, double* __restrict__ weights,
                                                            double* __restrict__ logw, double* __restrict__ theta,
                                                            double* __restrict__ logt, double* __restrict__ logf,
                                                            const int* __restrict__ state) {
    __shared__ double nks[BN_MAX_K];
    __shared__ double total;
    if (state && state[BST_DONE]) return;
    const int c = threadIdx.x, k = blockIdx.x, LS = L + 1;
    if (c < K) {                                            // every component's nk: the weights' denominator
        double a = 0.0;
        for (int blk = 0; blk < blocks; ++blk) a += ws[((long)blk * K + c) * LS + L];
        nks[c] = a;
    }
    __syncthreads();
    if (c == 0) {
        double t = 0.0;
        for (int j = 0; j < K; ++j) t += nks[j] + DG_NK_EPS;
        total = t;
    }
    if (c < L) {
        double s = 0.0;
        for (int blk = 0; blk < blocks; ++blk) s += ws[((long)blk * K + k) * LS + c];
        const double nk = nks[k];
        const double den = nk + 2.0 * prior;
        const double th = (s + prior) / den;
        theta[(long)k * L + c] = th;
        logt[(long)k * L + c] = log(th);
        logf[(long)k * L + c] = log(((nk - s) + prior) / den);
    }
    __syncthreads();
    if (c == 0) {
        const double w = (nks[k] + DG_NK_EPS) / total;
        weights[k] = w;
        logw[k] = log(w);
    }
}

static bool bn_ok(int N, int L, int K) {
    return L >= 1 && L <= DG_MAX_L && K >= 1 && K <= BN_MAX_K && N >= K && N <= BN_MAX_N && (long)N * K <= DG_MAX_NK;
}

}  // namespace rbvae

using namespace rbvae;

#define BN_CHECK_SHAPE(name)                                                                                          \
    do {                                                                                                              \
        if (!bn_ok(N, L, K))                                                                                          \
            return fail(RBVAE_E_UNSUPPORTED,                                                                          \
                        name ": (N=%d, L=%d, K=%d) outside 1 <= L <= %d, 1 <= K <= %d, K <= N <= %d, N K <= %ld", N, L, K, \
                        DG_MAX_L, BN_MAX_K, BN_MAX_N, DG_MAX_NK);                                                     \
    } while (0)

extern "C" int rbvae_bern_ok(int N, int L, int K) { return bn_ok(N, L, K) ? 1 : 0; }

extern "C" int rbvae_bern_chunk_components(int L) { return L >= 1 && L <= DG_MAX_L ? BN_CHUNK / (2 * L) : 0; }

extern "C" size_t rbvae_bern_ws_bytes(int N, int L, int K) {
    if (!bn_ok(N, L, K)) return 0;
    return sizeof(double) * (size_t)row_blocks(N) * K * (L + 1);
}

extern "C" int rbvae_bern_pack(const float* codes, int N, int L, uint32_t* bits, void* stream) {
    const int K = 1;
    BN_CHECK_SHAPE("bern_pack");
    RBVAE_CHECK_ARG(codes && bits, "bern_pack: null pointer");
    hipLaunchKernelGGL(bern_pack_k, dim3(cdiv(N, BN_THREADS / 64)), dim3(BN_THREADS), 0, (hipStream_t)stream, codes, N, L,
                       (uint4*)bits);
    RBVAE_CHECK_LAUNCH("bern_pack");
    return RBVAE_OK;
}

extern "C" int rbvae_bern_emit(const uint32_t* bits, int N, int L, const double* logt, const double* logf, int K,
                               double* logb, double* rowmax, double* e, const int* state, void* stream) {
    BN_CHECK_SHAPE("bern_emit");
    if (!rbvae_hmm_ok(N, L, K))
        return fail(RBVAE_E_UNSUPPORTED, "bern_emit: (N=%d, L=%d, K=%d) outside rbvae_hmm_ok", N, L, K);
    RBVAE_CHECK_ARG(bits && logt && logf && logb && rowmax && e, "bern_emit: null pointer");
    hipLaunchKernelGGL(bern_emit_k, dim3(cdiv(N, BN_THREADS)), dim3(BN_THREADS), 0, (hipStream_t)stream, (const uint4*)bits,
                       N, L, logt, logf, K, logb, rowmax, e, state);
    RBVAE_CHECK_LAUNCH("bern_emit");
    return RBVAE_OK;
}

extern "C" int rbvae_bern_estep(const uint32_t* bits, int N, int L, const double* logt, const double* logf,
                                const double* logw, int K, double* resp, double* lognorm, int* label, const int* state,
                                void* stream) {
    BN_CHECK_SHAPE("bern_estep");
    RBVAE_CHECK_ARG(bits && logt && logf && logw && lognorm, "bern_estep: null pointer");
    hipLaunchKernelGGL(bern_estep_k, dim3(cdiv(N, BN_THREADS)), dim3(BN_THREADS), 0, (hipStream_t)stream,
                       (const uint4*)bits, N, L, logt, logf, logw, K, resp, lognorm, label, state);
    RBVAE_CHECK_LAUNCH("bern_estep");
    return RBVAE_OK;
}

extern "C" int rbvae_bern_mstep(const uint32_t* bits, int N, int L, const double* resp, int K, double prior,
                                double* weights, double* logw, double* theta, double* logt, double* logf, double* ws,
                                const int* state, void* stream) {
    BN_CHECK_SHAPE("bern_mstep");
    RBVAE_CHECK_ARG(bits && resp && weights && logw && theta && logt && logf && ws, "bern_mstep: null pointer");
    RBVAE_CHECK_ARG(prior > 0.0, "bern_mstep: prior=%g", prior);
    const int blocks = row_blocks(N), rows = row_block_rows(N);
    const dim3 grid(blocks, cdiv((long)K * (L + 1), BN_THREADS));
    hipLaunchKernelGGL(bern_partial_k, grid, dim3(BN_THREADS), 0, (hipStream_t)stream, (const uint4*)bits, N, L, resp, K,
                       rows, ws, state);
    RBVAE_CHECK_LAUNCH("bern_mstep (sums)");
    hipLaunchKernelGGL(bern_finish_k, dim3(K), dim3(BN_THREADS), 0, (hipStream_t)stream, (const double*)ws, blocks, L, K,
                       prior, weights, logw, theta, logt, logf, state);
    RBVAE_CHECK_LAUNCH("bern_mstep (finish)");
    return RBVAE_OK;
}
