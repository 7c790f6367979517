// Density clustering of the latents: scikit-learn's DBSCAN in its order-free form, on a bit-packed radius graph (density.py
// drives it).  DESIGN.md section 7 has the characterisation; include/rbvae_hip.h every rule.
//   db_adj_k        a workgroup owns one word of the graph (64 columns, a lane each) and DB_ROWS query rows.  The columns sit in
//                   LDS as f32 [L][65] (a lane reads its own column: consecutive dwords, no conflict; the stride of 65 spreads
//                   the staging writes); the query rows pass through LDS as f64, DB_QR at a time, read at a wave-uniform address
//                   (a broadcast).  A lane carries DB_U query rows side by side, each a chain in l; the wave's ballot of
//                   `d2 <= eps2` is the word
//   db_adj_bits_k   the same ownership on packed codes: the lane's column is four words in registers, the query rows' words come
//                   from LDS, the distance is four xor / popcount
//   db_count_k      a wave per row adds the popcounts of its words
//   db_core_k       a wave per word: the ballot of cnt >= min_samples, and f = i or N
//   db_copy_k / db_hook_k / db_decide_k     one Jacobi round of FastSV: f_out = f_in; a wave per core row takes the minimum
//                   grandparent of its core neighbours and applies the three integer atomicMin; one workgroup compares the
//                   buffers and decides
//   db_roots_k      one workgroup: the root mask, the exclusive scan of its word popcounts, the number of clusters
//   db_label_k      a wave per row: cid of the row's root, or of the smallest root among a non-core row's core neighbours
// Distances are f64 through pairdist.h, never contracted; everything behind the comparison is integer.  No floating-point
// atomics; two runs agree bit for bit, the number of rounds included.
#include "common.h"
#include "pairdist.h"

#pragma clang fp contract(off)

namespace rbvae {

constexpr int DB_THREADS = 256, DB_WAVES = DB_THREADS / 64;
constexpr int DB_MAX_N = 65536, DB_MAX_L = 128, DB_MAX_W = DB_MAX_N / 64;
constexpr int DB_U = 4;                     // query rows a lane carries side by side
constexpr int DB_QR = DB_WAVES * DB_U;      // query rows staged per pass
constexpr int DB_ROWS = 256;                // query rows per workgroup
constexpr int DB_CS = 65;                   // dword stride of one coordinate of the 64 columns in LDS
constexpr int DB_SCAN = 1024;               // threads of the two one-workgroup kernels
constexpr int DST_DONE = 0, DST_ROUNDS = 1, DST_CHANGED = 2;

typedef unsigned long long u64;

static_assert(DB_ROWS % DB_QR == 0 && DB_MAX_W <= DB_SCAN, "the tiles divide; the scan has a thread per word");

__device__ __forceinline__ int wave_min_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}

// Dynamic LDS: cols f32 [L][DB_CS] | xq f64 [DB_QR][L]
__global__ __launch_bounds__(DB_THREADS) void db_adj_k(const float* __restrict__ X, int N, int L, double eps2,
                                                       u64* __restrict__ adj, int W) {
    extern __shared__ __attribute__((aligned(16))) unsigned char db_lds[];
    float* cols = reinterpret_cast<float*>(db_lds);
    double* xq = reinterpret_cast<double*>(db_lds + (((size_t)L * DB_CS * sizeof(float) + 15) & ~(size_t)15));
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int word = blockIdx.x, j0 = word * 64, j = j0 + lane;
    const int r0 = blockIdx.y * DB_ROWS, r1 = min(N, r0 + DB_ROWS);
    const int nc = min(64, N - j0);                         // the columns that exist; the others are zeros and never set a bit
    for (int e = tid; e < 64 * L; e += DB_THREADS) {        // the 64 rows are one contiguous piece of X
        const int c = e / L, l = e - c * L;
        cols[l * DB_CS + c] = c < nc ? X[(long)j0 * L + e] : 0.f;
    }
    for (int i0 = r0; i0 < r1; i0 += DB_QR) {
        __syncthreads();                                    // the previous pass's reads are done (first pass: cols is written)
        for (int e = tid; e < DB_QR * L; e += DB_THREADS) {
            const int q = e / L;
            xq[e] = i0 + q < N ? (double)X[(long)i0 * L + e] : 0.0;
        }
        __syncthreads();
        const double* q = xq + wave * DB_U * L;
        double s[DB_U];
#pragma unroll
        for (int u = 0; u < DB_U; ++u) s[u] = 0.0;
        for (int l = 0; l < L; ++l) {
            const double b = (double)cols[l * DB_CS + lane];
#pragma unroll
            for (int u = 0; u < DB_U; ++u) d2_step(s[u], q[u * L + l], b);
        }
#pragma unroll
        for (int u = 0; u < DB_U; ++u) {
            const int i = i0 + wave * DB_U + u;             // the same in every lane of a wave
            if (i < N) {
                const u64 m = __ballot(j < N && s[u] <= eps2);      // NaN compares false
                if (lane == 0) adj[(long)i * W + word] = m;
            }
        }
    }
}

__global__ __launch_bounds__(DB_THREADS) void db_adj_bits_k(const uint4* __restrict__ bits, int N, int max_bits,
                                                            u64* __restrict__ adj, int W) {
    __shared__ uint4 qs[DB_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int word = blockIdx.x, j = word * 64 + lane;
    const int r0 = blockIdx.y * DB_ROWS;
    const uint4 mine = j < N ? bits[j] : make_uint4(0u, 0u, 0u, 0u);
    qs[tid] = r0 + tid < N ? bits[r0 + tid] : make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
    for (int q = wave; q < DB_ROWS; q += DB_WAVES) {
        const int i = r0 + q;
        if (i >= N) break;                                  // the same in every lane of a wave
        const uint4 a = qs[q];
        const int d = __popc(a.x ^ mine.x) + __popc(a.y ^ mine.y) + __popc(a.z ^ mine.z) + __popc(a.w ^ mine.w);
        const u64 m = __ballot(j < N && d <= max_bits);
        if (lane == 0) adj[(long)i * W + word] = m;
    }
}

__global__ __launch_bounds__(DB_THREADS) void db_count_k(const u64* __restrict__ adj, int N, int W, int* __restrict__ cnt) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * DB_WAVES + (threadIdx.x >> 6);
    if (i >= N) return;
    int c = 0;
    for (int w = lane; w < W; w += 64) c += __popcll(adj[(long)i * W + w]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == 0) cnt[i] = c;
}

__global__ __launch_bounds__(DB_THREADS) void db_core_k(const int* __restrict__ cnt, int N, int W, int min_samples,
                                                        u64* __restrict__ core_mask, int* __restrict__ f) {
    const int lane = threadIdx.x & 63;
    const int word = blockIdx.x * DB_WAVES + (threadIdx.x >> 6);
    if (word >= W) return;
    const int i = word * 64 + lane;
    const bool core = i < N && cnt[i] >= min_samples;
    const u64 m = __ballot(core);
    if (lane == 0) core_mask[word] = m;
    if (i < N) f[i] = core ? i : N;
}

// f_in's entry as a parent: anything outside [0, N) is N, which is never followed
__device__ __forceinline__ int db_parent(const int* __restrict__ f, int N, int u) {
    const int p = f[u];
    return (unsigned)p < (unsigned)N ? p : N;
}

__global__ __launch_bounds__(DB_THREADS) void db_copy_k(const int* __restrict__ f_in, int N, int* __restrict__ f_out,
                                                        const int* __restrict__ state) {
    if (state[DST_DONE]) return;
    const int u = blockIdx.x * DB_THREADS + threadIdx.x;
    if (u < N) f_out[u] = f_in[u];
}

__global__ __launch_bounds__(DB_THREADS) void db_hook_k(const u64* __restrict__ adj, const u64* __restrict__ core_mask, int N,
                                                        int W, const int* __restrict__ f_in, int* f_out,
                                                        const int* __restrict__ state) {
    if (state[DST_DONE]) return;
    const int lane = threadIdx.x & 63;
    const int u = blockIdx.x * DB_WAVES + (threadIdx.x >> 6);
    if (u >= N) return;                                     // the same in every lane of a wave, as every test below
    if (!((core_mask[u >> 6] >> (u & 63)) & 1ull)) return;
    int mn = N;
    for (int w = lane; w < W; w += 64) {
        u64 m = adj[(long)u * W + w] & core_mask[w];
        if (w == (u >> 6)) m &= ~(1ull << (u & 63));
        while (m) {
            const int v = w * 64 + __builtin_ctzll(m);
            m &= m - 1;
            const int p = v < N ? db_parent(f_in, N, v) : N;   // a mask from db_core_k has no bit at or above N
            if (p < N) mn = min(mn, db_parent(f_in, N, p));
        }
    }
    mn = wave_min_int(mn);
    if (lane != 0) return;
    const int p = db_parent(f_in, N, u);
    if (mn < N) {
        if (p < N) atomicMin(&f_out[p], mn);                // hooking
        atomicMin(&f_out[u], mn);                           // aggressive
    }
    if (p < N) {
        const int gf = db_parent(f_in, N, p);
        if (gf < N) atomicMin(&f_out[u], gf);               // shortcut
    }
}

__global__ __launch_bounds__(DB_SCAN) void db_decide_k(const int* __restrict__ f_in, const int* __restrict__ f_out, int N,
                                                       int* state) {
    __shared__ int any;
    const bool done = state[DST_DONE] != 0;
    if (threadIdx.x == 0) any = 0;
    __syncthreads();                                        // every thread has read done before thread 0 may write it
    if (done) return;
    bool ch = false;
    for (int u = threadIdx.x; u < N; u += DB_SCAN) ch |= f_out[u] != f_in[u];
    if (ch) atomicOr(&any, 1);
    __syncthreads();
    if (threadIdx.x == 0) {
        state[DST_ROUNDS] += 1;
        state[DST_CHANGED] = any;
        if (!any) state[DST_DONE] = 1;
    }
}

// rootmask u64 [W], base int32 [W]: the roots of a word and the number of roots in the words before it
__global__ __launch_bounds__(DB_SCAN) void db_roots_k(const u64* __restrict__ core_mask, const int* __restrict__ f, int N,
                                                      int W, u64* __restrict__ rootmask, int* __restrict__ base,
                                                      int* __restrict__ n_clusters) {
    __shared__ int tot[DB_SCAN];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int w = wave; w < DB_SCAN; w += DB_SCAN / 64) {    // the same trip count in every wave: the ballots stay whole
        const int i = w * 64 + lane;
        const bool root = w < W && i < N && ((core_mask[w] >> lane) & 1ull) && f[i] == i;
        const u64 m = __ballot(root);
        if (lane == 0) {
            tot[w] = __popcll(m);
            if (w < W) rootmask[w] = m;
        }
    }
    __syncthreads();
    const int own = tot[tid];
    for (int o = 1; o < DB_SCAN; o <<= 1) {                 // Hillis-Steele, inclusive; integer sums
        const int add = tid >= o ? tot[tid - o] : 0;
        __syncthreads();
        tot[tid] += add;
        __syncthreads();
    }
    if (tid < W) base[tid] = tot[tid] - own;
    if (tid == DB_SCAN - 1) n_clusters[0] = tot[tid];
}

__device__ __forceinline__ int db_cid(const u64* __restrict__ rootmask, const int* __restrict__ base, int r) {
    return base[r >> 6] + __popcll(rootmask[r >> 6] & ((1ull << (r & 63)) - 1ull));
}

__global__ __launch_bounds__(DB_THREADS) void db_label_k(const u64* __restrict__ adj, const u64* __restrict__ core_mask,
                                                         const int* __restrict__ f, int N, int W,
                                                         const u64* __restrict__ rootmask, const int* __restrict__ base,
                                                         int* __restrict__ labels) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * DB_WAVES + (threadIdx.x >> 6);
    if (i >= N) return;                                     // the same in every lane of a wave
    int r = N;
    if ((core_mask[i >> 6] >> (i & 63)) & 1ull) {
        r = db_parent(f, N, i);
    } else {
        for (int w = lane; w < W; w += 64) {
            u64 m = adj[(long)i * W + w] & core_mask[w];
            while (m) {
                const int v = w * 64 + __builtin_ctzll(m);
                m &= m - 1;
                if (v < N) r = min(r, db_parent(f, N, v));
            }
        }
        r = wave_min_int(r);
    }
    if (lane == 0) labels[i] = r < N ? db_cid(rootmask, base, r) : -1;
}

static bool db_ok(int N, int L) { return N >= 2 && N <= DB_MAX_N && L >= 1 && L <= DB_MAX_L; }

static size_t db_adj_lds(int L) {
    return (((size_t)L * DB_CS * sizeof(float) + 15) & ~(size_t)15) + (size_t)DB_QR * L * sizeof(double);
}

static int db_count(const u64* adj, int N, int W, int* cnt, hipStream_t stream) {
    hipLaunchKernelGGL(db_count_k, dim3(cdiv(N, DB_WAVES)), dim3(DB_THREADS), 0, stream, adj, N, W, cnt);
    RBVAE_CHECK_LAUNCH("dbscan (row counts)");
    return RBVAE_OK;
}

}  // namespace rbvae

using namespace rbvae;

#define DB_CHECK_SHAPE(name)                                                                                          \
    do {                                                                                                              \
        if (!db_ok(N, L))                                                                                             \
            return fail(RBVAE_E_UNSUPPORTED, name ": (N=%d, L=%d) outside 2 <= N <= %d, 1 <= L <= %d", N, L, DB_MAX_N, \
                        DB_MAX_L);                                                                                    \
    } while (0)

extern "C" int rbvae_dbscan_ok(int N, int L) { return db_ok(N, L) ? 1 : 0; }

extern "C" int rbvae_dbscan_words(int N) { return N >= 1 && N <= DB_MAX_N ? cdiv(N, 64) : 0; }

extern "C" size_t rbvae_dbscan_ws_bytes(int N) { return db_ok(N, 1) ? (size_t)16 * cdiv(N, 64) : 0; }

extern "C" int rbvae_dbscan_adj(const float* X, int N, int L, double eps2, unsigned long long* adj, int* cnt, void* stream) {
    DB_CHECK_SHAPE("dbscan_adj");
    RBVAE_CHECK_ARG(X && adj && cnt, "dbscan_adj: null pointer");
    RBVAE_CHECK_ARG(eps2 >= 0.0, "dbscan_adj: eps2=%g is negative or NaN", eps2);
    const int W = cdiv(N, 64);
    hipLaunchKernelGGL(db_adj_k, dim3(W, cdiv(N, DB_ROWS)), dim3(DB_THREADS), db_adj_lds(L), (hipStream_t)stream, X, N, L, eps2,
                       adj, W);
    RBVAE_CHECK_LAUNCH("dbscan_adj");
    return db_count(adj, N, W, cnt, (hipStream_t)stream);
}

extern "C" int rbvae_dbscan_adj_bits(const uint32_t* bits, int N, int L, int max_bits, unsigned long long* adj, int* cnt,
                                     void* stream) {
    DB_CHECK_SHAPE("dbscan_adj_bits");
    RBVAE_CHECK_ARG(bits && adj && cnt, "dbscan_adj_bits: null pointer");
    RBVAE_CHECK_ARG(max_bits >= 0 && max_bits <= L, "dbscan_adj_bits: max_bits=%d outside 0..L=%d", max_bits, L);
    const int W = cdiv(N, 64);
    hipLaunchKernelGGL(db_adj_bits_k, dim3(W, cdiv(N, DB_ROWS)), dim3(DB_THREADS), 0, (hipStream_t)stream, (const uint4*)bits,
                       N, max_bits, adj, W);
    RBVAE_CHECK_LAUNCH("dbscan_adj_bits");
    return db_count(adj, N, W, cnt, (hipStream_t)stream);
}

extern "C" int rbvae_dbscan_core(const int* cnt, int N, int min_samples, unsigned long long* core_mask, int* f, void* stream) {
    const int L = 1;
    DB_CHECK_SHAPE("dbscan_core");
    RBVAE_CHECK_ARG(cnt && core_mask && f, "dbscan_core: null pointer");
    RBVAE_CHECK_ARG(min_samples >= 1, "dbscan_core: min_samples=%d", min_samples);
    const int W = cdiv(N, 64);
    hipLaunchKernelGGL(db_core_k, dim3(cdiv(W, DB_WAVES)), dim3(DB_THREADS), 0, (hipStream_t)stream, cnt, N, W, min_samples,
                       core_mask, f);
    RBVAE_CHECK_LAUNCH("dbscan_core");
    return RBVAE_OK;
}

extern "C" int rbvae_dbscan_round(const unsigned long long* adj, const unsigned long long* core_mask, int N, const int* f_in,
                                  int* f_out, int* state, void* stream) {
    const int L = 1;
    DB_CHECK_SHAPE("dbscan_round");
    RBVAE_CHECK_ARG(adj && core_mask && f_in && f_out && state, "dbscan_round: null pointer");
    RBVAE_CHECK_ARG(f_in != f_out, "dbscan_round: f_in and f_out are the same buffer");
    const int W = cdiv(N, 64);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(db_copy_k, dim3(cdiv(N, DB_THREADS)), dim3(DB_THREADS), 0, s, f_in, N, f_out, (const int*)state);
    RBVAE_CHECK_LAUNCH("dbscan_round (copy)");
    hipLaunchKernelGGL(db_hook_k, dim3(cdiv(N, DB_WAVES)), dim3(DB_THREADS), 0, s, adj, core_mask, N, W, f_in, f_out,
                       (const int*)state);
    RBVAE_CHECK_LAUNCH("dbscan_round (minima)");
    hipLaunchKernelGGL(db_decide_k, dim3(1), dim3(DB_SCAN), 0, s, f_in, (const int*)f_out, N, state);
    RBVAE_CHECK_LAUNCH("dbscan_round (decision)");
    return RBVAE_OK;
}

extern "C" int rbvae_dbscan_labels(const unsigned long long* adj, const unsigned long long* core_mask, const int* f, int N,
                                   int* labels, int* n_clusters, void* ws, void* stream) {
    const int L = 1;
    DB_CHECK_SHAPE("dbscan_labels");
    RBVAE_CHECK_ARG(adj && core_mask && f && labels && n_clusters && ws, "dbscan_labels: null pointer");
    RBVAE_CHECK_ARG(((uintptr_t)ws & 7) == 0, "dbscan_labels: ws is not 8-byte aligned");
    const int W = cdiv(N, 64);
    u64* rootmask = (u64*)ws;
    int* base = (int*)(rootmask + W);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(db_roots_k, dim3(1), dim3(DB_SCAN), 0, s, core_mask, f, N, W, rootmask, base, n_clusters);
    RBVAE_CHECK_LAUNCH("dbscan_labels (roots)");
    hipLaunchKernelGGL(db_label_k, dim3(cdiv(N, DB_WAVES)), dim3(DB_THREADS), 0, s, adj, core_mask, f, N, W,
                       (const u64*)rootmask, (const int*)base, labels);
    RBVAE_CHECK_LAUNCH("dbscan_labels");
    return RBVAE_OK;
}
