// HDBSCAN* of the latents (Campello, Moulavi, Zimek, Sander 2015) in an order-free form: the minimum spanning tree of the
// mutual reachability graph by Boruvka rounds on the device, and the condensed tree, the selection, the labels and the
// membership strengths on the host (density.py drives both).  DESIGN.md section 7 has the characterisation; include/rbvae_hip.h
// every rule.
//   mst_start_k     comp[i] = i, the per-component minima cleared, state = {0, 0, N, 0}
//   mst_search_k    the hot kernel: a workgroup owns MS_ROWS query rows and a slice of the columns.  The query rows sit in LDS
//                   as f64 and are read at a wave-uniform address (a broadcast); the columns pass through LDS in tiles of 64
//                   as f32 [L][65] (a lane reads its own column: consecutive dwords, no conflict), with their core distances
//                   and components beside them.  A lane carries MS_U query rows side by side as independent chains in l, and
//                   keeps the least w2 of its own columns for each of its MS_RW x MS_U rows in registers: its columns ascend,
//                   so `<` keeps the lowest j.  One butterfly per row at the end gives the slice's least (w2, j)
//   mst_rowmin_k    a thread per row: the least (w2, j) over the slices, in slice order; atomicMin of the w2 bits (a
//                   non-negative f64 orders as a u64) into the row's component
//   mst_key_k       a thread per row: among the rows that hold their component's least w2, atomicMin of (lo << 32 | hi)
//   mst_hook_k      a thread per component: hook onto the component at the other end of the chosen edge; of two components
//                   that chose the same edge the smaller id stays a root and the one that holds lo emits it; every other
//                   component emits its own
//   mst_merge_k     one workgroup: pointer jumping in LDS to the roots, the smallest row of every tree, the new comp, the
//                   count of components and the decision
// Distances are f64 through pairdist.h, never contracted; every atomic is an integer minimum or a counter whose value does not
// depend on the order of arrival.  The emitted list is in the order the counter handed out and must be sorted by (w2, lo, hi),
// which is a strict total order: after the sort two runs agree bit for bit, the number of rounds included.
// rbvae_hdbscan_tree / rbvae_hdbscan_cut are host code and make no GPU call.
#include "common.h"
#include "pairdist.h"

#include <math.h>

#include <algorithm>
#include <limits>
#include <vector>

#pragma clang fp contract(off)

namespace rbvae {

constexpr int MS_THREADS = 256, MS_WAVES = MS_THREADS / 64;
constexpr int MS_MAX_N = 16384, MS_MAX_L = 128;
constexpr int MS_U = 4;                             // query rows a lane carries side by side
constexpr int MS_RW = 2;                            // groups of MS_U rows a wave owns
constexpr int MS_ROWS = MS_WAVES * MS_RW * MS_U;    // query rows per workgroup
constexpr int MS_CS = 65;                           // dword stride of one coordinate of the 64 columns in LDS
constexpr int MS_MAX_S = 8;                         // column slices
constexpr int MS_MERGE = 1024;                      // threads of the one-workgroup kernel
constexpr int MS_JUMPS = 15;                        // 2^15 > MS_MAX_N + 1: the deepest chain is flat after that many doublings
constexpr int MST_DONE = 0, MST_ROUNDS = 1, MST_COMPS = 2, MST_EDGES = 3;

typedef unsigned long long u64;
constexpr u64 MS_NONE = ~0ull;

static_assert((1 << MS_JUMPS) > MS_MAX_N + 1, "pointer jumping reaches every root");

struct MstWs {                                      // the workspace's pieces, every one N (or MS_MAX_S N) long
    u64 *compw, *compkey, *candw, *part_w;
    int *candj, *parent, *part_j;
};

static size_t mst_ws_bytes(int N) { return (size_t)N * ((3 + MS_MAX_S) * sizeof(u64) + (2 + MS_MAX_S) * sizeof(int)); }

static MstWs mst_ws(void* ws, int N) {
    MstWs w;
    w.compw = (u64*)ws;
    w.compkey = w.compw + N;
    w.candw = w.compkey + N;
    w.part_w = w.candw + N;
    w.candj = (int*)(w.part_w + (size_t)MS_MAX_S * N);
    w.parent = w.candj + N;
    w.part_j = w.parent + N;
    return w;
}

__global__ __launch_bounds__(MS_THREADS) void mst_start_k(int N, int* __restrict__ comp, u64* __restrict__ compw,
                                                          u64* __restrict__ compkey, int* __restrict__ state) {
    const int i = blockIdx.x * MS_THREADS + threadIdx.x;
    if (i < N) {
        comp[i] = i;
        compw[i] = MS_NONE;
        compkey[i] = MS_NONE;
    }
    if (i < 4) state[i] = i == MST_COMPS ? N : 0;
}

// Dynamic LDS: cols f32 [L][MS_CS] | xq f64 [MS_ROWS][L] | ccore f64 [64] | ccomp int32 [64]
__global__ __launch_bounds__(MS_THREADS) void mst_search_k(const float* __restrict__ X, const double* __restrict__ core2,
                                                           const int* __restrict__ comp, int N, int L, int slice_cols,
                                                           u64* __restrict__ part_w, int* __restrict__ part_j,
                                                           const int* __restrict__ state) {
    if (state[MST_DONE]) return;
    extern __shared__ __attribute__((aligned(16))) unsigned char ms_lds[];
    float* cols = reinterpret_cast<float*>(ms_lds);
    double* xq = reinterpret_cast<double*>(ms_lds + (((size_t)L * MS_CS * sizeof(float) + 15) & ~(size_t)15));
    double* ccore = xq + (size_t)MS_ROWS * L;
    int* ccomp = reinterpret_cast<int*>(ccore + 64);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r0 = blockIdx.x * MS_ROWS;
    const int c0 = blockIdx.y * slice_cols, c1 = min(N, c0 + slice_cols);      // slice_cols is a multiple of 64
    for (int e = tid; e < MS_ROWS * L; e += MS_THREADS) {
        const int q = e / L;
        xq[e] = r0 + q < N ? (double)X[(long)r0 * L + e] : 0.0;
    }
    double qcore[MS_RW][MS_U], bw[MS_RW][MS_U];
    int qcomp[MS_RW][MS_U], bj[MS_RW][MS_U];
#pragma unroll
    for (int rw = 0; rw < MS_RW; ++rw)
#pragma unroll
        for (int u = 0; u < MS_U; ++u) {
            const int i = r0 + (wave * MS_RW + rw) * MS_U + u;      // the same in every lane of a wave
            qcore[rw][u] = i < N ? core2[i] : 0.0;
            qcomp[rw][u] = i < N ? comp[i] : -2;
            bw[rw][u] = __longlong_as_double(0x7ff0000000000000ll);
            bj[rw][u] = 0x7fffffff;
        }
    for (int j0 = c0; j0 < c1; j0 += 64) {
        __syncthreads();                                    // the previous tile's reads are done (first tile: xq is written)
        const int nc = min(64, N - j0);                     // the columns that exist; the others are never chosen
        for (int e = tid; e < 64 * L; e += MS_THREADS) {    // the 64 rows are one contiguous piece of X
            const int c = e / L, l = e - c * L;
            cols[l * MS_CS + c] = c < nc ? X[(long)j0 * L + e] : 0.f;
        }
        if (tid < 64) {
            ccore[tid] = tid < nc ? core2[j0 + tid] : 0.0;
            ccomp[tid] = tid < nc ? comp[j0 + tid] : -1;
        }
        __syncthreads();
        const int j = j0 + lane;
        const double cj = ccore[lane];
        const int cc = ccomp[lane];
#pragma unroll
        for (int rw = 0; rw < MS_RW; ++rw) {
            const double* q = xq + (size_t)(wave * MS_RW + rw) * MS_U * L;
            double s[MS_U];
#pragma unroll
            for (int u = 0; u < MS_U; ++u) s[u] = 0.0;
            for (int l = 0; l < L; ++l) {
                const double b = (double)cols[l * MS_CS + lane];
#pragma unroll
                for (int u = 0; u < MS_U; ++u) d2_step(s[u], q[u * L + l], b);
            }
#pragma unroll
            for (int u = 0; u < MS_U; ++u) {
                double w = s[u] > qcore[rw][u] ? s[u] : qcore[rw][u];
                w = w > cj ? w : cj;
                if (j < N && cc != qcomp[rw][u] && w < bw[rw][u]) {    // this lane's columns ascend: `<` keeps the lowest j
                    bw[rw][u] = w;
                    bj[rw][u] = j;
                }
            }
        }
    }
#pragma unroll
    for (int rw = 0; rw < MS_RW; ++rw)
#pragma unroll
        for (int u = 0; u < MS_U; ++u) {
            double w = bw[rw][u];
            int j = bj[rw][u];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double ow = __shfl_xor(w, o, 64);
                const int oj = __shfl_xor(j, o, 64);
                if (key_less(ow, oj, w, j)) {
                    w = ow;
                    j = oj;
                }
            }
            const int i = r0 + (wave * MS_RW + rw) * MS_U + u;
            if (lane == 0 && i < N) {
                part_w[(size_t)blockIdx.y * N + i] = (u64)__double_as_longlong(w);
                part_j[(size_t)blockIdx.y * N + i] = j;
            }
        }
}

__global__ __launch_bounds__(MS_THREADS) void mst_rowmin_k(const u64* __restrict__ part_w, const int* __restrict__ part_j,
                                                           int N, int S, const int* __restrict__ comp,
                                                           u64* __restrict__ candw, int* __restrict__ candj, u64* compw,
                                                           const int* __restrict__ state) {
    if (state[MST_DONE]) return;
    const int i = blockIdx.x * MS_THREADS + threadIdx.x;
    if (i >= N) return;
    u64 w = part_w[i];
    int j = part_j[i];
    for (int s = 1; s < S; ++s) {                           // the slices' columns ascend with s: `<` keeps the lowest j
        const u64 ws = part_w[(size_t)s * N + i];
        if (ws < w) {
            w = ws;
            j = part_j[(size_t)s * N + i];
        }
    }
    candw[i] = w;
    candj[i] = j;
    const int c = comp[i];
    if ((unsigned)j < (unsigned)N && (unsigned)c < (unsigned)N) atomicMin(&compw[c], w);
}

__global__ __launch_bounds__(MS_THREADS) void mst_key_k(const u64* __restrict__ candw, const int* __restrict__ candj, int N,
                                                        const int* __restrict__ comp, const u64* __restrict__ compw,
                                                        u64* compkey, const int* __restrict__ state) {
    if (state[MST_DONE]) return;
    const int i = blockIdx.x * MS_THREADS + threadIdx.x;
    if (i >= N) return;
    const int j = candj[i], c = comp[i];
    if ((unsigned)j >= (unsigned)N || (unsigned)c >= (unsigned)N || candw[i] != compw[c]) return;
    const u64 lo = (u64)min(i, j), hi = (u64)max(i, j);
    atomicMin(&compkey[c], lo << 32 | hi);
}

// Component c hooks onto t(c), the component at the other end of its least edge.  t(c) could have chosen that edge too, so
// key(t(c)) <= key(c): the keys do not increase along c -> t(c) -> ..., and around a cycle they are all equal.  The order is
// strict, so a cycle's components all chose ONE edge, which has two ends: the only cycles are pairs, broken towards the
// smaller id.
__global__ __launch_bounds__(MS_THREADS) void mst_hook_k(int N, const int* __restrict__ comp, const u64* __restrict__ compw,
                                                         const u64* __restrict__ compkey, int* __restrict__ parent,
                                                         int* __restrict__ edges, double* __restrict__ w2, int* state) {
    if (state[MST_DONE]) return;
    const int c = blockIdx.x * MS_THREADS + threadIdx.x;
    if (c >= N) return;
    const int r = comp[c];
    if (r != c) {
        parent[c] = (unsigned)r < (unsigned)N ? r : c;
        return;
    }
    const u64 key = compkey[c];
    const int lo = (int)(key >> 32), hi = (int)(key & 0xffffffffull);
    if (key == MS_NONE || (unsigned)lo >= (unsigned)N || (unsigned)hi >= (unsigned)N) {     // no row outside c
        parent[c] = c;
        return;
    }
    const bool mine_lo = comp[lo] == c;
    const int t = comp[mine_lo ? hi : lo];
    if ((unsigned)t >= (unsigned)N) {
        parent[c] = c;
        return;
    }
    const bool both = compkey[t] == key;                    // t chose this very edge
    parent[c] = both && c < t ? c : t;
    if (both && !mine_lo) return;                           // the side that holds lo emits it
    const int slot = atomicAdd(&state[MST_EDGES], 1);
    if (slot < N - 1) {
        edges[2 * slot] = lo;
        edges[2 * slot + 1] = hi;
        w2[slot] = __longlong_as_double((long long)compw[c]);
    }
}

// Dynamic LDS: p int32 [N] | m int32 [N]
__global__ __launch_bounds__(MS_MERGE) void mst_merge_k(int N, const int* __restrict__ parent, int* __restrict__ comp,
                                                        u64* __restrict__ compw, u64* __restrict__ compkey, int* state) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mg_lds[];
    __shared__ int roots;
    int* p = reinterpret_cast<int*>(mg_lds);
    int* m = p + N;
    const int tid = threadIdx.x;
    const bool done = state[MST_DONE] != 0;
    if (tid == 0) roots = 0;
    __syncthreads();                                        // every thread has read done before thread 0 may write it
    if (done) return;
    for (int i = tid; i < N; i += MS_MERGE) {
        p[i] = parent[i];
        m[i] = N;
    }
    __syncthreads();
    // in place: a racing read sees an entry's old or new value, both ancestors, so an entry only moves towards its root and
    // no later than it would with two buffers
    for (int it = 0; it < MS_JUMPS; ++it) {
        for (int i = tid; i < N; i += MS_MERGE) p[i] = p[p[i]];
        __syncthreads();
    }
    for (int i = tid; i < N; i += MS_MERGE) atomicMin(&m[p[i]], i);
    __syncthreads();
    int mine = 0;
    for (int i = tid; i < N; i += MS_MERGE) {
        const int c = m[p[i]];
        comp[i] = c;
        mine += c == i;
        compw[i] = MS_NONE;
        compkey[i] = MS_NONE;
    }
    if (mine) atomicAdd(&roots, mine);
    __syncthreads();
    if (tid == 0) {
        state[MST_ROUNDS] += 1;
        state[MST_COMPS] = roots;
        if (roots <= 1) state[MST_DONE] = 1;
    }
}

static bool mst_ok(int N, int L) { return N >= 2 && N <= MS_MAX_N && L >= 1 && L <= MS_MAX_L; }

static size_t mst_search_lds(int L) {
    return (((size_t)L * MS_CS * sizeof(float) + 15) & ~(size_t)15) + (size_t)MS_ROWS * L * sizeof(double) +
           64 * (sizeof(double) + sizeof(int));
}

static bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

// ---- the host tree ------------------------------------------------------------------------------------------------------

static int uf_find(std::vector<int>& f, int x) {
    while (f[x] != x) {
        f[x] = f[f[x]];
        x = f[x];
    }
    return x;
}

// the edges span 0 .. N - 1 as a tree and the weights are finite, non-negative and ascending
static const char* tree_input_error(const int* edges, const double* d, int N) {
    std::vector<int> f(N);
    for (int i = 0; i < N; ++i) f[i] = i;
    for (int e = 0; e < N - 1; ++e) {
        const int a = edges[2 * e], b = edges[2 * e + 1];
        if (a < 0 || a >= N || b < 0 || b >= N) return "an edge's end is outside 0 .. N - 1";
        if (!(d[e] >= 0.0) || !std::isfinite(d[e])) return "a weight is negative, infinite or NaN";
        if (e > 0 && d[e] < d[e - 1]) return "the weights descend";
        const int ra = uf_find(f, a), rb = uf_find(f, b);
        if (ra == rb) return "the edges hold a cycle (N - 1 edges: they are no spanning tree)";
        f[ra] = rb;
    }
    return nullptr;
}

struct Dendrogram {                                 // nodes 0 .. N - 1 are the rows; an inner node is born at distance dist
    std::vector<int> size, minrow, first, next;
    std::vector<double> dist;
    int root;
};

// multiway: all edges of one weight are added at once, and every component that absorbed older ones is one node
static Dendrogram build_dendrogram(const int* edges, const double* d, int N) {
    Dendrogram t;
    t.size.assign(N, 1);
    t.minrow.resize(N);
    t.first.assign(N, -1);
    t.next.assign(N, -1);
    t.dist.assign(N, 0.0);
    std::vector<int> f(N), usize(N, 1), nodeof(N), seen(N, -1), made(N, -1), newid(N);
    std::vector<int> olds, oldnodes, ra, rb;
    for (int i = 0; i < N; ++i) f[i] = nodeof[i] = t.minrow[i] = i;
    int level = 0;
    for (int e = 0; e < N - 1; ++level) {
        int g = e;
        while (g < N - 1 && d[g] == d[e]) ++g;
        olds.clear();
        oldnodes.clear();
        for (int k = e; k < g; ++k)
            for (int side = 0; side < 2; ++side) {
                const int r = uf_find(f, edges[2 * k + side]);
                if (seen[r] != level) {
                    seen[r] = level;
                    olds.push_back(r);
                    oldnodes.push_back(nodeof[r]);
                }
            }
        for (int k = e; k < g; ++k) {
            int a = uf_find(f, edges[2 * k]), b = uf_find(f, edges[2 * k + 1]);
            if (usize[a] < usize[b]) std::swap(a, b);
            f[b] = a;
            usize[a] += usize[b];
        }
        for (size_t k = 0; k < olds.size(); ++k) {
            const int nr = uf_find(f, olds[k]), ch = oldnodes[k];
            if (made[nr] != level) {
                made[nr] = level;
                newid[nr] = (int)t.size.size();
                t.size.push_back(0);
                t.minrow.push_back(N);
                t.first.push_back(-1);
                t.next.push_back(-1);
                t.dist.push_back(d[e]);
            }
            const int v = newid[nr];
            t.size[v] += t.size[ch];
            t.minrow[v] = std::min(t.minrow[v], t.minrow[ch]);
            t.next[ch] = t.first[v];
            t.first[v] = ch;
        }
        for (size_t k = 0; k < olds.size(); ++k) {
            const int nr = uf_find(f, olds[k]);
            nodeof[nr] = newid[nr];
        }
        e = g;
    }
    t.root = (int)t.size.size() - 1;
    return t;
}

static int tree_shape_error(const char* name, int N, int mcs) {
    if (N < 2 || N > MS_MAX_N) return fail(RBVAE_E_UNSUPPORTED, "%s: N=%d outside 2 <= N <= %d", name, N, MS_MAX_N);
    if (mcs < 2 || mcs > N) return fail(RBVAE_E_INVALID, "%s: min_cluster_size=%d outside 2 .. N=%d", name, mcs, N);
    return RBVAE_OK;
}

}  // namespace rbvae

using namespace rbvae;

extern "C" int rbvae_mst_ok(int N, int L) { return mst_ok(N, L) ? 1 : 0; }

extern "C" size_t rbvae_mst_ws_bytes(int N) { return mst_ok(N, 1) ? mst_ws_bytes(N) : 0; }

#define MS_CHECK_SHAPE(name)                                                                                           \
    do {                                                                                                               \
        if (!mst_ok(N, L))                                                                                             \
            return fail(RBVAE_E_UNSUPPORTED, name ": (N=%d, L=%d) outside 2 <= N <= %d, 1 <= L <= %d", N, L, MS_MAX_N, \
                        MS_MAX_L);                                                                                     \
    } while (0)

extern "C" int rbvae_mst_start(int N, int* comp, int* state, void* ws, void* stream) {
    const int L = 1;
    MS_CHECK_SHAPE("mst_start");
    RBVAE_CHECK_ARG(comp && state && ws, "mst_start: null pointer");
    RBVAE_CHECK_ARG(((uintptr_t)ws & 7) == 0 && ((uintptr_t)comp & 3) == 0 && ((uintptr_t)state & 3) == 0,
                    "mst_start: ws must be 8-byte aligned, comp and state 4-byte aligned");
    const size_t nb = mst_ws_bytes(N);
    RBVAE_CHECK_ARG(!overlap(comp, (size_t)4 * N, ws, nb) && !overlap(state, 16, ws, nb) && !overlap(comp, (size_t)4 * N, state, 16),
                    "mst_start: comp, state and ws overlap");
    const MstWs w = mst_ws(ws, N);
    hipLaunchKernelGGL(mst_start_k, dim3(cdiv(N, MS_THREADS)), dim3(MS_THREADS), 0, (hipStream_t)stream, N, comp, w.compw,
                       w.compkey, state);
    RBVAE_CHECK_LAUNCH("mst_start");
    return RBVAE_OK;
}

static int mst_run(const float* X, const double* core2, int N, int L, int* comp, int* edges, double* w2, int* state, void* ws,
                   void* stream, bool search_only) {
    MS_CHECK_SHAPE("mst_round");
    RBVAE_CHECK_ARG(X && core2 && comp && edges && w2 && state && ws, "mst_round: null pointer");
    RBVAE_CHECK_ARG((((uintptr_t)core2 | (uintptr_t)w2 | (uintptr_t)ws) & 7) == 0 &&
                        (((uintptr_t)X | (uintptr_t)comp | (uintptr_t)edges | (uintptr_t)state) & 3) == 0,
                    "mst_round: core2, w2 and ws must be 8-byte aligned, X, comp, edges and state 4-byte aligned");
    {
        const void* p[7] = {X, core2, comp, edges, w2, state, ws};
        const size_t n[7] = {(size_t)4 * N * L, (size_t)8 * N, (size_t)4 * N, (size_t)8 * (N - 1), (size_t)8 * (N - 1), 16,
                             mst_ws_bytes(N)};
        for (int a = 0; a < 7; ++a)
            for (int b = std::max(a + 1, 2); b < 7; ++b)    // X and core2 are only read: they may share storage
                RBVAE_CHECK_ARG(!overlap(p[a], n[a], p[b], n[b]), "mst_round: buffers %d and %d overlap", a, b);
    }
    const MstWs w = mst_ws(ws, N);
    hipStream_t s = (hipStream_t)stream;
    const int tiles = cdiv(N, 64), blocks = cdiv(N, MS_ROWS);
    int S = std::min(std::min(MS_MAX_S, tiles), std::max(1, cdiv(1024, blocks)));      // enough workgroups for 256 CUs
    const int slice_cols = cdiv(tiles, S) * 64;
    S = cdiv(N, slice_cols);                                // no empty slice
    const size_t lds = mst_search_lds(L), mlds = (size_t)8 * N;
    static size_t reserved = 0, mreserved = 0;              // process-wide, as rbvae_knn's
    if (lds > reserved) {
        if (hipFuncSetAttribute((const void*)mst_search_k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return fail(RBVAE_E_LAUNCH, "mst_round: cannot reserve %zu bytes of LDS", lds);
        reserved = lds;
    }
    if (mlds > mreserved) {
        if (hipFuncSetAttribute((const void*)mst_merge_k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)mlds) != hipSuccess)
            return fail(RBVAE_E_LAUNCH, "mst_round: cannot reserve %zu bytes of LDS", mlds);
        mreserved = mlds;
    }
    const dim3 rows(cdiv(N, MS_THREADS)), thr(MS_THREADS);
    hipLaunchKernelGGL(mst_search_k, dim3(blocks, S), thr, lds, s, X, core2, (const int*)comp, N, L, slice_cols, w.part_w,
                       w.part_j, (const int*)state);
    RBVAE_CHECK_LAUNCH("mst_round (search)");
    if (search_only) return RBVAE_OK;
    hipLaunchKernelGGL(mst_rowmin_k, rows, thr, 0, s, (const u64*)w.part_w, (const int*)w.part_j, N, S, (const int*)comp,
                       w.candw, w.candj, w.compw, (const int*)state);
    RBVAE_CHECK_LAUNCH("mst_round (row minima)");
    hipLaunchKernelGGL(mst_key_k, rows, thr, 0, s, (const u64*)w.candw, (const int*)w.candj, N, (const int*)comp,
                       (const u64*)w.compw, w.compkey, (const int*)state);
    RBVAE_CHECK_LAUNCH("mst_round (component keys)");
    hipLaunchKernelGGL(mst_hook_k, rows, thr, 0, s, N, (const int*)comp, (const u64*)w.compw, (const u64*)w.compkey, w.parent,
                       edges, w2, state);
    RBVAE_CHECK_LAUNCH("mst_round (hook)");
    hipLaunchKernelGGL(mst_merge_k, dim3(1), dim3(MS_MERGE), mlds, s, N, (const int*)w.parent, comp, w.compw, w.compkey, state);
    RBVAE_CHECK_LAUNCH("mst_round (merge)");
    return RBVAE_OK;
}

extern "C" int rbvae_mst_round(const float* X, const double* core2, int N, int L, int* comp, int* edges, double* w2,
                               int* state, void* ws, void* stream) {
    return mst_run(X, core2, N, L, comp, edges, w2, state, ws, stream, false);
}

extern "C" int rbvae_mst_search(const float* X, const double* core2, int N, int L, int* comp, int* edges, double* w2,
                                int* state, void* ws, void* stream) {
    return mst_run(X, core2, N, L, comp, edges, w2, state, ws, stream, true);
}

extern "C" int rbvae_hdbscan_tree(const int* edges, const double* d, int N, int min_cluster_size, int method, int* labels,
                                  double* prob, int* cl_parent, double* cl_birth, double* cl_lambda_max, double* cl_stability,
                                  int* cl_size, int* cl_selected, int* cl_min_row, int* n_table) {
    const int mcs = min_cluster_size;
    if (int rc = tree_shape_error("hdbscan_tree", N, mcs)) return rc;
    RBVAE_CHECK_ARG(method == 0 || method == 1, "hdbscan_tree: method=%d is neither 0 (eom) nor 1 (leaf)", method);
    RBVAE_CHECK_ARG(edges && d && labels && prob && cl_parent && cl_birth && cl_lambda_max && cl_stability && cl_size &&
                        cl_selected && cl_min_row && n_table, "hdbscan_tree: null pointer");
    if (const char* why = tree_input_error(edges, d, N)) return fail(RBVAE_E_INVALID, "hdbscan_tree: %s", why);
    const double inf = std::numeric_limits<double>::infinity();
    const Dendrogram t = build_dendrogram(edges, d, N);

    // the condensed tree, top down; a cluster's levels are met in ascending lambda
    std::vector<int> parent{-1}, size{N}, minrow{0};
    std::vector<double> birth{0.0}, lmax{0.0}, stab{0.0};
    std::vector<int> row_cl(N, 0);
    std::vector<double> row_lam(N, 0.0);
    std::vector<std::pair<int, int>> todo{{t.root, 0}};
    std::vector<int> big, walk;
    while (!todo.empty()) {
        const int v = todo.back().first, C = todo.back().second;
        todo.pop_back();
        const double lam = t.dist[v] == 0.0 ? inf : 1.0 / t.dist[v];
        long leaving = 0;
        big.clear();
        for (int ch = t.first[v]; ch >= 0; ch = t.next[ch]) {
            if (t.size[ch] >= mcs) {
                big.push_back(ch);
                continue;
            }
            leaving += t.size[ch];
            walk.assign(1, ch);
            while (!walk.empty()) {
                const int x = walk.back();
                walk.pop_back();
                if (x < N) {
                    row_cl[x] = C;
                    row_lam[x] = lam;
                }
                for (int y = t.first[x]; y >= 0; y = t.next[y]) walk.push_back(y);
            }
        }
        if (big.size() >= 2) {
            for (int ch : big) {
                leaving += t.size[ch];
                todo.push_back({ch, (int)parent.size()});
                parent.push_back(C);
                size.push_back(t.size[ch]);
                minrow.push_back(t.minrow[ch]);
                birth.push_back(lam);
                lmax.push_back(0.0);
                stab.push_back(0.0);
            }
        } else if (big.size() == 1) {
            todo.push_back({big[0], C});
        }
        const double term = (lam - birth[C]) * (double)leaving;
        stab[C] = stab[C] + term;
        lmax[C] = lam;
    }

    // the table's order: (birth, smallest row) ascending, so a parent stands before its children
    const int K = (int)parent.size();
    std::vector<int> order(K), rank(K);
    for (int c = 0; c < K; ++c) order[c] = c;
    std::sort(order.begin(), order.end(), [&](int a, int b) {
        return birth[a] < birth[b] || (birth[a] == birth[b] && minrow[a] < minrow[b]);
    });
    for (int k = 0; k < K; ++k) rank[order[k]] = k;
    std::vector<int> tp(K), nchild(K, 0), start(K + 1, 0), kids(K > 1 ? K - 1 : 0), sel(K, 0);
    for (int k = 0; k < K; ++k) tp[k] = parent[order[k]] < 0 ? -1 : rank[parent[order[k]]];
    for (int k = 1; k < K; ++k) ++nchild[tp[k]];
    for (int k = 0; k < K; ++k) start[k + 1] = start[k] + nchild[k];
    {
        std::vector<int> at(start.begin(), start.end() - 1);
        for (int k = 1; k < K; ++k) kids[at[tp[k]]++] = k;  // k ascends: a cluster's children stand in ascending order
    }
    if (method == 0) {
        std::vector<double> s(K);
        for (int k = 0; k < K; ++k) s[k] = stab[order[k]];
        for (int k = K - 1; k >= 1; --k) {
            sel[k] = 1;
            if (nchild[k]) {
                double sum = 0.0;
                for (int q = start[k]; q < start[k + 1]; ++q) sum = sum + s[kids[q]];
                if (sum > s[k]) {
                    s[k] = sum;
                    sel[k] = 0;
                }
            }
        }
        std::vector<char> covered(K, 0);
        for (int k = 1; k < K; ++k) {
            covered[k] = sel[tp[k]] || covered[tp[k]];
            if (covered[k]) sel[k] = 0;
        }
    } else {
        for (int k = 1; k < K; ++k) sel[k] = nchild[k] == 0;
    }
    std::vector<int> anc(K, -1), id(K, -1), chosen;
    for (int k = 1; k < K; ++k) anc[k] = sel[k] ? k : anc[tp[k]];
    for (int k = 1; k < K; ++k)
        if (sel[k]) chosen.push_back(k);
    std::sort(chosen.begin(), chosen.end(), [&](int a, int b) { return minrow[order[a]] < minrow[order[b]]; });
    for (size_t q = 0; q < chosen.size(); ++q) id[chosen[q]] = (int)q;

    for (int i = 0; i < N; ++i) {
        const int a = anc[rank[row_cl[i]]];
        if (a < 0) {
            labels[i] = -1;
            prob[i] = 0.0;
            continue;
        }
        labels[i] = id[a];
        const double lm = lmax[order[a]], lr = row_lam[i];
        prob[i] = (lm == 0.0 || std::isinf(lr)) ? 1.0 : (lr < lm ? lr : lm) / lm;
    }
    for (int k = 0; k < K; ++k) {
        const int c = order[k];
        cl_parent[k] = tp[k];
        cl_birth[k] = birth[c];
        cl_lambda_max[k] = lmax[c];
        cl_stability[k] = stab[c];
        cl_size[k] = size[c];
        cl_selected[k] = sel[k];
        cl_min_row[k] = minrow[c];
    }
    n_table[0] = K;
    return RBVAE_OK;
}

extern "C" int rbvae_hdbscan_cut(const int* edges, const double* d, int N, double cut_distance, int min_cluster_size,
                                 int* labels, int* n_clusters) {
    if (int rc = tree_shape_error("hdbscan_cut", N, min_cluster_size)) return rc;
    RBVAE_CHECK_ARG(edges && d && labels && n_clusters, "hdbscan_cut: null pointer");
    RBVAE_CHECK_ARG(cut_distance >= 0.0, "hdbscan_cut: cut_distance=%g is negative or NaN", cut_distance);
    if (const char* why = tree_input_error(edges, d, N)) return fail(RBVAE_E_INVALID, "hdbscan_cut: %s", why);
    std::vector<int> f(N), size(N, 1), id(N, -1);
    for (int i = 0; i < N; ++i) f[i] = i;
    for (int e = 0; e < N - 1 && d[e] <= cut_distance; ++e) {
        int a = uf_find(f, edges[2 * e]), b = uf_find(f, edges[2 * e + 1]);
        if (size[a] < size[b]) std::swap(a, b);
        f[b] = a;
        size[a] += size[b];
    }
    int n = 0;
    for (int i = 0; i < N; ++i) {                           // i ascends: a component is numbered at its smallest row
        const int r = uf_find(f, i);
        if (size[r] < min_cluster_size) {
            labels[i] = -1;
            continue;
        }
        if (id[r] < 0) id[r] = n++;
        labels[i] = id[r];
    }
    n_clusters[0] = n;
    return RBVAE_OK;
}
