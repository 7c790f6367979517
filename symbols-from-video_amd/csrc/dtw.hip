// Two sequences aligned: dynamic time warping of the N rows of X against the M rows of Y (both in time order) with the
// step pattern {diagonal, up, left}, optionally inside a Sakoe-Chiba band or with open ends on Y (subsequence mode).
// include/rbvae_hip.h has the definition; tests/_dtw_ref.py restates it operation for operation.
//   dtw_prefill_k   with a band only: dirs = 3 everywhere, last_row and table = +inf, so tiles wholly outside the band
//                   are never launched (or return at once) and still read as the contract says
//   dtw_tile_k      a workgroup owns a DT_TI x DT_TJ tile of the table.  The tiles of one anti-diagonal are independent:
//                   one launch per tile anti-diagonal, and the launch order on the stream is the only dependency -- no
//                   workgroup ever waits for another.  Phase 1, all four waves: the tile's costs into LDS, the rows of X
//                   and Y passing through LDS in chunks of DT_LC coordinates as [l][row] f64 images, a thread holding a
//                   4 x 4 tile of d2_step accumulators (segment.hip's layer kernel); packed codes: the popcount of the
//                   XOR.  Phase 2, wave 0: lane r owns row r and is at column s - r in step s; D[i-1][j] comes from lane
//                   r - 1 by a lane shift, D[i-1][j-1] is the value that shift brought one step earlier, D[i][j-1] the
//                   lane's own last result; no barrier inside the chain.  D overwrites the cost in LDS.  Phase 3, all
//                   waves: the tile's last row into the frontier row, its last column into the frontier column, its
//                   last cell into the corner table, the directions packed four to a byte, and the table when asked.
//   dtw_trace_k     one workgroup: the end cell (the argmin of last_row under key_less in subsequence mode), then the
//                   walk along dirs, a tile's 1 KB of directions staged in LDS by all threads and walked by thread 0,
//                   which writes the pairs from the last row of path downwards; then all threads move them to the front.
// Between tiles: frow f64 [M] holds the last row of the newest tile above in every column block, fcol f64 [N] the last
// column of the newest tile to the left in every row block; each block of either has one writer per launch, the tile that
// also read it.  The corner D[i0-1][j0-1] of tile (ti, tj) is neither: tile (ti, tj-1) overwrote frow[j0-1] and tile
// (ti-1, tj) fcol[i0-1] one launch earlier, so every full tile leaves its last cell in corner[ti][tj], written once.
// A frontier value is used only where its cell lies inside the band, +inf otherwise, so a tile that never ran is never read.
// No floating-point atomics; two runs agree bit for bit.  Contraction is off.
// Many pairs (two stacks of sequences and a pair list, a device plan with one row per pair): dtw_tile_k<., true> and
// dtw_trace_k<true> take the pair from blockIdx.y / blockIdx.x and everything about it from its plan row, each pair with its own
// frontiers and corners, so one launch serves the same tile anti-diagonal of all pairs and every pair's bytes are those of the
// single-pair kernels.  dtw_ranges_k and dtw_bary_update_k are the two launches of a DBA step.
#include "common.h"
#include "pairdist.h"

#include <math.h>

#include <vector>

#pragma clang fp contract(off)

namespace rbvae {

constexpr int DTW_MAX_N = 16384, DTW_MAX_L = 128;
constexpr int DT_THREADS = 256;
constexpr int DT_TI = 64, DT_TJ = 64;   // tile edges: DT_TI is the wave (a lane per row), DT_TJ a multiple of 4 (a byte of dirs)
constexpr int DT_LC = 16;               // coordinates per LDS chunk
constexpr int DT_PRE = 2 * DT_TI * DT_LC / DT_THREADS;   // values of a chunk a thread stages
constexpr int DT_LD = DT_TI + 2;        // f64 stride of an [l][row] image: 528 B keeps 16-byte reads aligned
static_assert(DT_TI == 64 && DT_TJ == DT_TI, "a lane per row; the band's tile range assumes square tiles");

__device__ __forceinline__ bool dtw_in_band(int i, int j, int window) { return window < 0 || abs(i - j) <= window; }

// lane r takes lane r - 1's value, lane 0 keeps its own: a wave shift right by one lane in the data-parallel primitives
// (dpp_ctrl 0x138), two register moves where a shuffle goes through the LDS crossbar and waits for it
__device__ __forceinline__ double lane_up1(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(lo, lo, 0x138, 0xf, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(hi, hi, 0x138, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

__global__ __launch_bounds__(DT_THREADS) void dtw_prefill_k(int N, int M, unsigned char* __restrict__ dirs,
                                                            double* __restrict__ last_row, double* __restrict__ table) {
    const long W4 = (M + 3) >> 2, nd = (long)N * W4, nt = (long)N * M;
    const long g = (long)blockIdx.x * DT_THREADS + threadIdx.x, step = (long)gridDim.x * DT_THREADS;
    for (long e = g; e < nd; e += step) dirs[e] = 0xFF;
    for (long e = g; e < M; e += step) last_row[e] = INFINITY;
    if (table)
        for (long e = g; e < nt; e += step) table[e] = INFINITY;
}

// The dependent chain of one tile on one wave.  Lane r owns row r and is at column c = s - r in step s.  The cost and the
// frontier value of the lane's next column are read one step ahead, so a step waits for nothing but the neighbour's last
// result; there is no branch in the loop: every choice is a select, and a lane outside its row's columns stores to a spare
// slot of its own.  EDGE: the tile may hold start cells (row 0) or cells outside the band.
template <bool EDGE>
__device__ __forceinline__ void dtw_chain(double* cst, unsigned char* sd, const double* fr, double* spare,
                                          unsigned char* spare_d, int r, int i, int j0, int nr, int nc, int window, int sub,
                                          double left, double pu) {
    double* crow = cst + r * DT_TJ;
    unsigned char* drow = sd + r * DT_TJ;
    const bool row_ok = r < nr;
    const int steps = nr + nc - 1;
    double d_n = crow[0], f_n = fr[0];
    int c = -r;
#pragma unroll 2
    for (int s = 0; s < steps; ++s, ++c) {
        double up = lane_up1(left);                         // lane r - 1 finished column c one step ago
        const double d = d_n, f = f_n;
        const int cn = min(max(c + 1, 0), DT_TJ - 1);
        d_n = crow[cn];
        f_n = fr[cn];
        up = r == 0 ? f : up;
        const bool dg = pu <= up && pu <= left, ul = up <= left;    // diagonal, then up, then left
        double v = d + (dg ? pu : (ul ? up : left));
        int dir = dg ? 0 : (ul ? 1 : 2);
        if (EDGE) {
            const int j = j0 + c;
            const bool start = i == 0 && (sub || j == 0), out = !dtw_in_band(i, j, window);
            v = out ? INFINITY : (start ? d : v);
            dir = (start || out) ? 3 : dir;
        }
        const bool act = row_ok && (unsigned)c < (unsigned)nc;
        *(act ? crow + c : spare + r) = v;
        *(act ? drow + c : spare_d + r) = (unsigned char)dir;
        pu = act ? up : pu;
        left = act ? v : left;
    }
}

// The device plan of a batch of pairs (rbvae_dtw_pairs_plan): DP_HDR int64 of header {P, the rows of the X stack, of the Y
// stack, 0}, then DP_ROW int64 per pair.  The offsets count what the header says: rows, bytes of dirs, doubles of last_row
// and of ws, rows of path.
constexpr int DP_HDR = 4, DP_ROW = 10;
enum { DP_X0, DP_Y0, DP_N, DP_M, DP_NTI, DP_NTJ, DP_DIRS, DP_LAST, DP_WS, DP_PATH };

// the extents of the arrays a batched launch was given: every index read from the plan is clamped to them
struct DtwExt {
    long x_rows, y_rows, dirs_bytes, last_n, ws_n, path_rows;
};

struct DtwPair {
    long x0, y0, dirs, last, ws, path;
    int n, m, nTi, nTj;
    bool ok;
};

__device__ __forceinline__ long clampl(long v, long lo, long hi) { return (v > hi ? hi : v) < lo ? lo : (v > hi ? hi : v); }

// Pair p of the plan with every index inside the extents (an extent of 0 means that the launch does not touch that array).
// A stale plan gives wrong numbers; a pair whose block fits nowhere is skipped (ok = false).
__device__ __forceinline__ DtwPair dtw_pair(const long* __restrict__ plan, int p, const DtwExt& e) {
    const long* r = plan + DP_HDR + (long)p * DP_ROW;
    DtwPair q;
    q.n = (int)clampl(r[DP_N], 1, e.x_rows < DTW_MAX_N ? e.x_rows : DTW_MAX_N);
    q.m = (int)clampl(r[DP_M], 1, e.y_rows < DTW_MAX_N ? e.y_rows : DTW_MAX_N);
    q.nTi = (q.n + DT_TI - 1) / DT_TI;                      // the tile counts follow the clamped lengths
    q.nTj = (q.m + DT_TJ - 1) / DT_TJ;
    const long W4 = (q.m + 3) >> 2, wsn = (long)q.n + q.m + (long)q.nTi * q.nTj, cap = (long)q.n + q.m - 1;
    q.x0 = clampl(r[DP_X0], 0, e.x_rows - q.n);
    q.y0 = clampl(r[DP_Y0], 0, e.y_rows - q.m);
    q.dirs = clampl(r[DP_DIRS], 0, e.dirs_bytes - q.n * W4);
    q.last = clampl(r[DP_LAST], 0, e.last_n - q.m);
    q.ws = clampl(r[DP_WS], 0, e.ws_n - wsn);
    q.path = clampl(r[DP_PATH], 0, e.path_rows - cap);
    q.ok = e.x_rows >= 1 && e.y_rows >= 1 && (e.dirs_bytes == 0 || e.dirs_bytes >= q.n * W4) &&
           (e.last_n == 0 || e.last_n >= q.m) && (e.ws_n == 0 || e.ws_n >= wsn) && (e.path_rows == 0 || e.path_rows >= cap);
    return q;
}

// grid: the tiles ti_lo .. of tile anti-diagonal `diag`, tj = diag - ti.  metric 0 / 1: X, Y f32 [.][L]; BITS: uint32 [.][4].
// PAIRS: grid (the most tiles one pair has on this diagonal, P): the pair is blockIdx.y, whose plan row gives the rows of X
// and Y, N, M, nTj, its own frow / fcol / corner inside ws and its blocks of dirs and last_row; blockIdx.x counts the pair's
// tiles on the diagonal from its own first one, and a workgroup beyond its last one returns before any work.  No band, no
// open ends, no table.  Everything after that is the single pair's code.
template <bool BITS, bool PAIRS>
__global__ __launch_bounds__(DT_THREADS) void dtw_tile_k(const void* __restrict__ Xv, const void* __restrict__ Yv, int N, int M,
                                                         int L, int root, int window, int sub, int diag, int ti_lo, int nTj,
                                                         double* __restrict__ frow, double* __restrict__ fcol,
                                                         double* __restrict__ corner, unsigned char* __restrict__ dirs,
                                                         double* __restrict__ last_row, double* __restrict__ table,
                                                         const long* __restrict__ plan, DtwExt ext) {
    if constexpr (PAIRS) {
        const DtwPair q = dtw_pair(plan, blockIdx.y, ext);
        ti_lo = diag - (q.nTj - 1) > 0 ? diag - (q.nTj - 1) : 0;
        const int ti_hi = diag < q.nTi - 1 ? diag : q.nTi - 1;
        if (!q.ok || ti_lo + (int)blockIdx.x > ti_hi) return;   // this pair has no such tile on this diagonal
        Xv = static_cast<const char*>(Xv) + q.x0 * (BITS ? 16 : 4 * (long)L);
        Yv = static_cast<const char*>(Yv) + q.y0 * (BITS ? 16 : 4 * (long)L);
        N = q.n, M = q.m, nTj = q.nTj, window = -1, sub = 0, table = nullptr;
        frow += q.ws;                                       // the single pair's workspace layout, the pair's own
        fcol = frow + M;
        corner = fcol + N;
        dirs += q.dirs;
        last_row += q.last;
    }
    __shared__ __attribute__((aligned(16))) double cst[DT_TI * DT_TJ];      // the costs, then D
    __shared__ __attribute__((aligned(16))) double px[DT_LC * DT_LD];
    __shared__ __attribute__((aligned(16))) double py[DT_LC * DT_LD];
    __shared__ double fr[DT_TJ];                                            // D[i0 - 1][j0 ..]
    __shared__ unsigned char sd[DT_TI * DT_TJ];                             // a direction per cell
    __shared__ double spare[64];                                            // where a lane outside its columns stores
    __shared__ unsigned char spare_d[64];
    const int ti = ti_lo + blockIdx.x, tj = diag - ti;
    const int i0 = ti * DT_TI, j0 = tj * DT_TJ;
    const int nr = min(DT_TI, N - i0), nc = min(DT_TJ, M - j0);             // ragged tiles: rows and columns inside the table
    if (window >= 0 && (i0 - (j0 + nc - 1) > window || j0 - (i0 + nr - 1) > window)) return;    // wholly outside the band
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;

    // ---- phase 1: the costs ----
    if constexpr (BITS) {
        uint32_t* bx = reinterpret_cast<uint32_t*>(px);
        uint32_t* by = reinterpret_cast<uint32_t*>(py);
        const uint32_t* X = static_cast<const uint32_t*>(Xv);
        const uint32_t* Y = static_cast<const uint32_t*>(Yv);
        for (int e = tid; e < 2 * DT_TI * 4; e += DT_THREADS) {
            const int side = e / (DT_TI * 4), f = e - side * (DT_TI * 4);
            const int r = f >> 2;
            if (side) by[f] = r < nc ? Y[(long)(j0 + r) * 4 + (f & 3)] : 0u;
            else bx[f] = r < nr ? X[(long)(i0 + r) * 4 + (f & 3)] : 0u;
        }
        __syncthreads();
        for (int e = tid; e < DT_TI * DT_TJ; e += DT_THREADS) {
            const int r = e / DT_TJ, c = e - r * DT_TJ;
            int p = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) p += __popc(bx[r * 4 + w] ^ by[c * 4 + w]);
            cst[e] = (double)p;
        }
    } else {
        const float* X = static_cast<const float*>(Xv);
        const float* Y = static_cast<const float*>(Yv);
        double acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
        // a chunk is 2 x DT_TI x DT_LC values, DT_PRE a thread; the next chunk's are loaded into registers before this chunk's
        // arithmetic and stored to LDS after it, so the loads' latency hides behind the d2_steps
        float pre[DT_PRE];
        auto load_chunk = [&](int l0) {
            const int lc = min(DT_LC, L - l0);
#pragma unroll
            for (int q = 0; q < DT_PRE; ++q) {
                const int e = tid + q * DT_THREADS;
                const int side = e / (DT_TI * DT_LC), f = e - side * (DT_TI * DT_LC);
                const int r = f / DT_LC, l = f - r * DT_LC;
                float v = 0.f;                              // rows past N or M are never read
                if (l < lc) {
                    if (side) { if (r < nc) v = Y[(long)(j0 + r) * L + l0 + l]; }
                    else { if (r < nr) v = X[(long)(i0 + r) * L + l0 + l]; }
                }
                pre[q] = v;
            }
        };
        load_chunk(0);
        for (int l0 = 0; l0 < L; l0 += DT_LC) {
            const int lc = min(DT_LC, L - l0);
            if (l0) __syncthreads();                        // the previous chunk's reads are done
#pragma unroll
            for (int q = 0; q < DT_PRE; ++q) {
                const int e = tid + q * DT_THREADS;
                const int side = e / (DT_TI * DT_LC), f = e - side * (DT_TI * DT_LC);
                const int r = f / DT_LC, l = f - r * DT_LC;
                (side ? py : px)[l * DT_LD + r] = (double)pre[q];
            }
            __syncthreads();
            if (l0 + DT_LC < L) load_chunk(l0 + DT_LC);
#pragma unroll 2
            for (int l = 0; l < lc; ++l) {
                const double2 a0 = *reinterpret_cast<const double2*>(px + l * DT_LD + 2 * ty);
                const double2 a1 = *reinterpret_cast<const double2*>(px + l * DT_LD + 32 + 2 * ty);
                const double2 b0 = *reinterpret_cast<const double2*>(py + l * DT_LD + 2 * tx);
                const double2 b1 = *reinterpret_cast<const double2*>(py + l * DT_LD + 32 + 2 * tx);
                const double a[4] = {a0.x, a0.y, a1.x, a1.y}, b[4] = {b0.x, b0.y, b1.x, b1.y};
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) d2_step(acc[i][j], a[i], b[j]);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = (i >> 1) * 32 + 2 * ty + (i & 1);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = (j >> 1) * 32 + 2 * tx + (j & 1);
                cst[r * DT_TJ + c] = root ? sqrt(acc[i][j]) : acc[i][j];
            }
        }
    }
    if (tid < DT_TJ) {
        const int j = j0 + tid;
        fr[tid] = (i0 > 0 && tid < nc && dtw_in_band(i0 - 1, j, window)) ? frow[j] : INFINITY;
    }
    __syncthreads();

    // ---- phase 2: the chain, wave 0, lane = row ----
    if (tid < 64) {
        const int r = tid, i = i0 + r;
        const bool row_ok = r < nr;
        const double left = (j0 > 0 && row_ok && dtw_in_band(i, j0 - 1, window)) ? fcol[i] : INFINITY;   // D[i][j0 - 1]
        double pu = lane_up1(left);                                                                        // D[i - 1][j0 - 1]
        if (r == 0)
            pu = (i0 > 0 && j0 > 0 && dtw_in_band(i0 - 1, j0 - 1, window)) ? corner[(long)(ti - 1) * nTj + tj - 1] : INFINITY;
        const bool cut = window >= 0 && (i0 + nr - 1 - j0 > window || j0 + nc - 1 - i0 > window);   // the band's edge crosses the tile
        if (cut || i0 == 0)                                 // the same in every lane: only such tiles hold start or band cells
            dtw_chain<true>(cst, sd, fr, spare, spare_d, r, i, j0, nr, nc, window, sub, left, pu);
        else
            dtw_chain<false>(cst, sd, fr, spare, spare_d, r, i, j0, nr, nc, window, sub, left, pu);
    }
    __syncthreads();

    // ---- phase 3: what the neighbours and the caller read ----
    if (tid < nc) {
        const double v = cst[(nr - 1) * DT_TJ + tid];
        frow[j0 + tid] = v;
        if (i0 + nr == N) last_row[j0 + tid] = v;
    }
    if (tid < nr) fcol[i0 + tid] = cst[tid * DT_TJ + nc - 1];
    if (tid == 0 && nr == DT_TI && nc == DT_TJ) corner[(long)ti * nTj + tj] = cst[DT_TI * DT_TJ - 1];
    const long W4 = (M + 3) >> 2;
    for (int e = tid; e < DT_TI * (DT_TJ / 4); e += DT_THREADS) {
        const int r = e / (DT_TJ / 4), b = e - r * (DT_TJ / 4);
        if (r < nr && 4 * b < nc) {
            unsigned v = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) v |= (4 * b + q < nc ? (unsigned)sd[r * DT_TJ + 4 * b + q] : 3u) << (2 * q);
            dirs[(long)(i0 + r) * W4 + (j0 >> 2) + b] = (unsigned char)v;
        }
    }
    if (table)
        for (int e = tid; e < DT_TI * DT_TJ; e += DT_THREADS) {
            const int r = e / DT_TJ, c = e - r * DT_TJ;
            if (r < nr && c < nc) table[(long)(i0 + r) * M + j0 + c] = cst[e];
        }
}

// state int32 [3] = {len, start_j, end_j}; len = -1 where dirs holds no walk from the end cell to row 0.  PAIRS: blockIdx.x is
// the pair, whose blocks of dirs, last_row and path come from its plan row, state + 3 p and cost + p; the same walk.
template <bool PAIRS>
__global__ __launch_bounds__(DT_THREADS) void dtw_trace_k(const unsigned char* __restrict__ dirs,
                                                          const double* __restrict__ last_row, int N, int M, int sub,
                                                          int* __restrict__ path, int* __restrict__ state,
                                                          double* __restrict__ cost, const long* __restrict__ plan, DtwExt ext) {
    if constexpr (PAIRS) {
        const DtwPair q = dtw_pair(plan, blockIdx.x, ext);
        if (!q.ok) return;
        N = q.n, M = q.m, sub = 0;
        dirs += q.dirs;
        last_row += q.last;
        path += 2 * q.path;
        state += 3 * (long)blockIdx.x;
        cost += blockIdx.x;
    }
    __shared__ unsigned char td[DT_TI * (DT_TJ / 4)];
    __shared__ double rv[DT_THREADS];
    __shared__ int rj[DT_THREADS];
    __shared__ int pos[4];                                  // i, j, steps so far, status (0 walking, 1 done, 2 malformed)
    const int tid = threadIdx.x;
    const long W4 = (M + 3) >> 2;
    int end_j = M - 1;
    if (sub) {                                              // the smallest last_row[j], the lowest j on a tie
        double bv = INFINITY;
        int bj = M;                                         // beats nothing: every j < M wins a tie against it
        for (int j = tid; j < M; j += DT_THREADS) {
            const double v = last_row[j];
            if (key_less(v, j, bv, bj)) {
                bv = v;
                bj = j;
            }
        }
        rv[tid] = bv;
        rj[tid] = bj;
        __syncthreads();
        for (int s = DT_THREADS / 2; s > 0; s >>= 1) {
            if (tid < s && key_less(rv[tid + s], rj[tid + s], rv[tid], rj[tid])) {
                rv[tid] = rv[tid + s];
                rj[tid] = rj[tid + s];
            }
            __syncthreads();
        }
        end_j = rj[0] < M ? rj[0] : 0;                      // all +inf or NaN: no end; the walk below still stays in range
    }
    const int cap = N + M - 1;                              // the rows of path: the longest walk there is
    int status = 0;
    if (tid == 0) {
        pos[0] = N - 1;
        pos[1] = end_j;
        pos[2] = 0;
        pos[3] = 0;
    }
    __syncthreads();
    while (true) {
        const int i = pos[0], j = pos[1];
        const int i0 = i / DT_TI * DT_TI, j0 = j / DT_TJ * DT_TJ;
        for (int e = tid; e < DT_TI * (DT_TJ / 4); e += DT_THREADS) {
            const int r = e / (DT_TJ / 4), b = e - r * (DT_TJ / 4);
            td[e] = (i0 + r < N && (j0 >> 2) + b < W4) ? dirs[(long)(i0 + r) * W4 + (j0 >> 2) + b] : 0xFF;
        }
        __syncthreads();
        if (tid == 0) {
            int ci = i, cj = j, k = pos[2], st = 0;
            while (ci >= i0 && cj >= j0) {                  // inside the staged tile
                if (k >= cap) {
                    st = 2;
                    break;
                }
                path[2 * (long)(cap - 1 - k)] = ci;         // the walk runs backwards: from the last row of path down
                path[2 * (long)(cap - 1 - k) + 1] = cj;
                ++k;
                const int dir = (td[(ci - i0) * (DT_TJ / 4) + ((cj - j0) >> 2)] >> (2 * (cj & 3))) & 3;
                if (dir == 3) {
                    st = (ci == 0 && (sub || cj == 0)) ? 1 : 2;
                    break;
                }
                if ((dir != 2 && ci == 0) || (dir != 1 && cj == 0)) {
                    st = 2;                                 // a step out of the table
                    break;
                }
                ci -= dir != 2;
                cj -= dir != 1;
            }
            pos[0] = ci;
            pos[1] = cj;
            pos[2] = k;
            pos[3] = st;
        }
        __syncthreads();
        status = pos[3];
        if (status) break;
        __syncthreads();                                    // pos and td are read before the next tile replaces them
    }
    const int len = pos[2], start_j = pos[1];
    // the pairs stand in rows cap - len .. cap - 1: down to rows 0 .. len - 1, a block of rows at a time from the front, every
    // block read whole before it is written (a row's new place lies below its old one, so no row is lost)
    const int off = cap - len;
    if (status == 1 && off > 0) {
        int2* p2 = reinterpret_cast<int2*>(path);
        for (int base = 0; base < len; base += DT_THREADS) {
            const int t = base + tid;
            int2 v = make_int2(0, 0);
            if (t < len) v = p2[off + t];
            __syncthreads();
            if (t < len) p2[t] = v;
            __syncthreads();
        }
    }
    if (tid == 0) {
        state[0] = status == 1 ? len : -1;
        state[1] = status == 1 ? start_j : -1;
        state[2] = end_j;
        cost[0] = last_row[end_j];
    }
}

static bool dtw_ok(long N, long M, long L, int metric, long window, int sub) {
    if (N < 1 || N > DTW_MAX_N || M < 1 || M > DTW_MAX_N || L < 1 || L > DTW_MAX_L) return false;
    if (metric < 0 || metric > 2 || window < -1 || (sub != 0 && sub != 1)) return false;
    if (window >= 0 && (sub || window < (N > M ? N - M : M - N))) return false;   // no path inside the band
    return true;
}

#define DTW_CHECK_SHAPE(name)                                                                                                  \
    do {                                                                                                                      \
        if (!dtw_ok(N, M, L, metric, window, subsequence))                                                                    \
            return fail(RBVAE_E_UNSUPPORTED,                                                                                  \
                        name ": (N=%d, M=%d, L=%d, metric=%d, window=%d, subsequence=%d) outside 1 <= N, M <= %d, "          \
                             "1 <= L <= %d, metric 0..2, window = -1 or |N - M| <= window without subsequence",              \
                        N, M, L, metric, window, subsequence, DTW_MAX_N, DTW_MAX_L);                                          \
    } while (0)

static int dtw_fill(const char* name, bool bits, const void* X, int N, const void* Y, int M, int L, int root, int window,
                    int sub, unsigned char* dirs, double* last_row, double* table, void* ws, hipStream_t st) {
    const int nTi = cdiv(N, DT_TI), nTj = cdiv(M, DT_TJ);
    double* frow = (double*)ws;
    double* fcol = frow + M;
    double* corner = fcol + N;
    int q = nTi + nTj;                                      // |ti - tj| <= q: every tile
    if (window >= 0) {
        if (window < DTW_MAX_N) q = (window + DT_TI - 1) / DT_TI;   // a tile with |ti - tj| > q lies wholly outside the band
        const long cells = table ? (long)N * M : (long)N * ((M + 3) >> 2);
        const int blocks = (int)(cells / 1024 < 1 ? 1 : cells / 1024 > 4096 ? 4096 : cells / 1024);
        hipLaunchKernelGGL(dtw_prefill_k, dim3(blocks), dim3(DT_THREADS), 0, st, N, M, dirs, last_row, table);
        if (hipGetLastError() != hipSuccess) return fail(RBVAE_E_LAUNCH, "%s (prefill): launch failed", name);
    }
    for (int d = 0; d < nTi + nTj - 1; ++d) {
        int lo = d - (nTj - 1) > 0 ? d - (nTj - 1) : 0, hi = d < nTi - 1 ? d : nTi - 1;
        if (d - q > 0 && (d - q + 1) / 2 > lo) lo = (d - q + 1) / 2;       // |2 ti - d| <= q
        if ((d + q) / 2 < hi) hi = (d + q) / 2;
        if (lo > hi) continue;
        if (bits)
            hipLaunchKernelGGL((dtw_tile_k<true, false>), dim3(hi - lo + 1), dim3(DT_THREADS), 0, st, X, Y, N, M, L, root, window, sub,
                               d, lo, nTj, frow, fcol, corner, dirs, last_row, table, (const long*)nullptr, DtwExt{});
        else
            hipLaunchKernelGGL((dtw_tile_k<false, false>), dim3(hi - lo + 1), dim3(DT_THREADS), 0, st, X, Y, N, M, L, root, window, sub,
                               d, lo, nTj, frow, fcol, corner, dirs, last_row, table, (const long*)nullptr, DtwExt{});
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fail(RBVAE_E_LAUNCH, "%s (tile anti-diagonal %d): %s", name, d, hipGetErrorString(e));
    }
    return RBVAE_OK;
}

// ---- many pairs ----------------------------------------------------------------------------------------------------------------

// One thread per path element k < len = state[0]: lo[i] where element k - 1 has another i, hi[i] where element k + 1 has.
// Every row has one first and one last element, so every lo[i] and hi[i] has one writer.  len < 1: nothing is written.
__global__ __launch_bounds__(DT_THREADS) void dtw_ranges_k(const int* __restrict__ path, const int* __restrict__ state, int n,
                                                           int m, int* __restrict__ lo, int* __restrict__ hi) {
    const int len = min(state[0], n + m - 1);
    const int k = blockIdx.x * DT_THREADS + threadIdx.x;
    if (k >= len) return;
    const int i = path[2 * (long)k], j = min(max(path[2 * (long)k + 1], 0), m - 1);
    if ((unsigned)i >= (unsigned)n) return;                 // not a path of this table
    if (k == 0 || path[2 * (long)(k - 1)] != i) lo[i] = j;
    if (k == len - 1 || path[2 * (long)(k + 1)] != i) hi[i] = j;
}

// One thread per (i, l), l fastest: acc in f64 over the pairs p ascending and the rows lo[p][i] .. hi[p][i] of pair p's Y
// sequence ascending, then one f64 division by the number of rows added and one rounding to f32.
__global__ __launch_bounds__(DT_THREADS) void dtw_bary_update_k(const float* __restrict__ Y, const long* __restrict__ plan,
                                                                DtwExt ext, int P, int L, int T, const int* __restrict__ lo,
                                                                const int* __restrict__ hi, float* __restrict__ out,
                                                                int* __restrict__ count) {
    const long g = (long)blockIdx.x * DT_THREADS + threadIdx.x;
    if (g >= (long)T * L) return;
    const int i = (int)(g / L), l = (int)(g - (long)i * L);
    double acc = 0.0;
    int cnt = 0;
    for (int p = 0; p < P; ++p) {
        const DtwPair q = dtw_pair(plan, p, ext);
        if (!q.ok) continue;
        const int a = min(max(lo[(long)p * T + i], 0), q.m - 1), b = min(max(hi[(long)p * T + i], 0), q.m - 1);
        const float* y = Y + (q.y0 + a) * L + l;
        for (int j = a; j <= b; ++j, y += L) acc += (double)*y;
        cnt += b >= a ? b - a + 1 : 0;
    }
    out[g] = (float)(acc / (double)cnt);
    if (l == 0) count[i] = cnt;
}

constexpr int DTW_MAX_P = 65535;                            // gridDim.y

static size_t dirs_block(long n, long m) { return ((size_t)n * ((m + 3) >> 2) + 15) & ~(size_t)15; }

// the host lengths and pairs against the limits -> NULL, or what is wrong
static const char* dtw_pairs_why(const int* len_x, long Sx, const int* len_y, long Sy, const int* pairs, long P, long L,
                                 int metric) {
    static thread_local char b[256];
    auto say = [&](const char* fmt, long a, long c) {
        snprintf(b, 256, fmt, a, c);
        return (const char*)b;
    };
    if (Sx < 1 || Sy < 1) return say("(Sx=%ld, Sy=%ld): every stack needs a sequence", Sx, Sy);
    if (P < 1 || P > DTW_MAX_P) return say("P=%ld outside 1 <= P <= %ld", P, DTW_MAX_P);
    if (L < 1 || L > DTW_MAX_L) return say("L=%ld outside 1 <= L <= %ld", L, DTW_MAX_L);
    if (metric < 0 || metric > 2) return say("metric=%ld outside 0 .. %ld", metric, 2);
    long tx = 0, ty = 0;
    for (long s = 0; s < Sx; ++s) {
        if (len_x[s] < 1 || len_x[s] > DTW_MAX_N) return say("len_x[%ld]=%ld outside 1 .. 16384", s, len_x[s]);
        tx += len_x[s];
    }
    for (long s = 0; s < Sy; ++s) {
        if (len_y[s] < 1 || len_y[s] > DTW_MAX_N) return say("len_y[%ld]=%ld outside 1 .. 16384", s, len_y[s]);
        ty += len_y[s];
    }
    if (tx > INT32_MAX || ty > INT32_MAX) return say("the stacks hold %ld and %ld rows, more than an int counts", tx, ty);
    for (long p = 0; p < P; ++p) {
        if (pairs[2 * p] < 0 || pairs[2 * p] >= Sx) return say("pairs[%ld][0]=%ld names no sequence of the X stack", p, pairs[2 * p]);
        if (pairs[2 * p + 1] < 0 || pairs[2 * p + 1] >= Sy)
            return say("pairs[%ld][1]=%ld names no sequence of the Y stack", p, pairs[2 * p + 1]);
    }
    return nullptr;
}

// the offsets of every pair's blocks, pair order, as the header states them; any of the outputs may be NULL
static void dtw_pairs_offsets(const int* len_x, const int* len_y, const int* pairs, int P, int64_t* dirs_off, int64_t* last_off,
                              int64_t* ws_off, int64_t* path_off) {
    int64_t d = 0, l = 0, w = 0, r = 0;
    for (int p = 0; p <= P; ++p) {
        if (dirs_off) dirs_off[p] = d;
        if (last_off) last_off[p] = l;
        if (ws_off) ws_off[p] = w;
        if (path_off) path_off[p] = r;
        if (p == P) break;
        const long n = len_x[pairs[2 * p]], m = len_y[pairs[2 * p + 1]];
        d += (int64_t)dirs_block(n, m);
        l += m;
        w += (int64_t)sizeof(double) * (n + m + (long)cdiv(n, DT_TI) * cdiv(m, DT_TJ));
        r += n + m - 1;
    }
}

static int dtw_pairs_fill(const char* name, bool bits, const void* X, int Nx, const void* Y, int Ny, int L, int metric,
                          const void* plan, int P, int n_diag, int max_tiles, unsigned char* dirs, size_t dirs_bytes,
                          double* last_row, size_t last_n, void* ws, size_t ws_bytes, hipStream_t st) {
    const int max_t = cdiv(DTW_MAX_N, DT_TI);
    if (Nx < 1 || Ny < 1 || L < 1 || L > DTW_MAX_L || metric < 0 || metric > 2 || P < 1 || P > DTW_MAX_P || n_diag < 1 ||
        n_diag > 2 * max_t - 1 || max_tiles < 1 || max_tiles > max_t)
        return fail(RBVAE_E_UNSUPPORTED,
                    "%s: (Nx=%d, Ny=%d, L=%d, metric=%d, P=%d, n_diag=%d, max_tiles=%d) outside 1 <= Nx, Ny, 1 <= L <= %d, "
                    "metric 0..2, 1 <= P <= %d, 1 <= n_diag <= %d, 1 <= max_tiles <= %d",
                    name, Nx, Ny, L, metric, P, n_diag, max_tiles, DTW_MAX_L, DTW_MAX_P, 2 * max_t - 1, max_t);
    if (!bits && metric == 2)
        return fail(RBVAE_E_UNSUPPORTED, "%s: metric=2 (hamming) takes packed codes: rbvae_dtw_pairs_fill_bits", name);
    RBVAE_CHECK_ARG(X && Y && plan && dirs && last_row && ws, "%s: null pointer", name);
    RBVAE_CHECK_ARG(dirs_bytes >= 1 && last_n >= 1 && ws_bytes >= sizeof(double), "%s: an output of no bytes", name);
    const DtwExt ext{Nx, Ny, (long)dirs_bytes, (long)last_n, (long)(ws_bytes / sizeof(double)), 0};
    double* w = (double*)ws;
    for (int d = 0; d < n_diag; ++d) {
        const dim3 grid(d + 1 < max_tiles ? d + 1 : max_tiles, P);      // no pair has more tiles on diagonal d
        if (bits)
            hipLaunchKernelGGL((dtw_tile_k<true, true>), grid, dim3(DT_THREADS), 0, st, X, Y, 0, 0, L, 0, -1, 0, d, 0, 0, w,
                               (double*)nullptr, (double*)nullptr, dirs, last_row, (double*)nullptr, (const long*)plan, ext);
        else
            hipLaunchKernelGGL((dtw_tile_k<false, true>), grid, dim3(DT_THREADS), 0, st, X, Y, 0, 0, L, metric == 1, -1, 0, d, 0,
                               0, w, (double*)nullptr, (double*)nullptr, dirs, last_row, (double*)nullptr, (const long*)plan, ext);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fail(RBVAE_E_LAUNCH, "%s (tile anti-diagonal %d): %s", name, d, hipGetErrorString(e));
    }
    return RBVAE_OK;
}

}  // namespace rbvae

using namespace rbvae;

extern "C" int rbvae_dtw_ok(int N, int M, int L, int metric, int window, int subsequence) {
    return dtw_ok(N, M, L, metric, window, subsequence) ? 1 : 0;
}

extern "C" int rbvae_dtw_tile_rows(void) { return DT_TI; }
extern "C" int rbvae_dtw_tile_cols(void) { return DT_TJ; }

extern "C" size_t rbvae_dtw_ws_bytes(int N, int M) {
    if (!dtw_ok(N, M, 1, 0, -1, 0)) return 0;
    return ((size_t)N + M + (size_t)cdiv(N, DT_TI) * cdiv(M, DT_TJ)) * sizeof(double);
}

extern "C" size_t rbvae_dtw_dirs_bytes(int N, int M) {
    if (!dtw_ok(N, M, 1, 0, -1, 0)) return 0;
    return (size_t)N * ((M + 3) >> 2);
}

extern "C" int rbvae_dtw_fill(const float* X, int N, const float* Y, int M, int L, int metric, int window, int subsequence,
                              unsigned char* dirs, double* last_row, double* table, void* ws, void* stream) {
    DTW_CHECK_SHAPE("dtw_fill");
    if (metric == 2)
        return fail(RBVAE_E_UNSUPPORTED, "dtw_fill: metric=2 (hamming) takes packed codes: rbvae_dtw_fill_bits");
    RBVAE_CHECK_ARG(X && Y && dirs && last_row && ws, "dtw_fill: null pointer");
    return dtw_fill("dtw_fill", false, X, N, Y, M, L, metric == 1, window, subsequence, dirs, last_row, table, ws,
                    (hipStream_t)stream);
}

extern "C" int rbvae_dtw_fill_bits(const uint32_t* xbits, int N, const uint32_t* ybits, int M, int L, int window,
                                   int subsequence, unsigned char* dirs, double* last_row, double* table, void* ws,
                                   void* stream) {
    const int metric = 2;
    DTW_CHECK_SHAPE("dtw_fill_bits");
    RBVAE_CHECK_ARG(xbits && ybits && dirs && last_row && ws, "dtw_fill_bits: null pointer");
    return dtw_fill("dtw_fill_bits", true, xbits, N, ybits, M, L, 0, window, subsequence, dirs, last_row, table, ws,
                    (hipStream_t)stream);
}

extern "C" int rbvae_dtw_trace(const unsigned char* dirs, const double* last_row, int N, int M, int subsequence, int* path,
                               int* state, double* cost, void* stream) {
    const int L = 1, metric = 0, window = -1;
    DTW_CHECK_SHAPE("dtw_trace");
    RBVAE_CHECK_ARG(dirs && last_row && path && state && cost, "dtw_trace: null pointer");
    RBVAE_CHECK_ARG(((uintptr_t)path & 7) == 0, "dtw_trace: path must be 8-byte aligned");
    hipLaunchKernelGGL(dtw_trace_k<false>, dim3(1), dim3(DT_THREADS), 0, (hipStream_t)stream, dirs, last_row, N, M, subsequence,
                       path, state, cost, (const long*)nullptr, DtwExt{});
    RBVAE_CHECK_LAUNCH("dtw_trace");
    return RBVAE_OK;
}

// ---- many pairs: two stacks and a pair list ---------------------------------------------------------------------------------------

#define DTW_CHECK_PAIRS(name)                                                                                                  \
    do {                                                                                                                      \
        RBVAE_CHECK_ARG(len_x && len_y && pairs, name ": null pointer");                                                      \
        if (const char* why = dtw_pairs_why(len_x, Sx, len_y, Sy, pairs, P, L, metric))                                       \
            return fail(RBVAE_E_UNSUPPORTED, name ": %s", why);                                                               \
    } while (0)

extern "C" int rbvae_dtw_pairs_ok(const int* len_x, int Sx, const int* len_y, int Sy, const int* pairs, int P, int L,
                                  int metric) {
    return len_x && len_y && pairs && !dtw_pairs_why(len_x, Sx, len_y, Sy, pairs, P, L, metric) ? 1 : 0;
}

extern "C" int rbvae_dtw_pairs_sizes(const int* len_x, int Sx, const int* len_y, int Sy, const int* pairs, int P,
                                     int64_t* dirs_off, int64_t* last_off, int64_t* ws_off, int64_t* path_off, size_t* totals) {
    const int L = 1, metric = 0;
    DTW_CHECK_PAIRS("dtw_pairs_sizes");
    RBVAE_CHECK_ARG(dirs_off && last_off && ws_off && path_off && totals, "dtw_pairs_sizes: null pointer");
    dtw_pairs_offsets(len_x, len_y, pairs, P, dirs_off, last_off, ws_off, path_off);
    totals[0] = (size_t)dirs_off[P], totals[1] = (size_t)last_off[P], totals[2] = (size_t)ws_off[P], totals[3] = (size_t)path_off[P];
    return RBVAE_OK;
}

extern "C" size_t rbvae_dtw_pairs_plan_bytes(int P) {
    if (P < 1 || P > DTW_MAX_P) return 0;
    return (DP_HDR + (size_t)P * DP_ROW) * sizeof(int64_t);
}

extern "C" int rbvae_dtw_pairs_plan(const int* len_x, int Sx, const int* len_y, int Sy, const int* pairs, int P, void* plan_dev,
                                    size_t plan_bytes, int* launch, void* stream) {
    const int L = 1, metric = 0;
    DTW_CHECK_PAIRS("dtw_pairs_plan");
    RBVAE_CHECK_ARG(plan_dev && launch, "dtw_pairs_plan: null pointer");
    const size_t need = rbvae_dtw_pairs_plan_bytes(P);
    RBVAE_CHECK_ARG(plan_bytes >= need, "dtw_pairs_plan: plan of %zu bytes, %zu needed", plan_bytes, need);
    std::vector<int64_t> row_x(Sx + 1, 0), row_y(Sy + 1, 0), off[4];
    for (int s = 0; s < Sx; ++s) row_x[s + 1] = row_x[s] + len_x[s];
    for (int s = 0; s < Sy; ++s) row_y[s + 1] = row_y[s] + len_y[s];
    for (auto& o : off) o.resize(P + 1);
    dtw_pairs_offsets(len_x, len_y, pairs, P, off[0].data(), off[1].data(), off[2].data(), off[3].data());
    std::vector<int64_t> h(need / sizeof(int64_t), 0);
    h[0] = P, h[1] = row_x[Sx], h[2] = row_y[Sy];
    int n_diag = 0, max_tiles = 0;
    for (int p = 0; p < P; ++p) {
        const int a = pairs[2 * p], b = pairs[2 * p + 1];
        const int nTi = cdiv(len_x[a], DT_TI), nTj = cdiv(len_y[b], DT_TJ);
        int64_t* r = h.data() + DP_HDR + (size_t)p * DP_ROW;
        r[DP_X0] = row_x[a], r[DP_Y0] = row_y[b], r[DP_N] = len_x[a], r[DP_M] = len_y[b], r[DP_NTI] = nTi, r[DP_NTJ] = nTj;
        r[DP_DIRS] = off[0][p], r[DP_LAST] = off[1][p], r[DP_WS] = off[2][p] / (int64_t)sizeof(double), r[DP_PATH] = off[3][p];
        n_diag = nTi + nTj - 1 > n_diag ? nTi + nTj - 1 : n_diag;
        max_tiles = (nTi < nTj ? nTi : nTj) > max_tiles ? (nTi < nTj ? nTi : nTj) : max_tiles;
    }
    // the host copy lives until the transfer has been taken: the stream is waited for (once per batch, not per launch)
    hipError_t err = hipMemcpyAsync(plan_dev, h.data(), need, hipMemcpyHostToDevice, (hipStream_t)stream);
    if (err == hipSuccess) err = hipStreamSynchronize((hipStream_t)stream);
    if (err != hipSuccess) return fail(RBVAE_E_LAUNCH, "dtw_pairs_plan: %s", hipGetErrorString(err));
    launch[0] = n_diag, launch[1] = max_tiles;
    return RBVAE_OK;
}

extern "C" int rbvae_dtw_pairs_fill(const float* X, int Nx, const float* Y, int Ny, int L, int metric, const void* plan, int P,
                                    int n_diag, int max_tiles, unsigned char* dirs, size_t dirs_bytes, double* last_row,
                                    size_t last_n, void* ws, size_t ws_bytes, void* stream) {
    return dtw_pairs_fill("dtw_pairs_fill", false, X, Nx, Y, Ny, L, metric, plan, P, n_diag, max_tiles, dirs, dirs_bytes, last_row,
                          last_n, ws, ws_bytes, (hipStream_t)stream);
}

extern "C" int rbvae_dtw_pairs_fill_bits(const uint32_t* xbits, int Nx, const uint32_t* ybits, int Ny, int L, const void* plan,
                                         int P, int n_diag, int max_tiles, unsigned char* dirs, size_t dirs_bytes,
                                         double* last_row, size_t last_n, void* ws, size_t ws_bytes, void* stream) {
    return dtw_pairs_fill("dtw_pairs_fill_bits", true, xbits, Nx, ybits, Ny, L, 2, plan, P, n_diag, max_tiles, dirs, dirs_bytes,
                          last_row, last_n, ws, ws_bytes, (hipStream_t)stream);
}

extern "C" int rbvae_dtw_pairs_trace(const unsigned char* dirs, size_t dirs_bytes, const double* last_row, size_t last_n,
                                     const void* plan, int P, int* path, size_t path_rows, int* state, double* cost,
                                     void* stream) {
    if (P < 1 || P > DTW_MAX_P) return fail(RBVAE_E_UNSUPPORTED, "dtw_pairs_trace: P=%d outside 1 <= P <= %d", P, DTW_MAX_P);
    RBVAE_CHECK_ARG(dirs && last_row && plan && path && state && cost, "dtw_pairs_trace: null pointer");
    RBVAE_CHECK_ARG(dirs_bytes >= 1 && last_n >= 1 && path_rows >= 1, "dtw_pairs_trace: an array of no bytes");
    RBVAE_CHECK_ARG(((uintptr_t)path & 7) == 0, "dtw_pairs_trace: path must be 8-byte aligned");
    const DtwExt ext{DTW_MAX_N, DTW_MAX_N, (long)dirs_bytes, (long)last_n, 0, (long)path_rows};
    hipLaunchKernelGGL(dtw_trace_k<true>, dim3(P), dim3(DT_THREADS), 0, (hipStream_t)stream, dirs, last_row, 0, 0, 0, path, state,
                       cost, (const long*)plan, ext);
    RBVAE_CHECK_LAUNCH("dtw_pairs_trace");
    return RBVAE_OK;
}

extern "C" int rbvae_dtw_path_ranges(const int* path, const int* state, int n, int m, int* lo, int* hi, void* stream) {
    if (!dtw_ok(n, m, 1, 0, -1, 0))
        return fail(RBVAE_E_UNSUPPORTED, "dtw_path_ranges: (n=%d, m=%d) outside 1 <= n, m <= %d", n, m, DTW_MAX_N);
    RBVAE_CHECK_ARG(path && state && lo && hi, "dtw_path_ranges: null pointer");
    hipLaunchKernelGGL(dtw_ranges_k, dim3(cdiv(n + m - 1, DT_THREADS)), dim3(DT_THREADS), 0, (hipStream_t)stream, path, state, n, m,
                       lo, hi);
    RBVAE_CHECK_LAUNCH("dtw_path_ranges");
    return RBVAE_OK;
}

extern "C" int rbvae_dtw_barycenter_update(const float* Y, int Ny, int L, const void* plan, int P, const int* lo, const int* hi,
                                           int T, float* out, int* count, void* stream) {
    if (Ny < 1 || L < 1 || L > DTW_MAX_L || P < 1 || P > DTW_MAX_P || T < 1 || T > DTW_MAX_N)
        return fail(RBVAE_E_UNSUPPORTED,
                    "dtw_barycenter_update: (Ny=%d, L=%d, P=%d, T=%d) outside 1 <= Ny, 1 <= L <= %d, 1 <= P <= %d, 1 <= T <= %d",
                    Ny, L, P, T, DTW_MAX_L, DTW_MAX_P, DTW_MAX_N);
    RBVAE_CHECK_ARG(Y && plan && lo && hi && out && count, "dtw_barycenter_update: null pointer");
    const DtwExt ext{T, Ny, 0, 0, 0, 0};
    hipLaunchKernelGGL(dtw_bary_update_k, dim3(cdiv((long)T * L, DT_THREADS)), dim3(DT_THREADS), 0, (hipStream_t)stream, Y,
                       (const long*)plan, ext, P, L, T, lo, hi, out, count);
    RBVAE_CHECK_LAUNCH("dtw_barycenter_update");
    return RBVAE_OK;
}
