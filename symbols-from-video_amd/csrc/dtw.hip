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
#include "common.h"
#include "pairdist.h"

#include <math.h>

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

// grid: the tiles ti_lo .. of tile anti-diagonal `diag`, tj = diag - ti.  metric 0 / 1: X, Y f32 [.][L]; BITS: uint32 [.][4]
template <bool BITS>
__global__ __launch_bounds__(DT_THREADS) void dtw_tile_k(const void* __restrict__ Xv, const void* __restrict__ Yv, int N, int M,
                                                         int L, int root, int window, int sub, int diag, int ti_lo, int nTj,
                                                         double* __restrict__ frow, double* __restrict__ fcol,
                                                         double* __restrict__ corner, unsigned char* __restrict__ dirs,
                                                         double* __restrict__ last_row, double* __restrict__ table) {
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

// state int32 [3] = {len, start_j, end_j}; len = -1 where dirs holds no walk from the end cell to row 0
__global__ __launch_bounds__(DT_THREADS) void dtw_trace_k(const unsigned char* __restrict__ dirs,
                                                          const double* __restrict__ last_row, int N, int M, int sub,
                                                          int* __restrict__ path, int* __restrict__ state,
                                                          double* __restrict__ cost) {
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
            hipLaunchKernelGGL(dtw_tile_k<true>, dim3(hi - lo + 1), dim3(DT_THREADS), 0, st, X, Y, N, M, L, root, window, sub, d,
                               lo, nTj, frow, fcol, corner, dirs, last_row, table);
        else
            hipLaunchKernelGGL(dtw_tile_k<false>, dim3(hi - lo + 1), dim3(DT_THREADS), 0, st, X, Y, N, M, L, root, window, sub,
                               d, lo, nTj, frow, fcol, corner, dirs, last_row, table);
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
    hipLaunchKernelGGL(dtw_trace_k, dim3(1), dim3(DT_THREADS), 0, (hipStream_t)stream, dirs, last_row, N, M, subsequence, path,
                       state, cost);
    RBVAE_CHECK_LAUNCH("dtw_trace");
    return RBVAE_OK;
}
