// Binarise + KL, pairwise-distance losses, MSE: the small f32 reductions of the RBVAE step.  All sums run in a fixed order
// (bitwise reproducible run to run).
//
// Kernels here promise equal bits to each other (contrast_term_fused_k / _bwd_k their gradients, the two binarise kernels y
// and z), so each repeated step has ONE definition, by the conventions of epilogue.h and lstm_steps.h (values and plain
// pointers in, a value or a small struct out, mode branches in the kernels, tools/isa_diff.py judges per kernel): bc_uniform,
// bc_noise, bin_code (common.h); grad_weight; hinge_coef; acc_store; rows_total / rows_mean; contrast_row; triplet_row;
// on the host kl_prior (common.h).  DESIGN.md section 4: which kernel takes which helper, and what stayed inline.
//
// Rounding: in both binarise kernels the compiler contracts  h + ratio * (log(u + e) - log(1 - u + e))  into one fma (the
// v_fmac_f32 after the two logs).  lstm_pair_fwd_k / lstm_pair_fwd_unit_k round the noise to f32 in LDS and add it on a
// later diagonal, so the two families' codes may differ by that one rounding.  Keep both: no explicit fmaf or rounding
// in bc_noise / bin_code, and no bit-equality test between a binarise launch and the pair launch.
#include "epilogue.h"

namespace rbvae {

thread_local char g_err[512] = {0};
char* err_buf() { return g_err; }
int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

constexpr int RED_THREADS = 1024;

// ---- the steps the kernels below repeat -------------------------------------------------------------------------------
// The binary-concrete uniform of element i: the caller's U[i], or (U == null) the 24-bit draw in [0,1) from the counter
// hash (device-side noise).  The staging prologues of the two LSTM pair forward kernels (lstm.hip) mirror this and bc_noise.
__device__ __forceinline__ float bc_uniform(const float* U, unsigned long long seed, int i) {
    return U ? U[i] : (float)(hash_u32(seed, (unsigned long long)i) >> 8) * (1.0f / 16777216.0f);
}
// The logistic noise term; bin_code's h + noise contracts with it into one fma (rounding note above)
__device__ __forceinline__ float bc_noise(float u, float ratio, float neps) {
    return ratio * (logf(u + neps) - logf(1.0f - u + neps));
}
// The weight of a gradient kernel: the upstream scale, times the optional device scalar gs[0]
__device__ __forceinline__ float grad_weight(float w, const float* gs) { return gs ? w * gs[0] : w; }
// Coefficient of (a - b + eps) in the gradient of w * max(margin - d, 0)^2, m = max(margin - d, 0), d = |a - b + eps|
__device__ __forceinline__ float hinge_coef(float w, float m, float d) { return (m > 0.f && d > 0.f) ? -2.f * w * m / d : 0.f; }
__device__ __forceinline__ void acc_store(float* p, float g, int accumulate) { *p = accumulate ? *p + g : g; }
// Tail of the single-workgroup forward kernels: lane 0 of every wave keeps the sum of the wave's rows, block sum, and (rows_mean)
// thread 0 writes the mean
__device__ __forceinline__ float rows_total(float acc, int lane, float* red) { return block_sum((lane == 0) ? acc : 0.f, red); }
__device__ __forceinline__ void rows_mean(float acc, int lane, float* red, float denom, float* out) {
    const float tot = rows_total(acc, lane, red);
    if (threadIdx.x == 0) out[0] = tot / denom;
}

__global__ __launch_bounds__(RED_THREADS) void binarize_kl_fwd_k(
    const float* __restrict__ h, const float* __restrict__ U, float* __restrict__ y_soft,
    float* __restrict__ z, float* __restrict__ kl_mean, int rows, int L, float tau, float ratio,
    float neps, int hard, float lp, float l1p, float keps, int clamp, unsigned long long seed,
    const unsigned long long* __restrict__ seed_dev) {
    __shared__ float red[RED_THREADS / 64];
    const int n = rows * L;
    float acc = 0.f;
    if (seed_dev) seed = epi_seed(seed, seed_dev);      // (guarded: without the if the listing changes)
    // batches of UB elements per thread: every global load of a batch is in flight before the first use (the
    // one-element-per-iteration loop paid a memory round trip per element: 8 of them at 256 x 32)
    constexpr int UB = 8;
    for (int base = threadIdx.x; base < n; base += UB * RED_THREADS) {
        float hv[UB], uv[UB];
#pragma unroll
        for (int b = 0; b < UB; ++b) {
            const int i = base + b * RED_THREADS, ic = i < n ? i : n - 1;
            hv[b] = h[ic];
            uv[b] = bc_uniform(U, seed, ic);
        }
#pragma unroll
        for (int b = 0; b < UB; ++b) {
            const int i = base + b * RED_THREADS;
            if (i >= n) break;
            const BinCode code = bin_code(hv[b], bc_noise(uv[b], ratio, neps), tau, hard);
            y_soft[i] = code.y;
            z[i] = code.z;
            if (kl_mean) acc += kl_elem(code.z, lp, l1p, keps, clamp);
        }
    }
    if (kl_mean) {
        const float tot = block_sum(acc, red);
        if (threadIdx.x == 0) kl_mean[0] = tot / (float)rows;
    }
}

// many-workgroup form: one element per thread, per-block partial KL sums (fixed order inside the block)
__global__ __launch_bounds__(256) void binarize_kl_fwd_parts_k(
    const float* __restrict__ h, const float* __restrict__ U, float* __restrict__ y_soft,
    float* __restrict__ z, float* __restrict__ kl_parts, int n, float tau, const float* __restrict__ tau_dev,
    float ratio, float neps, int hard, float lp, float l1p, float keps, int clamp, unsigned long long seed,
    const unsigned long long* __restrict__ seed_dev) {
    __shared__ float red[4];
    if (tau_dev) tau = tau_dev[0];
    const int i = blockIdx.x * 256 + threadIdx.x;
    float acc = 0.f;
    if (i < n) {
        if (seed_dev) seed = epi_seed(seed, seed_dev);
        const float noise = bc_noise(bc_uniform(U, seed, i), ratio, neps);
        const BinCode code = bin_code(h[i], noise, tau, hard);
        y_soft[i] = code.y;
        z[i] = code.z;
        if (kl_parts) acc = kl_elem(code.z, lp, l1p, keps, clamp);
    }
    if (kl_parts) {
        const float tot = block_sum(acc, red);
        if (threadIdx.x == 0) kl_parts[blockIdx.x] = tot;
    }
}

__global__ void binarize_kl_bwd_k(const float* __restrict__ g_z, const float* __restrict__ y_soft,
                                  const float* __restrict__ z, float* __restrict__ dh, int accumulate,
                                  int n, int rows, float tau, const float* __restrict__ tau_dev, float klw,
                                  const float* __restrict__ gs, float lp, float l1p, float keps, int clamp) {
    __builtin_amdgcn_s_setprio(3);               // sits between the two LSTM backward launches of the chain
    if (tau_dev) tau = tau_dev[0];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float w = grad_weight(klw / (float)rows, gs);
    float g = g_z ? g_z[i] : 0.f;
    if (w != 0.f) g += w * kl_elem_grad(z[i], lp, l1p, keps, clamp);
    const float y = y_soft[i];
    const float v = g * y * (1.0f - y) / tau;
    dh[i] = accumulate ? dh[i] + v : v;         // acc_store, typed out: the call adds an instruction to this listing
}

__global__ __launch_bounds__(RED_THREADS) void kl_fwd_k(const float* __restrict__ q, float* out, int rows,
                                                        int L, float lp, float l1p, float eps, int clamp) {
    __shared__ float red[RED_THREADS / 64];
    float acc = 0.f;
    for (int i = threadIdx.x; i < rows * L; i += RED_THREADS) acc += kl_elem(q[i], lp, l1p, eps, clamp);
    const float tot = block_sum(acc, red);
    if (threadIdx.x == 0) out[0] = tot / (float)rows;
}

__global__ void kl_bwd_k(const float* __restrict__ q, float* __restrict__ dq, int n, int rows, float lp,
                         float l1p, float eps, int clamp, float scale, const float* __restrict__ gs) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float w = grad_weight(scale / (float)rows, gs);
    dq[i] = w * kl_elem_grad(q[i], lp, l1p, eps, clamp);
}

// One wave per row: sum_L (a - b + eps)^2 with a lane-strided loop + shuffle reduce.
__device__ __forceinline__ float row_sqdist(const float* a, const float* b, int L, float eps, int lane) {
    float s = 0.f;
    for (int k = lane; k < L; k += 64) {
        const float d = a[k] - b[k] + eps;
        s += d * d;
    }
    return wave_sum(s);
}

__global__ __launch_bounds__(RED_THREADS) void pairdist_fwd_k(
    const float* __restrict__ x1, const float* __restrict__ x2, long s1, long s2, int rows, int L,
    int label, float margin, float eps, float* out) {
    __shared__ float red[RED_THREADS / 64];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    float acc = 0.f;
    for (int r = wid; r < rows; r += RED_THREADS / 64) {
        const float d = sqrtf(row_sqdist(x1 + r * s1, x2 + r * s2, L, eps, lane));
        const float m = fmaxf(margin - d, 0.f);
        acc += label ? m * m : d * d;
    }
    rows_mean(acc, lane, red, (float)rows, out);
}

// dx1 = w * dloss/dx1 for one row; dx2 = -dx1.
__global__ void pairdist_bwd_k(const float* __restrict__ x1, const float* __restrict__ x2, long s1, long s2,
                               int rows, int L, int label, float margin, float eps, float scale,
                               const float* __restrict__ gs, float* dx1, float* dx2, long ds1, long ds2,
                               int accumulate) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float* a = x1 + r * s1;
    const float* b = x2 + r * s2;
    const float w = grad_weight(scale / (float)rows, gs);
    float coef;
    if (label == 0) {
        coef = 2.f * w;                        // d(d^2)/da = 2 (a - b + eps)
    } else {
        const float d = sqrtf(row_sqdist(a, b, L, eps, lane));
        const float m = fmaxf(margin - d, 0.f);
        coef = hinge_coef(w, m, d);
    }
    for (int k = lane; k < L; k += 64) {
        const float g = coef * (a[k] - b[k] + eps);
        if (dx1) acc_store(dx1 + r * ds1 + k, g, accumulate);
        if (dx2) acc_store(dx2 + r * ds2 + k, -g, accumulate);
    }
}

// ---- contrast_loss, 'cosine' branch (percep_RBVAE_train.py:94-96): dist = 1 - cosine_similarity(x1, x2) ----------
// torch.nn.functional.cosine_similarity: x1.x2 / (max(|x1|, eps) * max(|x2|, eps)), eps 1e-8.  One wave per row.
__device__ __forceinline__ void row_cos(const float* a, const float* b, int L, int lane, float& dot, float& na, float& nb) {
    float d = 0.f, sa = 0.f, sb = 0.f;
    for (int k = lane; k < L; k += 64) {
        d += a[k] * b[k];
        sa += a[k] * a[k];
        sb += b[k] * b[k];
    }
    dot = wave_sum(d);
    na = sqrtf(wave_sum(sa));
    nb = sqrtf(wave_sum(sb));
}

__global__ __launch_bounds__(RED_THREADS) void paircos_fwd_k(const float* __restrict__ x1, const float* __restrict__ x2,
                                                             long s1, long s2, int rows, int L, int label, float margin,
                                                             float eps, float* out) {
    __shared__ float red[RED_THREADS / 64];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    float acc = 0.f;
    for (int r = wid; r < rows; r += RED_THREADS / 64) {
        float dot, na, nb;
        row_cos(x1 + r * s1, x2 + r * s2, L, lane, dot, na, nb);
        const float d = 1.f - dot / (fmaxf(na, eps) * fmaxf(nb, eps));
        const float m = fmaxf(margin - d, 0.f);
        acc += label ? m * m : d * d;
    }
    rows_mean(acc, lane, red, (float)rows, out);
}

__global__ void paircos_bwd_k(const float* __restrict__ x1, const float* __restrict__ x2, long s1, long s2, int rows, int L,
                              int label, float margin, float eps, float scale, const float* __restrict__ gs, float* dx1,
                              float* dx2, long ds1, long ds2) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float* a = x1 + r * s1;
    const float* b = x2 + r * s2;
    float dot, na, nb;
    row_cos(a, b, L, lane, dot, na, nb);
    const float ca = fmaxf(na, eps), cb = fmaxf(nb, eps);
    const float cs = dot / (ca * cb), d = 1.f - cs;
    const float w = grad_weight(scale / (float)rows, gs);
    // dloss/dcos: label 0: d(d^2) = -2 d;  label 1: d(max(m - d, 0)^2) = +2 max(m - d, 0)
    const float g = label ? 2.f * w * fmaxf(margin - d, 0.f) : -2.f * w * d;
    // dcos/da = b / (ca cb) - [na > eps] cos a / na^2   (the clamped norm is a constant below eps)
    const float ia = na > eps ? cs / (na * na) : 0.f, ib = nb > eps ? cs / (nb * nb) : 0.f;
    const float inv = 1.f / (ca * cb);
    for (int k = lane; k < L; k += 64) {
        if (dx1) dx1[r * ds1 + k] = g * (b[k] * inv - ia * a[k]);
        if (dx2) dx2[r * ds2 + k] = g * (a[k] * inv - ib * b[k]);
    }
}

// ---- trainer's contrastive term, one launch --------------------------------
__global__ __launch_bounds__(RED_THREADS) void contrast_term_fwd_k(const float* __restrict__ h0,
                                                                   const float* __restrict__ h1, int B, int T,
                                                                   int L, float* out) {
    __shared__ float red[RED_THREADS / 64];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const float eps = 1e-6f;
    float sim = 0.f, dis = 0.f;
    for (int r = wid; r < B * T; r += RED_THREADS / 64) {
        const float d = sqrtf(row_sqdist(h0 + (long)r * L, h1 + (long)r * L, L, eps, lane));
        sim += d * d;
        const int t = r % T;
        if (t < T - 1) {
            const float d2 = sqrtf(row_sqdist(h0 + (long)r * L, h0 + (long)(r + 1) * L, L, eps, lane));
            const float m = fmaxf(1.0f - d2, 0.f);
            dis += m * m;
        }
    }
    const float ts = rows_total(sim, lane, red);
    const float td = rows_total(dis, lane, red);
    if (threadIdx.x == 0) out[0] = ts / (float)(B * T) + td / ((float)B * (float)(T - 1));
}

// One wave per (b, t) row r of h0 / h1: the row's gradients, and its two forward values.  Row t of h0 takes the similar
// term, the dissimilar pair (t, t+1) as first operand and the pair (t-1, t) as second.  sim = d(h0, h1)^2; dis =
// max(1 - d(h0[t], h0[t+1]), 0)^2 (0 for the last state of a sequence).
struct ContrastRow { float sim, dis; };
__device__ __forceinline__ ContrastRow contrast_row(const float* h0, const float* h1, int r, int B, int T, int L,
                                                    float scale, const float* gs, int lane, float* dh0, float* dh1) {
    const float eps = 1e-6f;
    const float w = grad_weight(scale, gs);
    const float wsim = 2.f * w / (float)(B * T);
    const float wdis = w / ((float)B * (float)(T - 1));
    const int t = r % T;
    const float* a = h0 + (long)r * L;
    const float* b = h1 + (long)r * L;
    const float d = sqrtf(row_sqdist(a, b, L, eps, lane));
    ContrastRow v = {d * d, 0.f};
    float cn = 0.f, cp = 0.f;   // coefficients of the (t,t+1) and (t-1,t) pairs
    if (t < T - 1) {
        const float d2 = sqrtf(row_sqdist(a, a + L, L, eps, lane));
        const float m = fmaxf(1.0f - d2, 0.f);
        v.dis = m * m;
        cn = hinge_coef(wdis, m, d2);
    }
    if (t > 0) {
        const float d2 = sqrtf(row_sqdist(a - L, a, L, eps, lane));
        cp = hinge_coef(wdis, fmaxf(1.0f - d2, 0.f), d2);
    }
    for (int k = lane; k < L; k += 64) {
        const float gsim = wsim * (a[k] - b[k] + eps);
        float g0 = gsim;
        if (t < T - 1) g0 += cn * (a[k] - a[k + L] + eps);
        if (t > 0) g0 -= cp * (a[k - L] - a[k] + eps);
        dh0[(long)r * L + k] = g0;
        dh1[(long)r * L + k] = -gsim;
    }
    return v;
}

__global__ void contrast_term_bwd_k(const float* __restrict__ h0, const float* __restrict__ h1, int B, int T,
                                    int L, float scale, const float* __restrict__ gs, float* __restrict__ dh0,
                                    float* __restrict__ dh1) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= B * T) return;
    contrast_row(h0, h1, r, B, T, L, scale, gs, lane, dh0, dh1);      // the forward values go unused
}

// Forward value (as per-block partial sums) and gradient of the contrastive term in ONE many-workgroup launch: the same
// row as contrast_term_bwd_k, plus the partial sums.  parts[2*block] = sum of d(h0,h1)^2 over the block's rows,
// parts[2*block+1] = sum of max(1 - d(h0[t], h0[t+1]), 0)^2; rbvae_combine_losses finishes  sum0/(B*T) + sum1/(B*(T-1)).
// The two-launch form above runs its forward in a single workgroup (10-12 us); this one is ~4 us and needs no side stream.
__global__ __launch_bounds__(256) void contrast_term_fused_k(const float* __restrict__ h0, const float* __restrict__ h1,
                                                             int B, int T, int L, float scale,
                                                             const float* __restrict__ gs, float* __restrict__ parts,
                                                             float* __restrict__ dh0, float* __restrict__ dh1) {
    __shared__ float red[4][2];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int r = blockIdx.x * 4 + wid;
    ContrastRow v = {0.f, 0.f};
    if (r < B * T) v = contrast_row(h0, h1, r, B, T, L, scale, gs, lane, dh0, dh1);
    if (lane == 0) { red[wid][0] = v.sim; red[wid][1] = v.dis; }
    __syncthreads();
    if (threadIdx.x < 2)
        parts[2 * blockIdx.x + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// ---- triplet ---------------------------------------------------------------
// One triplet row (one wave per row): the distances d(a,p), d(a,n) and, with swap, d(p,n); which negative the loss takes
// (torch.minimum sends the gradient to the smaller one, and half to each at a tie: exact whenever a and p are bitwise
// equal views); and the row's loss max(margin + d(a,p) - min(d(a,n), d(p,n)), 0).  triplet_fwd_k takes the loss
// (triplet_term_fwd_k mirrors it, typed out), triplet_row_bwd the rest.
struct TripletRow { float dap, dan, dpn, loss; bool use_pn, tie; };
__device__ __forceinline__ TripletRow triplet_row(const float* a, const float* p, const float* n, int L, float margin,
                                                  float eps, int swap, int lane) {
    TripletRow t = {sqrtf(row_sqdist(a, p, L, eps, lane)), sqrtf(row_sqdist(a, n, L, eps, lane)), 0.f, 0.f, false, false};
    float dneg = t.dan;
    if (swap) {
        t.dpn = sqrtf(row_sqdist(p, n, L, eps, lane));
        t.use_pn = t.dpn < t.dan;
        t.tie = t.dpn == t.dan;
        dneg = fminf(dneg, t.dpn);
    }
    t.loss = fmaxf(margin + t.dap - dneg, 0.f);
    return t;
}

__global__ __launch_bounds__(RED_THREADS) void triplet_fwd_k(
    const float* __restrict__ a, const float* __restrict__ p, const float* __restrict__ n, long sa, long sp,
    long sn, int rows, int L, float margin, float eps, int swap, float* out) {
    __shared__ float red[RED_THREADS / 64];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    float acc = 0.f;
    for (int r = wid; r < rows; r += RED_THREADS / 64)
        acc += triplet_row(a + r * sa, p + r * sp, n + r * sn, L, margin, eps, swap, lane).loss;
    rows_mean(acc, lane, red, (float)rows, out);
}

// grads of mean_r max(margin + d(a,p) - min(d(a,n), d(p,n)), 0) for one row per wave
__device__ __forceinline__ void triplet_row_bwd(const float* a, const float* p, const float* n, int L,
                                                float margin, float eps, int swap, float w, int lane,
                                                float* da, float* dp, float* dn, int accumulate) {
    const TripletRow t = triplet_row(a, p, n, L, margin, eps, swap, lane);
    const float dneg = t.use_pn ? t.dpn : t.dan;
    const bool active = (margin + t.dap - dneg) > 0.f;
    const float cap = (active && t.dap > 0.f) ? w / t.dap : 0.f;
    const float cng = (active && dneg > 0.f) ? -w / dneg : 0.f;
    for (int k = lane; k < L; k += 64) {
        const float gap = cap * (a[k] - p[k] + eps);           // d dap: +a, -p
        float ga = gap, gp = -gap, gn = 0.f;
        if (t.tie) {
            const float g1 = 0.5f * (cng * (a[k] - n[k] + eps)), g2 = 0.5f * (cng * (p[k] - n[k] + eps));
            ga += g1; gp += g2; gn = -g1 - g2;
        }
        else if (t.use_pn) { const float g = cng * (p[k] - n[k] + eps); gp += g; gn -= g; }
        else               { const float g = cng * (a[k] - n[k] + eps); ga += g; gn -= g; }
        if (da) acc_store(da + k, ga, accumulate);
        if (dp) acc_store(dp + k, gp, accumulate);
        if (dn) acc_store(dn + k, gn, accumulate);
    }
}

__global__ void triplet_bwd_k(const float* __restrict__ a, const float* __restrict__ p,
                              const float* __restrict__ n, long sa, long sp, long sn, int rows, int L,
                              float margin, float eps, int swap, float scale, const float* __restrict__ gs,
                              float* da, float* dp, float* dn, long dsa, long dsp, long dsn, int accumulate) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float w = grad_weight(scale / (float)rows, gs);
    triplet_row_bwd(a + r * sa, p + r * sp, n + r * sn, L, margin, eps, swap, w, lane,
                    da ? da + r * dsa : nullptr, dp ? dp + r * dsp : nullptr, dn ? dn + r * dsn : nullptr,
                    accumulate);
}

__global__ __launch_bounds__(RED_THREADS) void triplet_term_fwd_k(const float* __restrict__ h0,
                                                                  const float* __restrict__ h1, int B, int T,
                                                                  int L, float margin, float* out) {
    __shared__ float red[RED_THREADS / 64];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const float eps = 1e-8f;
    float acc = 0.f;
    for (int r = wid; r < B * T; r += RED_THREADS / 64) {
        if (r % T == T - 1) continue;
        // triplet_row(a, p, n, .., swap = 1).loss and, below, rows_mean, typed out: with either helper this listing changes,
        // and with triplet_row the launch measured 0.2 us slower; keep them alike
        const float* a = h0 + (long)r * L;
        const float* p = h1 + (long)r * L;
        const float* n = a + L;
        const float dap = sqrtf(row_sqdist(a, p, L, eps, lane));
        const float dan = fminf(sqrtf(row_sqdist(a, n, L, eps, lane)), sqrtf(row_sqdist(p, n, L, eps, lane)));
        acc += fmaxf(margin + dap - dan, 0.f);
    }
    acc = (lane == 0) ? acc : 0.f;
    const float tot = block_sum(acc, red);
    if (threadIdx.x == 0) out[0] = tot / ((float)B * (float)(T - 1));
}

// One block per sequence b; the T-1 triplets of a sequence touch overlapping rows,
// so a single wave walks them in order (T <= 17: negligible work).
__global__ void triplet_term_bwd_k(const float* __restrict__ h0, const float* __restrict__ h1, int B, int T,
                                   int L, float margin, float scale, const float* __restrict__ gs,
                                   float* __restrict__ dh0, float* __restrict__ dh1) {
    const int lane = threadIdx.x;
    const int b = blockIdx.x;
    const float w = grad_weight(scale / ((float)B * (float)(T - 1)), gs);
    for (int t = 0; t < T; ++t)
        for (int k = lane; k < L; k += 64) {
            dh0[((long)b * T + t) * L + k] = 0.f;
            dh1[((long)b * T + t) * L + k] = 0.f;
        }
    for (int s = 0; s < T - 1; ++s) {
        const long o = ((long)b * T + s) * L;
        triplet_row_bwd(h0 + o, h1 + o, h0 + o + L, L, margin, 1e-8f, 1, w, lane, dh0 + o, dh1 + o,
                        dh0 + o + L, 1);
    }
}

// ---- MSE -------------------------------------------------------------------
constexpr int MSE_BLOCKS = 512;
__global__ __launch_bounds__(256) void mse_partial_k(const float* __restrict__ a, const float* __restrict__ b,
                                                     long n, float* __restrict__ ws) {
    __shared__ float red[4];
    float acc = 0.f;
    const long n4 = n >> 2;
    const float4* a4 = reinterpret_cast<const float4*>(a);
    const float4* b4 = reinterpret_cast<const float4*>(b);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const float4 x = a4[i], y = b4[i];
        const float d0 = x.x - y.x, d1 = x.y - y.y, d2 = x.z - y.z, d3 = x.w - y.w;
        acc += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
    }
    if (blockIdx.x == 0)
        for (long i = (n4 << 2) + threadIdx.x; i < n; i += 256) { const float d = a[i] - b[i]; acc += d * d; }
    const float tot = block_sum(acc, red);
    if (threadIdx.x == 0) ws[blockIdx.x] = tot;
}
__global__ __launch_bounds__(MSE_BLOCKS) void mse_final_k(const float* __restrict__ ws, int nb, long n,
                                                          float* out) {
    __shared__ float red[MSE_BLOCKS / 64];
    const float v = (int)threadIdx.x < nb ? ws[threadIdx.x] : 0.f;
    const float tot = block_sum(v, red);
    if (threadIdx.x == 0) out[0] = tot / (float)n;
}
__global__ void mse_bwd_k(const float* __restrict__ a, const float* __restrict__ b, long n, float scale,
                          const float* __restrict__ gs, float* __restrict__ da) {
    const float w = grad_weight(2.f * scale / (float)n, gs);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        da[i] = w * (a[i] - b[i]);
}

}  // namespace rbvae

using namespace rbvae;

extern "C" {

int rbvae_version(void) { return 111; }

__global__ void counter_add_k(unsigned long long* c, unsigned long long inc) { c[0] += inc; }
int rbvae_counter_add(unsigned long long* counter, unsigned long long inc, void* stream) {
    RBVAE_CHECK_ARG(counter, "counter_add: null pointer");
    hipLaunchKernelGGL(counter_add_k, dim3(1), dim3(1), 0, (hipStream_t)stream, counter, inc);
    RBVAE_CHECK_LAUNCH("counter_add");
    return RBVAE_OK;
}
const char* rbvae_last_error(void) { return err_buf(); }

int rbvae_binarize_kl_fwd(const float* h, const float* U, float* y_soft, float* z, float* kl_mean, int rows,
                          int L, float tau, float noise_ratio, float noise_eps, int hard, float kl_p,
                          float kl_eps, int kl_clamp, unsigned long long seed, const unsigned long long* seed_dev,
                          void* stream) {
    RBVAE_CHECK_ARG(h && y_soft && z, "binarize_kl_fwd: null pointer");
    RBVAE_CHECK_ARG(rows > 0 && L > 0 && tau > 0.f, "binarize_kl_fwd: rows=%d L=%d tau=%g", rows, L, tau);
    KlPrior kp;                                  // (p is checked with or without kl_mean, as it always was here)
    RBVAE_CHECK_ARG(kl_prior(true, kl_p, &kp), "binarize_kl_fwd: p=%g outside (0,1)", kl_p);
    hipLaunchKernelGGL(binarize_kl_fwd_k, dim3(1), dim3(RED_THREADS), 0, (hipStream_t)stream, h, U, y_soft, z,
                       kl_mean, rows, L, tau, noise_ratio, noise_eps, hard, kp.lp, kp.l1p, kl_eps, kl_clamp, seed,
                       seed_dev);
    RBVAE_CHECK_LAUNCH("binarize_kl_fwd");
    return RBVAE_OK;
}

int rbvae_binarize_kl_nparts(int rows, int L) { return cdiv((long)rows * L, 256); }

int rbvae_binarize_kl_fwd_parts(const float* h, const float* U, float* y_soft, float* z, float* kl_parts, int rows,
                                int L, float tau, const float* tau_dev, float noise_ratio, float noise_eps, int hard,
                                float kl_p, float kl_eps, int kl_clamp, unsigned long long seed,
                                const unsigned long long* seed_dev, void* stream) {
    RBVAE_CHECK_ARG(h && y_soft && z, "binarize_kl_fwd_parts: null pointer");
    RBVAE_CHECK_ARG(rows > 0 && L > 0 && (tau_dev || tau > 0.f), "binarize_kl_fwd_parts: rows=%d L=%d tau=%g", rows, L, tau);
    KlPrior kp;
    RBVAE_CHECK_ARG(kl_prior(kl_parts != nullptr, kl_p, &kp), "binarize_kl_fwd_parts: kl_p=%g outside (0,1)", kl_p);
    const int n = rows * L;
    hipLaunchKernelGGL(binarize_kl_fwd_parts_k, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, h, U, y_soft, z,
                       kl_parts, n, tau, tau_dev, noise_ratio, noise_eps, hard, kp.lp, kp.l1p, kl_eps, kl_clamp, seed,
                       seed_dev);
    RBVAE_CHECK_LAUNCH("binarize_kl_fwd_parts");
    return RBVAE_OK;
}

int rbvae_binarize_kl_bwd(const float* g_z, const float* y_soft, const float* z, float* dh, int accumulate,
                          int rows, int L, float tau, const float* tau_dev, float kl_weight, const float* gscale_dev,
                          float kl_p, float kl_eps, int kl_clamp, void* stream) {
    RBVAE_CHECK_ARG(y_soft && z && dh, "binarize_kl_bwd: null pointer");
    RBVAE_CHECK_ARG(rows > 0 && L > 0 && (tau_dev || tau > 0.f), "binarize_kl_bwd: rows=%d L=%d tau=%g", rows, L, tau);
    // log(1 - p) of p = 1 would put an infinite gradient into dh silently; weight 0 skips the KL term (and its p)
    KlPrior kp;
    RBVAE_CHECK_ARG(kl_prior(kl_weight != 0.f, kl_p, &kp), "binarize_kl_bwd: p=%g outside (0,1)", kl_p);
    const int n = rows * L;
    hipLaunchKernelGGL(binarize_kl_bwd_k, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, g_z, y_soft, z,
                       dh, accumulate, n, rows, tau, tau_dev, kl_weight, gscale_dev, kp.lp, kp.l1p, kl_eps, kl_clamp);
    RBVAE_CHECK_LAUNCH("binarize_kl_bwd");
    return RBVAE_OK;
}

int rbvae_kl_fwd(const float* q, float* out, int rows, int L, float p, float eps, int clamp, void* stream) {
    RBVAE_CHECK_ARG(q && out && rows > 0 && L > 0, "kl_fwd: bad arguments");
    KlPrior kp;
    RBVAE_CHECK_ARG(kl_prior(true, p, &kp), "kl_fwd: p=%g outside (0,1)", p);
    hipLaunchKernelGGL(kl_fwd_k, dim3(1), dim3(RED_THREADS), 0, (hipStream_t)stream, q, out, rows, L, kp.lp, kp.l1p,
                       eps, clamp);
    RBVAE_CHECK_LAUNCH("kl_fwd");
    return RBVAE_OK;
}

int rbvae_kl_bwd(const float* q, float* dq, int rows, int L, float p, float eps, int clamp, float scale,
                 const float* gscale_dev, void* stream) {
    RBVAE_CHECK_ARG(q && dq && rows > 0 && L > 0, "kl_bwd: bad arguments");
    KlPrior kp;
    RBVAE_CHECK_ARG(kl_prior(true, p, &kp), "kl_bwd: p=%g outside (0,1)", p);
    const int n = rows * L;
    hipLaunchKernelGGL(kl_bwd_k, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, q, dq, n, rows, kp.lp, kp.l1p,
                       eps, clamp, scale, gscale_dev);
    RBVAE_CHECK_LAUNCH("kl_bwd");
    return RBVAE_OK;
}

int rbvae_pairdist_fwd(const float* x1, const float* x2, long s1, long s2, int rows, int L, int label,
                       float margin, float eps, float* out, void* stream) {
    RBVAE_CHECK_ARG(x1 && x2 && out && rows > 0 && L > 0, "pairdist_fwd: bad arguments");
    hipLaunchKernelGGL(pairdist_fwd_k, dim3(1), dim3(RED_THREADS), 0, (hipStream_t)stream, x1, x2, s1, s2, rows,
                       L, label, margin, eps, out);
    RBVAE_CHECK_LAUNCH("pairdist_fwd");
    return RBVAE_OK;
}

int rbvae_pairdist_bwd(const float* x1, const float* x2, long s1, long s2, int rows, int L, int label,
                       float margin, float eps, float scale, const float* gscale_dev, float* dx1, float* dx2,
                       long ds1, long ds2, int accumulate, void* stream) {
    RBVAE_CHECK_ARG(x1 && x2 && rows > 0 && L > 0, "pairdist_bwd: bad arguments");
    hipLaunchKernelGGL(pairdist_bwd_k, dim3(cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, x1, x2, s1, s2,
                       rows, L, label, margin, eps, scale, gscale_dev, dx1, dx2, ds1, ds2, accumulate);
    RBVAE_CHECK_LAUNCH("pairdist_bwd");
    return RBVAE_OK;
}

int rbvae_paircos_fwd(const float* x1, const float* x2, long s1, long s2, int rows, int L, int label, float margin,
                      float eps, float* out, void* stream) {
    RBVAE_CHECK_ARG(x1 && x2 && out && rows > 0 && L > 0, "paircos_fwd: bad arguments");
    hipLaunchKernelGGL(paircos_fwd_k, dim3(1), dim3(RED_THREADS), 0, (hipStream_t)stream, x1, x2, s1, s2, rows, L, label,
                       margin, eps, out);
    RBVAE_CHECK_LAUNCH("paircos_fwd");
    return RBVAE_OK;
}

int rbvae_paircos_bwd(const float* x1, const float* x2, long s1, long s2, int rows, int L, int label, float margin,
                      float eps, float scale, const float* gscale_dev, float* dx1, float* dx2, long ds1, long ds2,
                      void* stream) {
    RBVAE_CHECK_ARG(x1 && x2 && rows > 0 && L > 0, "paircos_bwd: bad arguments");
    hipLaunchKernelGGL(paircos_bwd_k, dim3(cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, x1, x2, s1, s2, rows, L,
                       label, margin, eps, scale, gscale_dev, dx1, dx2, ds1, ds2);
    RBVAE_CHECK_LAUNCH("paircos_bwd");
    return RBVAE_OK;
}

int rbvae_contrast_term_fwd(const float* h0, const float* h1, int B, int T, int L, float* out, void* stream) {
    RBVAE_CHECK_ARG(h0 && h1 && out && B > 0 && L > 0, "contrast_term_fwd: bad arguments");
    RBVAE_CHECK_ARG(T >= 2, "contrast_term_fwd: needs T >= 2 states (got %d)", T);
    hipLaunchKernelGGL(contrast_term_fwd_k, dim3(1), dim3(RED_THREADS), 0, (hipStream_t)stream, h0, h1, B, T, L,
                       out);
    RBVAE_CHECK_LAUNCH("contrast_term_fwd");
    return RBVAE_OK;
}

int rbvae_contrast_term_bwd(const float* h0, const float* h1, int B, int T, int L, float scale,
                            const float* gscale_dev, float* dh0, float* dh1, void* stream) {
    RBVAE_CHECK_ARG(h0 && h1 && dh0 && dh1 && B > 0 && L > 0, "contrast_term_bwd: bad arguments");
    RBVAE_CHECK_ARG(T >= 2, "contrast_term_bwd: needs T >= 2 states (got %d)", T);
    hipLaunchKernelGGL(contrast_term_bwd_k, dim3(cdiv(B * T, 4)), dim3(256), 0, (hipStream_t)stream, h0, h1, B,
                       T, L, scale, gscale_dev, dh0, dh1);
    RBVAE_CHECK_LAUNCH("contrast_term_bwd");
    return RBVAE_OK;
}

int rbvae_contrast_term_nparts(int B, int T) { return cdiv((long)B * T, 4); }

int rbvae_contrast_term_fused(const float* h0, const float* h1, int B, int T, int L, float scale,
                              const float* gscale_dev, float* parts, float* dh0, float* dh1, void* stream) {
    RBVAE_CHECK_ARG(h0 && h1 && parts && dh0 && dh1 && B > 0 && L > 0, "contrast_term_fused: bad arguments");
    RBVAE_CHECK_ARG(T >= 2, "contrast_term_fused: needs T >= 2 states (got %d)", T);
    hipLaunchKernelGGL(contrast_term_fused_k, dim3(cdiv(B * T, 4)), dim3(256), 0, (hipStream_t)stream, h0, h1, B, T, L,
                       scale, gscale_dev, parts, dh0, dh1);
    RBVAE_CHECK_LAUNCH("contrast_term_fused");
    return RBVAE_OK;
}

int rbvae_triplet_fwd(const float* a, const float* p, const float* n, long sa, long sp, long sn, int rows, int L,
                      float margin, float eps, int swap, float* out, void* stream) {
    RBVAE_CHECK_ARG(a && p && n && out && rows > 0 && L > 0, "triplet_fwd: bad arguments");
    hipLaunchKernelGGL(triplet_fwd_k, dim3(1), dim3(RED_THREADS), 0, (hipStream_t)stream, a, p, n, sa, sp, sn,
                       rows, L, margin, eps, swap, out);
    RBVAE_CHECK_LAUNCH("triplet_fwd");
    return RBVAE_OK;
}

int rbvae_triplet_bwd(const float* a, const float* p, const float* n, long sa, long sp, long sn, int rows, int L,
                      float margin, float eps, int swap, float scale, const float* gscale_dev, float* da,
                      float* dp, float* dn, long dsa, long dsp, long dsn, int accumulate, void* stream) {
    RBVAE_CHECK_ARG(a && p && n && rows > 0 && L > 0, "triplet_bwd: bad arguments");
    hipLaunchKernelGGL(triplet_bwd_k, dim3(cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, a, p, n, sa, sp,
                       sn, rows, L, margin, eps, swap, scale, gscale_dev, da, dp, dn, dsa, dsp, dsn, accumulate);
    RBVAE_CHECK_LAUNCH("triplet_bwd");
    return RBVAE_OK;
}

int rbvae_triplet_term_fwd(const float* h0, const float* h1, int B, int T, int L, float margin, float* out,
                           void* stream) {
    RBVAE_CHECK_ARG(h0 && h1 && out && B > 0 && L > 0, "triplet_term_fwd: bad arguments");
    RBVAE_CHECK_ARG(T >= 2, "triplet_term_fwd: needs T >= 2 states (got %d)", T);
    hipLaunchKernelGGL(triplet_term_fwd_k, dim3(1), dim3(RED_THREADS), 0, (hipStream_t)stream, h0, h1, B, T, L,
                       margin, out);
    RBVAE_CHECK_LAUNCH("triplet_term_fwd");
    return RBVAE_OK;
}

int rbvae_triplet_term_bwd(const float* h0, const float* h1, int B, int T, int L, float margin, float scale,
                           const float* gscale_dev, float* dh0, float* dh1, void* stream) {
    RBVAE_CHECK_ARG(h0 && h1 && dh0 && dh1 && B > 0 && L > 0, "triplet_term_bwd: bad arguments");
    RBVAE_CHECK_ARG(T >= 2, "triplet_term_bwd: needs T >= 2 states (got %d)", T);
    hipLaunchKernelGGL(triplet_term_bwd_k, dim3(B), dim3(64), 0, (hipStream_t)stream, h0, h1, B, T, L, margin,
                       scale, gscale_dev, dh0, dh1);
    RBVAE_CHECK_LAUNCH("triplet_term_bwd");
    return RBVAE_OK;
}

size_t rbvae_mse_ws_floats(long n) { (void)n; return MSE_BLOCKS; }

int rbvae_mse_fwd(const float* a, const float* b, long n, float* out, float* ws, void* stream) {
    RBVAE_CHECK_ARG(a && b && out && ws && n > 0, "mse_fwd: bad arguments");
    RBVAE_CHECK_ARG(((uintptr_t)a % 16 == 0) && ((uintptr_t)b % 16 == 0), "mse_fwd: inputs must be 16-byte aligned");
    int nb = cdiv(n >> 2, 256 * 4);
    nb = nb < 1 ? 1 : (nb > MSE_BLOCKS ? MSE_BLOCKS : nb);
    hipLaunchKernelGGL(mse_partial_k, dim3(nb), dim3(256), 0, (hipStream_t)stream, a, b, n, ws);
    hipLaunchKernelGGL(mse_final_k, dim3(1), dim3(MSE_BLOCKS), 0, (hipStream_t)stream, ws, nb, n, out);
    RBVAE_CHECK_LAUNCH("mse_fwd");
    return RBVAE_OK;
}

int rbvae_mse_bwd(const float* a, const float* b, long n, float scale, const float* gscale_dev, float* da,
                  void* stream) {
    RBVAE_CHECK_ARG(a && b && da && n > 0, "mse_bwd: bad arguments");
    int nb = cdiv(n, 256 * 4);
    nb = nb > 2048 ? 2048 : nb;
    hipLaunchKernelGGL(mse_bwd_k, dim3(nb), dim3(256), 0, (hipStream_t)stream, a, b, n, scale, gscale_dev, da);
    RBVAE_CHECK_LAUNCH("mse_bwd");
    return RBVAE_OK;
}

}  // extern "C"
