// The LDM / Stable-Diffusion VAE decoder's Upsample (src/stable-diffusion/ldm/modules/diffusionmodules/model.py:42-57:
// F.interpolate(x, scale_factor=2.0, mode="nearest") followed by Conv2d(c, c, 3, 1, 1)) without the upsampled activation,
// and the two ends of a decode (latent -> rows, rows -> image).
//
// Nearest x2 followed by a zero-padded 3x3 convolution is four 2x2 convolutions of the LOW-resolution input, one per
// output parity class (p, q) = (output row & 1, output column & 1), with pre-summed weights:
//
//   Out[n][2r+p][2c+q][co] = bias + addend + sum_{th,tw in {0,1}} sum_ci A[n][r-1+p+th][c-1+q+tw][ci] * Wf[co][cls][tap][ci]
//   cls = 2p + q, tap = 2th + tw,
//   Wf[co][cls][tap][ci] = sum_{kh in R(p,th)} sum_{kw in R(q,tw)} w[co][ci][kh][kw],
//   R(0,0) = {0}, R(0,1) = {1,2}, R(1,0) = {0,1}, R(1,1) = {2}
//
// (an upsampled pixel 2r+p+kh-1 is low-resolution pixel floor((2r+p+kh-1)/2); zero padding of the upsampled image is zero
// outside the low-resolution image).  4/9 of the multiply-adds of the form as written, and the activation of four times
// the input's size is neither written nor read back.
//
// upconv_halo_k is conv_halo_k (conv_halo.hip) with the tap loop of one parity class: a workgroup owns a 16 x 16 block of
// low-resolution pixels x 128 output channels x ONE class; per 128-byte channel slice the 18 x 18 patch is staged in LDS
// once (chunk-major image, conflict-free fragment reads, a tap = a constant slot offset, the class = a per-workgroup
// one), the folded tap tiles [128][128 B] arrive by LDS-DMA through a ring of FOUR slots -- four taps per slice, so the
// slot of a tap is static -- waited for with counted vmcnt; the tile leaves through LDS as whole 16-byte NHWC chunks to the
// stride-2 output pixels of the class.  Per slice a workgroup takes in 41 KB of patch + 4 x 16 KB of weights for
// 256 x 128 x 256 MACs.  The four classes of a block run back to back on one XCD (they read the same patch from its L2).
#include "conv_halo.h"

namespace rbvae {

struct UcArgs {
    const unsigned char* A;        // [Nimg*IH*IW][lda] T
    const unsigned char* W;        // [Nout][16][Kc] T (rbvae_upconv_fold)
    unsigned char* Out;            // [Nimg*2IH*2IW][ldo] T
    const float* bias;             // [Nout] or null
    const unsigned char* addend;   // [Nimg*2IH*2IW][ldo] T or null
    const unsigned char* zero;     // >= 128 zero bytes
    int Nimg, IH, IW, Kc, Nout, lda, ldo;
    int tiles_r, tiles_c, ntn, total;
};

constexpr int UC_RING = 4;         // = taps per class: ring slot of tap j is j
constexpr int UC_TAPS = 4;

template <typename T>
__global__ __launch_bounds__(512) void upconv_halo_k(const UcArgs p) {
    constexpr int ES = sizeof(T);
    constexpr int KE = 128 / ES, EC = 16 / ES;
    constexpr int MT = CH_MT, NTW = CH_NTW, LOADS = CH_LOADS;
    constexpr int PITCH = CH_BN * ES + 16;
    constexpr int A_BYTES = 2 * CH_ABUF;
    constexpr int CPR = CH_BN / EC;              // 16-B chunks per tile row
    constexpr int RL = 512 / CPR;                // row lanes of the store phase
    constexpr int ITERS = CH_BM / RL;
    constexpr int RINGB = ch_lds_main<T, UC_RING>();
    static_assert(CH_BM * PITCH <= RINGB && A_BYTES + UC_RING * CH_BBYTES <= RINGB, "LDS carve");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int* s_orow = (int*)(smem + RINGB);            // [256]
    int* s_pix = s_orow + CH_BM;                   // [336]

    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);

    // work item: (pixel block, channel tile, class), class fastest; an XCD walks a contiguous range of items, so the
    // 4 * ntn items that read one patch share an L2.  Bijective for any total.
    const int item = xcd_item(blockIdx.x, p.total);
    const int cls = item & 3, it4 = item >> 2;
    const int mtile = it4 / p.ntn, ntile = it4 - mtile * p.ntn;
    const int per_img = p.tiles_r * p.tiles_c;
    const int n = mtile / per_img, trc = mtile - n * per_img;
    const int tr = trc / p.tiles_c, tc = trc - tr * p.tiles_c;
    const int r0 = tr * CH_T, c0 = tc * CH_T, n0 = ntile * CH_BN;
    const int cp = cls >> 1, cq = cls & 1;
    const int OH = 2 * p.IH, OW = 2 * p.IW;

    // ---- tables: output row of every low-resolution pixel of the block (this class), source row of every patch slot
    if (tid < CH_BM) {
        const int r = r0 + (tid >> 4), c = c0 + (tid & 15);
        s_orow[tid] = (r < p.IH && c < p.IW) ? (n * OH + 2 * r + cp) * OW + 2 * c + cq : -1;
    }
    if (tid < CH_NSLOT_PAD) {                      // (inline: mirrors conv_halo_k's slot table with dh0 = dw0 = -1)
        int v = -1;
        if (tid < CH_NSLOT) {
            const int pr = tid / CH_PW, pc = tid - pr * CH_PW;
            const int ih = r0 + pr - 1, iw = c0 + pc - 1;
            if (ih >= 0 && ih < p.IH && iw >= 0 && iw < p.IW) v = (n * p.IH + ih) * p.IW + iw;
        }
        s_pix[tid] = v;
    }
    __syncthreads();

    // ---- input staging roles: piece i of this thread = (slot (tid>>3) + 64 i, chunk tid&7)
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;
    const int chunk = tid & 7;
    const unsigned char* zsrc = p.zero + chunk * 16;
    int pixr[CH_NA];                 // source pixel row of the six pieces: -1 zero (padding), -2 no such slot
#pragma unroll
    for (int i = 0; i < CH_NA; ++i) pixr[i] = ch_piece_pix(s_pix, tid, i);
    // the six staged pieces (ch_piece_load, ch_a_landed); loads, wait and uses sit inside one unrolled slice body (see
    // conv_halo.hip)
    u32x4_t areg[CH_NA];
    auto a_load = [&](int kc) {
#pragma unroll
        for (int i = 0; i < CH_NA; ++i) areg[i] = ch_piece_load(ch_piece_src<ES>(p.A, pixr[i], p.lda, kc, chunk, zsrc));
    };
    auto a_write = [&](int buf) {
#pragma unroll
        for (int i = 0; i < CH_NA; ++i) {
            // (inline: mirrors conv_halo_k's piece_write)
            const unsigned dst = lds0 + (unsigned)buf * CH_ABUF + ch_plane_off(chunk) + (unsigned)((tid >> 3) + 64 * i) * 16;
            if (pixr[i] >= -1) asm volatile("ds_write_b128 %0, %1" ::"v"(dst), "v"(areg[i]) : "memory");
        }
    };

    // ---- weight staging roles (LDS-DMA): instruction i of wave w moves rows (w*2+i)*8 .. +7 of the tap tile
    const int srow = lane >> 3, schunk = lane & 7;
    unsigned blane[LOADS];
#pragma unroll
    for (int i = 0; i < LOADS; ++i) blane[i] = ch_blane<ES, 16>((w * LOADS + i) * 8 + srow, schunk, p.Kc);
    const unsigned char* wtile = p.W + ((size_t)n0 * 16 * p.Kc + (size_t)cls * UC_TAPS * p.Kc) * ES;
    const int nkc = p.Kc / KE;
    // folded tap tile of (slice kc, tap j) -> ring slot j
    auto b_issue = [&](int kc, auto j_tag) {
        constexpr int j = decltype(j_tag)::value;
        ch_tile_issue(ch_tap_src<ES, j>(wtile, p.Kc, kc), blane, smem + A_BYTES + j * CH_BBYTES + (w * LOADS) * 1024);
    };

    // ---- fragment addresses: the class shifts every patch read by (p, q), a tap by its constant (th, tw)
    const int fi = lane & 15, fg = lane >> 4;
    const int wr = w >> 1, wc = w & 1;
    unsigned abase[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) abase[mt] = ch_aplane(lds0, fg) + (unsigned)((wr * MT + mt + cp) * CH_PW + fi + cq) * 16;
    const int fsw = (fi >> 1) & 7;
    const unsigned offB0 = ch_boff(lds0, wc * NTW * 16 + fi, (0 + fg) ^ fsw), offB1 = ch_boff(lds0, wc * NTW * 16 + fi, (4 + fg) ^ fsw);

    f32x4_t acc[MT][NTW];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) acc[mt][nt] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    unsigned ta[MT];                         // patch read addresses of the slice being read (buffer folded in)
    auto set_slice = [&](int kc) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) ta[mt] = ch_slice_addr(abase[mt], kc);
    };
    auto read_half = [&](auto j_tag, auto kk_tag, u32x4_t (&fa)[MT], u32x4_t (&fb)[NTW]) {
        constexpr int j = decltype(j_tag)::value, kk = decltype(kk_tag)::value;
        ch_read_half<kk * CH_KKOFF + ((j >> 1) * CH_PW + (j & 1)) * 16, j * CH_BBYTES>(ta, kk == 0 ? offB0 : offB1, 0u, fa, fb);
    };
    using K0 = std::integral_constant<int, 0>;
    using K1 = std::integral_constant<int, 1>;

    // ---- prologue: patch of slice 0 and its four tap tiles
    a_load(0);
    b_issue(0, std::integral_constant<int, 0>{});
    b_issue(0, std::integral_constant<int, 1>{});
    b_issue(0, std::integral_constant<int, 2>{});
    b_issue(0, std::integral_constant<int, 3>{});
    ch_a_landed<0>(areg);
    a_write(0);
    wait_vm_lgkm_barrier<0>();
    u32x4_t fa0[MT], fb0[NTW], fa1[MT], fb1[NTW];
    set_slice(0);
    read_half(K0{}, K0{}, fa0, fb0);

    // ---- main loop: slices of 128 bytes of channels, the four taps unrolled; the software pipeline over the 32-k halves
    // of conv_halo_k.  The barrier inside step s (between its two MFMA groups) says: every wave has the fragments of step s
    // in registers, and the tile of step s+1 has landed.  Behind it the tile of step s+4 goes into the slot step s just
    // left (slot s % 4).  Vector-memory operations in flight at that barrier, oldest first: tiles s+1, s+2, s+3, and the six
    // patch pieces of the next slice issued behind the tile of tap 0 -- so the counted wait leaves 2 tiles in flight, plus
    // the six pieces at taps 1 and 2.  At tap 3 the pieces are waited for (behind them: two tiles) and written to the
    // other patch buffer in front of the barrier, whose last reader finished a slice ago; the first read of the next
    // slice follows the barrier.
    auto slice = [&](int kc, auto more_tag) {
        constexpr bool more = decltype(more_tag)::value;       // another slice follows (the last slice is its own instance)
        static_for<0, UC_TAPS>([&](auto j_tag) {
            constexpr int j = decltype(j_tag)::value;
            constexpr int nj = (j + 1) % UC_TAPS;            // tap of the next step
            using NJ = std::integral_constant<int, nj>;
            read_half(j_tag, K1{}, fa1, fb1);
            frag_landed<MT + NTW>(fa0, fb0);
            __builtin_amdgcn_sched_barrier(0);
            mma_group<T>(acc, fa0, fb0);
            __builtin_amdgcn_sched_barrier(0);
            frag_landed<0>(fa1, fb1);
            if constexpr (j == UC_TAPS - 1 && !more) {       // the very last step reads nothing ahead
                __builtin_amdgcn_sched_barrier(0);
                mma_group<T>(acc, fa1, fb1);
            } else {
                if constexpr (more) {
                    if constexpr (j == 3) {
                        ch_a_landed<2 * LOADS>(areg);
                        a_write((kc + 1) & 1);
                    }
                    if constexpr (j == 1 || j == 2) wait_vm_lgkm_barrier<2 * LOADS + CH_NA>();
                    else wait_vm_lgkm_barrier<2 * LOADS>();
                    b_issue(kc + 1, j_tag);
                    if constexpr (j == 0) a_load(kc + 1);
                } else {
                    // the last slice issues nothing: tiles j+1 .. 3 are all that is in flight
                    if constexpr (j == 0) wait_vm_lgkm_barrier<2 * LOADS>();
                    else if constexpr (j == 1) wait_vm_lgkm_barrier<LOADS>();
                    else wait_vm_lgkm_barrier<0>();
                }
                if constexpr (nj == 0) set_slice(kc + 1);
                read_half(NJ{}, K0{}, fa0, fb0);
                __builtin_amdgcn_sched_barrier(0);
                mma_group<T>(acc, fa1, fb1);
                __builtin_amdgcn_sched_barrier(0);
            }
        });
    };
    for (int kcl = 0; kcl + 1 < nkc; ++kcl) {
        int kc = kcl;
        asm volatile("" : "+s"(kc));        // opaque: no per-tap address induction variables across the slice loop
        slice(kc, std::true_type{});
    }
    slice(nkc - 1, std::false_type{});
    __syncthreads();

    // ---- epilogue, register phase: bias; lane owns pixel fi, channels 4*fg..+3 of each 16 x 16 tile
    unsigned char* tile = smem;
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) {
        const int cb = (wc * NTW + nt) * 16 + 4 * fg;
        float bz[4] = {0.f, 0.f, 0.f, 0.f};
        if (p.bias) {
            const float4 b4 = *(const float4*)(p.bias + n0 + cb);
            bz[0] = b4.x; bz[1] = b4.y; bz[2] = b4.z; bz[3] = b4.w;
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int row = (wr * MT + mt) * 16 + fi;
            unsigned char* dst = tile + row * PITCH + cb * ES;
            if constexpr (ES == 4) {
                epi_stage<T>(dst, acc[mt][nt][0] + bz[0], acc[mt][nt][1] + bz[1], acc[mt][nt][2] + bz[2], acc[mt][nt][3] + bz[3]);
            } else {                                       // (epi_stage's bf16 half changes the listings: ch_bias_pack2)
                uint2 pk;
                pk.x = ch_bias_pack2(acc[mt][nt][0], bz[0], acc[mt][nt][1], bz[1]);
                pk.y = ch_bias_pack2(acc[mt][nt][2], bz[2], acc[mt][nt][3], bz[3]);
                *(uint2*)dst = pk;
            }
        }
    }
    lds_barrier();

    // ---- store phase: whole 16-B chunks of NHWC rows (+ addend) to the class's stride-2 output pixels; one pixel's 128
    // channels are one contiguous run of 128 * ES bytes
    const int sch = tid % CPR, rl = tid / CPR;
    const int scol = n0 + sch * EC;
    int orow_[ITERS];
    u32x4_t av[ITERS];
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
        orow_[it] = s_orow[it * RL + rl];
        if (p.addend) av[it] = ch_addend_chunk<ES>(p.addend, orow_[it], p.ldo, scol);
    }
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
        const int row = it * RL + rl;
        u32x4_t val = *(const u32x4_t*)(tile + row * PITCH + sch * 16);
        if (p.addend) {                               // (inline: mirrored by conv_halo_k's residual add)
            T* ev = (T*)&val;
            const T* ae = (const T*)&av[it];
#pragma unroll
            for (int e = 0; e < EC; ++e) Elem<T>::store(ev + e, Elem<T>::load(ev + e) + Elem<T>::load(ae + e));
        }
        ch_store_chunk<ES>(p.Out, orow_[it], p.ldo, scol, val);
    }
}

template <typename T>
static int launch_uc(const UcArgs& a, hipStream_t st) {
    const size_t lds = (size_t)ch_lds_main<T, UC_RING>() + CH_BM * 4 + CH_NSLOT_PAD * 4 + 16;
    static_assert(ch_lds_main<float, UC_RING>() + CH_BM * 4 + CH_NSLOT_PAD * 4 + 16 <= 160 * 1024, "LDS");
    lds_attr_once<upconv_halo_k<T>>(160 * 1024);
    hipLaunchKernelGGL((upconv_halo_k<T>), dim3(a.total), dim3(512), lds, st, a);
    RBVAE_CHECK_LAUNCH("upconv3x3_halo");
    return RBVAE_OK;
}

// ---- the folded weights --------------------------------------------------------------------------------------------
// out[co][4 cls + tap][k] for k < Kc: the f32 sum, kh ascending and inside it kw ascending, starting from +0, rounded once
// to T; k >= Ci: zero.
template <typename T>
__global__ void upconv_fold_k(const float* __restrict__ w, T* __restrict__ out, int Co, int Ci, int Kc) {
    const long total = (long)Co * 16 * Kc;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int k = (int)(i % Kc);
        const int slot = (int)(i / Kc % 16), co = (int)(i / Kc / 16);
        float s = 0.f;
        if (k < Ci) {
            const int cls = slot >> 2, tap = slot & 3;
            const int p = cls >> 1, q = cls & 1, th = tap >> 1, tw = tap & 1;
            const int h0 = th == 0 ? 0 : (p == 0 ? 1 : 2), h1 = th == 0 ? (p == 0 ? 0 : 1) : 2;
            const int w0 = tw == 0 ? 0 : (q == 0 ? 1 : 2), w1 = tw == 0 ? (q == 0 ? 0 : 1) : 2;
            const float* wp = w + ((size_t)co * Ci + k) * 9;
            for (int kh = h0; kh <= h1; ++kh)
                for (int kw = w0; kw <= w1; ++kw) s = __fadd_rn(s, wp[kh * 3 + kw]);
        }
        Elem<T>::store(out + i, s);
    }
}

// nearest x2 of NHWC rows as 16-byte chunks (the as-written baseline: model.py:52)
__global__ void nearest2x_rows_k(const uint4* __restrict__ in, uint4* __restrict__ out, int Nimg, int IH, int IW, int cpr,
                                 int ldi16, int ldo16) {
    const long total = (long)Nimg * 4 * IH * IW * cpr;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int ch = (int)(i % cpr);
        const long orow = i / cpr;
        const int OW = 2 * IW, OH = 2 * IH;
        const int ox = (int)(orow % OW), oy = (int)(orow / OW % OH), n = (int)(orow / OW / OH);
        const long irow = ((long)n * IH + (oy >> 1)) * IW + (ox >> 1);
        out[orow * ldo16 + ch] = in[irow * ldi16 + ch];
    }
}

// z f32 [N][Z][hw] -> rows [N*hw][Kpad] of T: z * f32(1 / scale_factor) (one f32 rounding), zero pad columns
template <typename T>
__global__ void latent_rows_k(const float* __restrict__ z, T* __restrict__ out, int N, int Z, int HW, int Kpad, float inv) {
    const long total = (long)N * HW * Kpad;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % Kpad);
        const long row = i / Kpad;
        const int n = (int)(row / HW), px = (int)(row % HW);
        const float v = c < Z ? __fmul_rn(z[((size_t)n * Z + c) * HW + px], inv) : 0.f;
        Elem<T>::store(out + i, v);
    }
}

// rows [N*HW][ld] of T (3 used columns) -> f32 [N][3][HW] and / or u8 [N][HW][3]
template <typename T>
__global__ void decoded_to_image_k(const T* __restrict__ rows, int ld, float* __restrict__ img, unsigned char* __restrict__ u8,
                                   int N, int HW) {
    const long total = (long)N * HW;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int n = (int)(i / HW), px = (int)(i % HW);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float x = Elem<T>::load(rows + (size_t)i * ld + c);
            if (img) img[((size_t)n * 3 + c) * HW + px] = x;
            if (u8) {
                float t = __fdiv_rn(__fadd_rn(x, 1.0f), 2.0f);
                t = t < 0.f ? 0.f : (t > 1.f ? 1.f : t);
                u8[(size_t)i * 3 + c] = (unsigned char)(int)__fmul_rn(255.f, t);
            }
        }
    }
}

static int grid_for(long total) {
    const long b = (total + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}

}  // namespace rbvae

using namespace rbvae;

extern "C" int rbvae_upconv_fold(int dtype, const float* w, void* out, int Co, int Ci, int Kc, void* stream) {
    RBVAE_CHECK_ARG(w && out, "upconv_fold: null pointer");
    RBVAE_CHECK_ARG(dtype == RBVAE_F32 || dtype == RBVAE_BF16, "upconv_fold: dtype %d", dtype);
    RBVAE_CHECK_ARG(Co > 0 && Ci > 0 && Kc >= Ci && (long)Co * 16 * Kc < (1l << 31), "upconv_fold: Co=%d Ci=%d Kc=%d", Co, Ci, Kc);
    const long total = (long)Co * 16 * Kc;
    if (dtype == RBVAE_F32)
        hipLaunchKernelGGL(upconv_fold_k<float>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, w, (float*)out, Co, Ci, Kc);
    else
        hipLaunchKernelGGL(upconv_fold_k<bf16_t>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, w, (bf16_t*)out, Co, Ci, Kc);
    RBVAE_CHECK_LAUNCH("upconv_fold");
    return RBVAE_OK;
}

extern "C" int rbvae_upconv3x3_halo_ok(int dtype, int Nimg, int IH, int IW, int Kc, int Nout) {
    if (dtype != RBVAE_F32 && dtype != RBVAE_BF16) return 0;
    const int KE = dtype == RBVAE_F32 ? 32 : 64;
    if (Kc <= 0 || Kc % KE || Nout <= 0 || Nout % CH_BN) return 0;
    // maps with a side below 5: at most 4 x 16 of a block's 256 pixel rows are real (a quarter of the matrix-core work):
    // rbvae_gather_gemm's 128-row tiles of the whole batch serve those
    if (Nimg < 1 || IH < 5 || IW < 5) return 0;
    if ((long)Nimg * 4 * IH * IW >= (1l << 30)) return 0;
    if ((long)Nimg * cdiv(IH, CH_T) * cdiv(IW, CH_T) * (Nout / CH_BN) * 4 >= (1l << 30)) return 0;
    if ((long)CH_BN * 16 * Kc * 4 >= (1l << 31)) return 0;         // 32-bit per-lane weight offsets
    return 1;
}

extern "C" int rbvae_upconv3x3_halo(int dtype, const void* A, const void* Wf, void* Out, const float* bias, const void* addend,
                                    const void* zero_page, int Nimg, int IH, int IW, int Kc, int Nout, int lda, int ldo,
                                    void* stream) {
    if (!rbvae_upconv3x3_halo_ok(dtype, Nimg, IH, IW, Kc, Nout))
        return fail(RBVAE_E_UNSUPPORTED, "upconv3x3_halo: shape not covered (dtype %d, %d x %dx%d, Kc %d, Nout %d)", dtype, Nimg,
                    IH, IW, Kc, Nout);
    RBVAE_CHECK_ARG(A && Wf && Out && zero_page, "upconv3x3_halo: null pointer");
    const int ES = dtype == RBVAE_F32 ? 4 : 2;
    if (const int e = epi_check_rows("upconv3x3_halo", ES, Kc, Nout, lda, ldo,
                                    (uintptr_t)A | (uintptr_t)Wf | (uintptr_t)Out | (uintptr_t)zero_page | (uintptr_t)addend | (uintptr_t)bias))
        return e;
    UcArgs a;
    a.A = (const unsigned char*)A; a.W = (const unsigned char*)Wf; a.Out = (unsigned char*)Out; a.bias = bias;
    a.addend = (const unsigned char*)addend; a.zero = (const unsigned char*)zero_page;
    a.Nimg = Nimg; a.IH = IH; a.IW = IW; a.Kc = Kc; a.Nout = Nout; a.lda = lda; a.ldo = ldo;
    a.tiles_r = cdiv(IH, CH_T); a.tiles_c = cdiv(IW, CH_T); a.ntn = Nout / CH_BN;
    a.total = Nimg * a.tiles_r * a.tiles_c * a.ntn * 4;
    hipStream_t st = (hipStream_t)stream;
    return dtype == RBVAE_F32 ? launch_uc<float>(a, st) : launch_uc<bf16_t>(a, st);
}

extern "C" int rbvae_nearest2x_rows(int dtype, const void* in, void* out, int Nimg, int IH, int IW, int C, int ldi, int ldo,
                                    void* stream) {
    RBVAE_CHECK_ARG(in && out, "nearest2x_rows: null pointer");
    RBVAE_CHECK_ARG(dtype == RBVAE_F32 || dtype == RBVAE_BF16, "nearest2x_rows: dtype %d", dtype);
    const int ES = dtype == RBVAE_F32 ? 4 : 2;
    RBVAE_CHECK_ARG(Nimg > 0 && IH > 0 && IW > 0 && C > 0 && (C * ES) % 16 == 0 && ldi >= C && ldo >= C && (ldi * ES) % 16 == 0 &&
                        (ldo * ES) % 16 == 0 && ((uintptr_t)in | (uintptr_t)out) % 16 == 0,
                    "nearest2x_rows: C=%d ldi=%d ldo=%d (16-byte chunks)", C, ldi, ldo);
    RBVAE_CHECK_ARG((long)Nimg * 4 * IH * IW < (1l << 30), "nearest2x_rows: more than 2^30 pixel rows");
    const int cpr = C * ES / 16;
    const long total = (long)Nimg * 4 * IH * IW * cpr;
    hipLaunchKernelGGL(nearest2x_rows_k, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const uint4*)in, (uint4*)out,
                       Nimg, IH, IW, cpr, ldi * ES / 16, ldo * ES / 16);
    RBVAE_CHECK_LAUNCH("nearest2x_rows");
    return RBVAE_OK;
}

extern "C" int rbvae_latent_rows(int dtype, const float* z, void* rows, int N, int Z, int HW, int Kpad, double scale_factor,
                                 void* stream) {
    RBVAE_CHECK_ARG(z && rows, "latent_rows: null pointer");
    RBVAE_CHECK_ARG(dtype == RBVAE_F32 || dtype == RBVAE_BF16, "latent_rows: dtype %d", dtype);
    RBVAE_CHECK_ARG(N > 0 && Z > 0 && HW > 0 && Kpad >= Z && (long)N * HW * Kpad < (1l << 40), "latent_rows: N=%d Z=%d HW=%d Kpad=%d",
                    N, Z, HW, Kpad);
    const float inv = (float)(1.0 / scale_factor);      // the double quotient rounded once, as torch rounds the scalar
    const long total = (long)N * HW * Kpad;
    if (dtype == RBVAE_F32)
        hipLaunchKernelGGL(latent_rows_k<float>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, z, (float*)rows, N, Z, HW, Kpad, inv);
    else
        hipLaunchKernelGGL(latent_rows_k<bf16_t>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, z, (bf16_t*)rows, N, Z, HW, Kpad, inv);
    RBVAE_CHECK_LAUNCH("latent_rows");
    return RBVAE_OK;
}

extern "C" int rbvae_decoded_to_image(int dtype, const void* rows, int ld, float* img, unsigned char* u8, int N, int HW,
                                      void* stream) {
    RBVAE_CHECK_ARG(rows && (img || u8), "decoded_to_image: null pointer");
    RBVAE_CHECK_ARG(dtype == RBVAE_F32 || dtype == RBVAE_BF16, "decoded_to_image: dtype %d", dtype);
    RBVAE_CHECK_ARG(N > 0 && HW > 0 && ld >= 3, "decoded_to_image: N=%d HW=%d ld=%d", N, HW, ld);
    const long total = (long)N * HW;
    if (dtype == RBVAE_F32)
        hipLaunchKernelGGL(decoded_to_image_k<float>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const float*)rows, ld, img, u8, N, HW);
    else
        hipLaunchKernelGGL(decoded_to_image_k<bf16_t>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)rows, ld, img, u8, N, HW);
    RBVAE_CHECK_LAUNCH("decoded_to_image");
    return RBVAE_OK;
}
