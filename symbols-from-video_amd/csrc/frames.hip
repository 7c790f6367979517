// Raw-frame front end: the reference's Pillow preprocessing on batches of u8 RGB frames (NHWC, 3 channels).
//   resample_h_k / resample_v_k  Pillow's 8-bit resampler (src/libImaging/Resample.c, ImagingResampleHorizontal_8bpc /
//                                ImagingResampleVertical_8bpc) as called by Image.resize in
//                                src/stable-diffusion/get_percep_embeddings.py:59-66 and
//                                models/contrastive_RBVAE/contrastive_RBVAE_train.py:110-114
//   perturb_k                    ToTensor -> add_gaussian_noise / add_occlusion -> ToPILImage
//                                (scripts/evaluation/state_consistency_eval/embedding_matching.py:141-193, 241-248)
//   u8_to_input_k                ToTensor / load_img's x / 255 -> 2x - 1 (get_percep_embeddings.py:68-71)
// Everything is exact: the resampler is integer arithmetic, and the f32 steps are the reference's operations in its
// order with contraction off (a fused multiply-add would round once where the reference rounds twice).
#include "common.h"

#pragma clang fp contract(off)

namespace rbvae {

constexpr int FR_THREADS = 256;
constexpr int RS_PREC = 22;                 // Resample.c PRECISION_BITS for 8-bit images

__device__ __forceinline__ unsigned char clip8(int acc) {
    const int v = acc >> RS_PREC;           // arithmetic shift, as Pillow
    return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// lds[(src & 3) + i] = src[i] for i < n: dword loads for the dwords wholly inside the row, byte loads at its two ends
// (rows of 3*W bytes start anywhere; nothing outside [src, src + n) is read).
__device__ __forceinline__ void stage_bytes(const unsigned char* __restrict__ src, long n, unsigned char* lds) {
    const int lead = (int)((uintptr_t)src & 3);
    const unsigned* base = (const unsigned*)(src - lead);
    const long nd = (lead + n + 3) >> 2;
    for (long j = threadIdx.x; j < nd; j += blockDim.x) {
        const long b0 = 4 * j - lead;                       // row byte of the dword's first byte
        if (b0 >= 0 && b0 + 4 <= n) {
            ((unsigned*)lds)[j] = base[j];
        } else {
            for (int b = 0; b < 4; ++b)
                if (b0 + b >= 0 && b0 + b < n) lds[4 * j + b] = src[b0 + b];
        }
    }
}

// dst[i] = lds[(dst & 3) + i] for i < n, the mirror image of stage_bytes
__device__ __forceinline__ void store_bytes(const unsigned char* lds, long n, unsigned char* __restrict__ dst) {
    const int lead = (int)((uintptr_t)dst & 3);
    unsigned* base = (unsigned*)(dst - lead);
    const long nd = (lead + n + 3) >> 2;
    for (long j = threadIdx.x; j < nd; j += blockDim.x) {
        const long b0 = 4 * j - lead;
        if (b0 >= 0 && b0 + 4 <= n) {
            base[j] = ((const unsigned*)lds)[j];
        } else {
            for (int b = 0; b < 4; ++b)
                if (b0 + b >= 0 && b0 + b < n) dst[b0 + b] = lds[4 * j + b];
        }
    }
}

// Horizontal pass: one workgroup per (output row, image).  Output row r is source row row0 + r resampled to out_w
// pixels; the source row is staged in LDS (dword loads), the output row assembled in LDS and written with dword stores.
__global__ __launch_bounds__(FR_THREADS) void resample_h_k(const unsigned char* __restrict__ in,
                                                           unsigned char* __restrict__ out, int in_h, int in_w,
                                                           int rows, int out_w, int row0, const int* __restrict__ bounds,
                                                           const int* __restrict__ kk, int ksize, int in_lds) {
    extern __shared__ unsigned char fr_lds[];
    const int r = blockIdx.x, n = blockIdx.y;
    const long in_bytes = 3L * in_w, out_bytes = 3L * out_w;
    const unsigned char* src = in + ((long)n * in_h + row0 + r) * in_bytes;
    unsigned char* dst = out + ((long)n * rows + r) * out_bytes;
    unsigned char* irow = fr_lds;
    unsigned char* orow = fr_lds + in_lds;
    stage_bytes(src, in_bytes, irow);
    __syncthreads();
    const int ilead = (int)((uintptr_t)src & 3), olead = (int)((uintptr_t)dst & 3);
    for (int x = threadIdx.x; x < out_w; x += blockDim.x) {
        const int xmin = bounds[2 * x], xmax = min(bounds[2 * x + 1], ksize);
        const int* k = kk + (long)x * ksize;
        int a0 = 1 << (RS_PREC - 1), a1 = a0, a2 = a0;
        for (int t = 0; t < xmax; ++t) {
            const int sx = xmin + t;
            if (sx < 0 || sx >= in_w) continue;
            const int c = k[t];
            const unsigned char* p = irow + ilead + 3 * sx;
            a0 += (int)p[0] * c;
            a1 += (int)p[1] * c;
            a2 += (int)p[2] * c;
        }
        unsigned char* q = orow + olead + 3 * x;
        q[0] = clip8(a0);
        q[1] = clip8(a1);
        q[2] = clip8(a2);
    }
    __syncthreads();
    store_bytes(orow, out_bytes, dst);
}

// Vertical pass: one workgroup per (VEC*256-byte slice of an output row, output row, image); every lane owns VEC
// consecutive bytes of the row (the three channels of a pixel are independent lanes of the same sum), so row reads
// and writes are coalesced and the row's coefficients are uniform across the workgroup.  Output row yy reads source
// rows bounds[yy][0] - row0 + t (Pillow's shift of the vertical bounds by the first row the horizontal pass kept).
template <int VEC>
__global__ __launch_bounds__(FR_THREADS) void resample_v_k(const unsigned char* __restrict__ in,
                                                           unsigned char* __restrict__ out, int in_h, long row_bytes,
                                                           int out_h, int row0, const int* __restrict__ bounds,
                                                           const int* __restrict__ kk, int ksize) {
    const int yy = blockIdx.y, n = blockIdx.z;
    const long b = ((long)blockIdx.x * FR_THREADS + threadIdx.x) * VEC;
    if (b >= row_bytes) return;
    const int ymin = bounds[2 * yy] - row0, ymax = min(bounds[2 * yy + 1], ksize);
    const int* k = kk + (long)yy * ksize;
    const unsigned char* src = in + (long)n * in_h * row_bytes + b;
    int acc[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] = 1 << (RS_PREC - 1);
    for (int t = 0; t < ymax; ++t) {
        const int sy = ymin + t;
        if (sy < 0 || sy >= in_h) continue;
        const int c = k[t];
        if constexpr (VEC == 4) {
            const unsigned w = *(const unsigned*)(src + (long)sy * row_bytes);
#pragma unroll
            for (int v = 0; v < 4; ++v) acc[v] += (int)((w >> (8 * v)) & 0xffu) * c;
        } else {
            acc[0] += (int)src[(long)sy * row_bytes] * c;
        }
    }
    unsigned char* dst = out + ((long)n * out_h + yy) * row_bytes + b;
    if constexpr (VEC == 4) {
        // Each clipped byte goes through an empty asm before it is packed.  Left to itself the compiler turns
        // clip8(a) | clip8(b) << 8 into v_ashr_pk_u8_i32, which writes 16 bits of its destination, and then ORs the other
        // two bytes into that register as if its upper half were zero.  The register is the high word of a 64-bit
        // multiply-add: small after any tap, never written when every tap of a row is skipped, and then whatever an
        // earlier wave left there comes out as bytes 2 and 3 of the dword (tests/test_frames_abi_gpu.py, synthetic-W4).
        unsigned w = 0;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            unsigned c = clip8(acc[v]);
            asm volatile("" : "+v"(c));
            w |= c << (8 * v);
        }
        *(unsigned*)dst = w;
    } else {
        dst[0] = clip8(acc[0]);
    }
}

// One pixel (three channels) per lane.  x = u8 / 255 (true division, ToTensor); kind 1: x = clamp(x + (n*std + mean),
// 0, 1) with n from the NCHW noise tensor; kind 2: x = 0.5 inside the frame's square; then ToPILImage's mul(255).byte()
// (truncation toward zero).
__global__ __launch_bounds__(FR_THREADS) void perturb_k(const unsigned char* __restrict__ in,
                                                        unsigned char* __restrict__ out, long npix, int H, int W, int kind,
                                                        const float* __restrict__ noise, float std_, float mean_,
                                                        const int* __restrict__ boxes) {
    const long hw = (long)H * W;
    for (long p = (long)blockIdx.x * FR_THREADS + threadIdx.x; p < npix; p += (long)gridDim.x * FR_THREADS) {
        const long n = p / hw, s = p - n * hw;
        const int y = (int)(s / W), x = (int)(s - (long)y * W);
        bool occ = false;
        if (kind == 2) {
            const int bx = boxes[3 * n], by = boxes[3 * n + 1], bs = boxes[3 * n + 2];
            occ = x >= bx && x < bx + bs && y >= by && y < by + bs;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v = (float)in[3 * p + c] / 255.0f;
            if (kind == 1) {
                const float t = noise[(n * 3 + c) * hw + s] * std_ + mean_;
                v = v + t;
                v = fminf(fmaxf(v, 0.0f), 1.0f);
            } else if (occ) {
                v = 0.5f;
            }
            out[3 * p + c] = (unsigned char)(int)(v * 255.0f);
        }
    }
}

// u8 NHWC -> f32 NCHW: mode 0 x / 255 (ToTensor), mode 1 2 * (x / 255) - 1 (load_img, two roundings)
__global__ __launch_bounds__(FR_THREADS) void u8_to_input_k(const unsigned char* __restrict__ in, float* __restrict__ out,
                                                            long npix, long hw, int mode) {
    for (long p = (long)blockIdx.x * FR_THREADS + threadIdx.x; p < npix; p += (long)gridDim.x * FR_THREADS) {
        const long n = p / hw, s = p - n * hw;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v = (float)in[3 * p + c] / 255.0f;
            if (mode == 1) v = 2.0f * v - 1.0f;
            out[(n * 3 + c) * hw + s] = v;
        }
    }
}

static int elementwise_blocks(long npix) {
    const long b = (npix + FR_THREADS - 1) / FR_THREADS;
    return (int)(b < 65536 ? b : 65536);
}

}  // namespace rbvae

using namespace rbvae;

extern "C" int rbvae_resample_u8(const unsigned char* in, unsigned char* out, int N, int in_h, int in_w, int out_h,
                                 int out_w, int vertical, int row0, const int* bounds, const int* kk, int ksize,
                                 void* stream) {
    RBVAE_CHECK_ARG(in && out && bounds && kk, "resample_u8: null pointer");
    RBVAE_CHECK_ARG(N > 0 && in_h > 0 && in_w > 0 && out_h > 0 && out_w > 0 && ksize > 0,
                    "resample_u8: bad shape N=%d in %dx%d out %dx%d ksize %d", N, in_h, in_w, out_h, out_w, ksize);
    RBVAE_CHECK_ARG(N <= 65535, "resample_u8: N=%d above 65535 (split the batch)", N);
    hipStream_t st = (hipStream_t)stream;
    if (!vertical) {
        RBVAE_CHECK_ARG(row0 >= 0 && row0 + out_h <= in_h, "resample_u8: rows %d..%d outside the %d source rows", row0,
                        row0 + out_h, in_h);
        const int in_lds = (int)((3L * in_w + 4 + 3) & ~3L), out_lds = (int)((3L * out_w + 4 + 3) & ~3L);
        if ((long)in_lds + out_lds > 65536)
            return fail(RBVAE_E_UNSUPPORTED, "resample_u8: rows of %d -> %d pixels exceed 64 KB of LDS", in_w, out_w);
        hipLaunchKernelGGL(resample_h_k, dim3(out_h, N), dim3(FR_THREADS), in_lds + out_lds, st, in, out, in_h, in_w,
                           out_h, out_w, row0, bounds, kk, ksize, in_lds);
    } else {
        RBVAE_CHECK_ARG(in_w == out_w, "resample_u8: the vertical pass keeps the width (%d != %d)", in_w, out_w);
        RBVAE_CHECK_ARG(out_h <= 65535, "resample_u8: %d output rows above 65535", out_h);
        const long row_bytes = 3L * out_w;
        const bool vec = row_bytes % 4 == 0 && (uintptr_t)in % 4 == 0 && (uintptr_t)out % 4 == 0;
        if (vec)
            hipLaunchKernelGGL(resample_v_k<4>, dim3(cdiv(row_bytes, 4 * FR_THREADS), out_h, N), dim3(FR_THREADS), 0, st,
                               in, out, in_h, row_bytes, out_h, row0, bounds, kk, ksize);
        else
            hipLaunchKernelGGL(resample_v_k<1>, dim3(cdiv(row_bytes, FR_THREADS), out_h, N), dim3(FR_THREADS), 0, st, in,
                               out, in_h, row_bytes, out_h, row0, bounds, kk, ksize);
    }
    RBVAE_CHECK_LAUNCH("resample_u8");
    return RBVAE_OK;
}

extern "C" int rbvae_perturb_u8(const unsigned char* in, unsigned char* out, int N, int H, int W, int kind,
                                const float* noise, float std_, float mean_, const int* boxes, void* stream) {
    RBVAE_CHECK_ARG(in && out && N > 0 && H > 0 && W > 0, "perturb_u8: bad arguments");
    RBVAE_CHECK_ARG(kind == 1 || kind == 2, "perturb_u8: kind %d is neither 1 (gaussian noise) nor 2 (occlusion)", kind);
    RBVAE_CHECK_ARG(kind != 1 || noise, "perturb_u8: gaussian noise needs the noise tensor");
    RBVAE_CHECK_ARG(kind != 2 || boxes, "perturb_u8: occlusion needs the boxes");
    const long npix = (long)N * H * W;
    hipLaunchKernelGGL(perturb_k, dim3(elementwise_blocks(npix)), dim3(FR_THREADS), 0, (hipStream_t)stream, in, out,
                       npix, H, W, kind, noise, std_, mean_, boxes);
    RBVAE_CHECK_LAUNCH("perturb_u8");
    return RBVAE_OK;
}

extern "C" int rbvae_u8_to_input(const unsigned char* in, float* out, int N, int H, int W, int mode, void* stream) {
    RBVAE_CHECK_ARG(in && out && N > 0 && H > 0 && W > 0, "u8_to_input: bad arguments");
    RBVAE_CHECK_ARG(mode == 0 || mode == 1, "u8_to_input: mode %d is neither 0 (ToTensor) nor 1 (SD)", mode);
    const long npix = (long)N * H * W;
    hipLaunchKernelGGL(u8_to_input_k, dim3(elementwise_blocks(npix)), dim3(FR_THREADS), 0, (hipStream_t)stream, in, out,
                       npix, (long)H * W, mode);
    RBVAE_CHECK_LAUNCH("u8_to_input");
    return RBVAE_OK;
}
