/* librbvae_hip -- C ABI of the MI355X (gfx950) RBVAE hot path.
 *
 * The reference (matt-suncy/symbols-from-video) has no FFI: its hot path is the
 * torch ops issued by Seq2SeqBinaryVAE.forward/encode and by the trainer's loss
 * functions.  Each entry point below replaces one of those op groups; the
 * reference call site it stands in for is cited as file:line (relative to the
 * reference root).  INTEGRATION.md shows the ctypes stub a maintainer adds.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer valid for the duration of the call in
 *    stream order; the library never allocates, frees or retains them;
 *  - `stream` is a hipStream_t (NULL = default stream); calls are asynchronous
 *    and never synchronise;
 *  - return value 0 = ok, negative = RBVAE_E_*; rbvae_last_error() gives a
 *    thread-local message; nothing throws or exits across the boundary;
 *  - `dtype` selects the activation/weight storage type of the conv/linear
 *    kernels: RBVAE_F32 (exact-fp32 parity mode, f32 MFMA) or RBVAE_BF16
 *    (bf16 storage, f32 accumulation, bf16 MFMA).  LSTM, binarise and the loss
 *    reductions are always f32;
 *  - activations are NHWC ("pixel rows of C channels"), weights are the packed
 *    layouts written by the rbvae_run_jobs pack jobs (kinds 0 and 3, see that entry
 *    point) from the reference-layout f32 parameters;
 *  - the keyed dropout of an epilogue (drop_mode 1 of rbvae_gather_gemm, rbvae_conv3x3s2_halo,
 *    rbvae_deconv3x3s2_halo and rbvae_conv_first_fused) takes 0 <= drop_p < 1: anything else, NaN included, is
 *    RBVAE_E_INVALID and nothing is launched (the threshold is floor(drop_p * 2^32), a conversion that is undefined from
 *    1.0 up and wraps below 0).  drop_p is not read in drop_mode 0 and 2.
 * The hardware-map probes and phase-stamp hooks of debug builds are NOT part of this
 * ABI: include/rbvae_dbg.h, librbvae_dbg.so.
 */
#ifndef RBVAE_HIP_H
#define RBVAE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RBVAE_OK 0
#define RBVAE_E_INVALID (-1)     /* bad argument (shape, alignment, null pointer) */
#define RBVAE_E_LAUNCH (-2)      /* HIP reported a launch error */
#define RBVAE_E_UNSUPPORTED (-3) /* configuration outside what the kernels cover */

#define RBVAE_F32 0
#define RBVAE_BF16 1

int rbvae_version(void);
/* counter[0] += inc: the device step counter the dropout / noise hashes mix in (graph replay safe). */
int rbvae_counter_add(unsigned long long* counter, unsigned long long inc, void* stream);
const char* rbvae_last_error(void);

/* ---- binarise + KL -------------------------------------------------------
 * binary_concrete_logits (models/percep_RBVAE/percep_RBVAE_model.py:17-44; triplet
 * variant triplet_RBVAE_model.py:18-45 = noise_ratio 1; simple variant
 * simple_RBVAE_model.py:17-44 = noise_eps 1e-10) fused with kl_binary_concrete
 * applied to the SAMPLE z (models/percep_RBVAE/percep_RBVAE_train.py:52-76 as
 * called at :528).  U is the uniform noise the reference draws with torch.rand
 * on the host (:33); the caller supplies it so codes are reproducible.
 *   y_soft = sigmoid((h + r*(log(U+e) - log(1-U+e))) / tau)
 *   z      = hard ? (y_soft > 0.5) : y_soft
 *   kl_mean[0] = mean_rows sum_L KL(clamp(sigmoid(z)) || Bernoulli(p))
 * kl_mean may be NULL (encode path).  U may be NULL: the kernel then draws 24-bit uniforms from a
 * counter hash of (seed + *seed_dev, element index) -- device-side noise for the fused trainer. */
int rbvae_binarize_kl_fwd(const float* h, const float* U, float* y_soft, float* z, float* kl_mean,
                          int rows, int L, float tau, float noise_ratio, float noise_eps, int hard,
                          float kl_p, float kl_eps, int kl_clamp, unsigned long long seed,
                          const unsigned long long* seed_dev, void* stream);
/* The same over many workgroups (256 elements each): kl_parts[b] = sum over block b of the per-element KL terms,
 * b < rbvae_binarize_kl_nparts(rows, L); kl_mean = sum(kl_parts) / rows is left to rbvae_combine_losses.  The
 * one-workgroup form above is ALU-latency bound at the trainer's 256 x 32 logits; this one is not. */
int rbvae_binarize_kl_nparts(int rows, int L);
int rbvae_binarize_kl_fwd_parts(const float* h, const float* U, float* y_soft, float* z, float* kl_parts,
                                int rows, int L, float tau, const float* tau_dev, float noise_ratio, float noise_eps, int hard,
                                float kl_p, float kl_eps, int kl_clamp, unsigned long long seed,
                                const unsigned long long* seed_dev, void* stream);
/* dh (+)= (g_z + kl_weight * gscale * dKL/dz) * y_soft*(1-y_soft)/tau (straight-through when hard).
 * g_z may be NULL; gscale_dev (device scalar, may be NULL = 1) multiplies kl_weight.  kl_p outside (0,1) is refused
 * unless kl_weight == 0 (the KL term, and with it kl_p, is then not evaluated).
 * tau_dev (here and in every entry point that has it): when not NULL the kernel reads the temperature from that
 * device float instead of `tau`, so a captured HIP graph follows the reference's annealing schedule
 * (percep_RBVAE_train.py:424-437) without being re-captured. */
int rbvae_binarize_kl_bwd(const float* g_z, const float* y_soft, const float* z, float* dh, int accumulate,
                          int rows, int L, float tau, const float* tau_dev, float kl_weight, const float* gscale_dev,
                          float kl_p, float kl_eps, int kl_clamp, void* stream);

/* kl_binary_concrete as a free function (percep_RBVAE_train.py:52-76; simple
 * variant simple_RBVAE_train.py:45-68 = clamp 0, eps 1e-10).  Both refuse p outside (0,1). */
int rbvae_kl_fwd(const float* q_logits, float* out_mean, int rows, int L, float p, float eps, int clamp,
                 void* stream);
int rbvae_kl_bwd(const float* q_logits, float* dq, int rows, int L, float p, float eps, int clamp,
                 float scale, const float* gscale_dev, void* stream);

/* ---- pairwise-distance losses -------------------------------------------
 * contrast_loss 'euclidean' branch (percep_RBVAE_train.py:79-107):
 *   d = ||x1 - x2 + eps||_2 over L;  label 0: mean(d^2);  label 1: mean(max(margin-d,0)^2)
 * Rows are addressed as base + row*stride so h_seq[:, s] slices need no copy. */
int rbvae_pairdist_fwd(const float* x1, const float* x2, long stride1, long stride2, int rows, int L,
                       int label, float margin, float eps, float* out_mean, void* stream);
int rbvae_pairdist_bwd(const float* x1, const float* x2, long stride1, long stride2, int rows, int L,
                       int label, float margin, float eps, float scale, const float* gscale_dev,
                       float* dx1, float* dx2, long dstride1, long dstride2, int accumulate, void* stream);
/* contrast_loss 'cosine' branch (percep_RBVAE_train.py:94-96; never taken by the reference's trainers):
 *   d = 1 - x1.x2 / (max(|x1|, eps) * max(|x2|, eps)),  eps = 1e-8 (torch.nn.functional.cosine_similarity), then as above. */
int rbvae_paircos_fwd(const float* x1, const float* x2, long stride1, long stride2, int rows, int L, int label,
                      float margin, float eps, float* out_mean, void* stream);
int rbvae_paircos_bwd(const float* x1, const float* x2, long stride1, long stride2, int rows, int L, int label,
                      float margin, float eps, float scale, const float* gscale_dev, float* dx1, float* dx2, long dstride1,
                      long dstride2, void* stream);
/* The trainer's whole contrastive term in one launch (percep_RBVAE_train.py:534-543):
 *   mean_{b,t} d(h0,h1)^2 + 1/(T-1) sum_s mean_b max(1 - d(h0[:,s],h0[:,s+1]),0)^2, eps 1e-6.
 * h0,h1: [B,T,L] contiguous.  bwd WRITES dh0,dh1 (scale * d term/dh). */
int rbvae_contrast_term_fwd(const float* h0, const float* h1, int B, int T, int L, float* out, void* stream);
int rbvae_contrast_term_bwd(const float* h0, const float* h1, int B, int T, int L, float scale,
                            const float* gscale_dev, float* dh0, float* dh1, void* stream);
/* Value and gradient of that term in ONE many-workgroup launch: parts[2k], parts[2k+1] (k < contrast_term_nparts)
 * = per-block sums of d(h0,h1)^2 and of max(1 - d(h0[:,s],h0[:,s+1]),0)^2; the term is
 * sum(parts[2k])/(B*T) + sum(parts[2k+1])/(B*(T-1)) (rbvae_combine_losses finishes it); dh0/dh1 as the _bwd form. */
int rbvae_contrast_term_nparts(int B, int T);
int rbvae_contrast_term_fused(const float* h0, const float* h1, int B, int T, int L, float scale,
                              const float* gscale_dev, float* parts, float* dh0, float* dh1, void* stream);
/* F.triplet_margin_loss(p=2, eps, swap) (triplet_RBVAE_train.py:82-96) on strided rows.  Backward: the negative
 * pair's gradient goes to the smaller of d(a,n), d(p,n) and is split evenly when they are equal (torch.minimum). */
int rbvae_triplet_fwd(const float* a, const float* p, const float* n, long sa, long sp, long sn, int rows, int L,
                      float margin, float eps, int swap, float* out_mean, void* stream);
int rbvae_triplet_bwd(const float* a, const float* p, const float* n, long sa, long sp, long sn, int rows, int L,
                      float margin, float eps, int swap, float scale, const float* gscale_dev,
                      float* da, float* dp, float* dn, long dsa, long dsp, long dsn, int accumulate, void* stream);
/* The triplet trainer's term (triplet_RBVAE_train.py:461-468): anchor h0[:,s], positive
 * h1[:,s], negative h0[:,s+1], averaged over s < T-1; eps 1e-8, swap on. bwd WRITES. */
int rbvae_triplet_term_fwd(const float* h0, const float* h1, int B, int T, int L, float margin, float* out,
                           void* stream);
int rbvae_triplet_term_bwd(const float* h0, const float* h1, int B, int T, int L, float margin, float scale,
                           const float* gscale_dev, float* dh0, float* dh1, void* stream);

/* recon_loss = F.mse_loss (percep_RBVAE_train.py:32-33).  ws: >= rbvae_mse_ws_floats(n) floats. */
size_t rbvae_mse_ws_floats(long n);
int rbvae_mse_fwd(const float* a, const float* b, long n, float* out_mean, float* ws, void* stream);
int rbvae_mse_bwd(const float* a, const float* b, long n, float scale, const float* gscale_dev, float* da,
                  void* stream);

/* ---- row-gather GEMM on the matrix cores ---------------------------------------
 * Out[orow(m)][n] = epi( sum_{taps j} sum_{k<Kc} A[arow(m,j)][k] * W[n][widx_j][k] ), NHWC rows.
 * Replaces nn.Conv2d(k,2,1) forward (percep_RBVAE_model.py:51-57), nn.ConvTranspose2d(k,2,1,op)
 * forward (:76-82, as the conv's input gradient over 4 output-parity classes), the
 * backward-data passes of both (autograd of percep_RBVAE_train.py:552) and, with one tap,
 * the wide Linear products (:61,:74).
 *   m -> (n, a, b) over Nimg x TH x TW;  A pixel (a*sa+dh_j, b*sa+dw_j) of an IH x IW grid (zero
 *   outside);  Out pixel (a*so+oh0, b*so+ow0) of an OH x OW grid;  grid.z = parity class.
 *   class_desc is a HOST int array: per class [ntaps, oh0, ow0, ntaps x (widx, dh, dw)].
 *   epilogue: +bias, relu, *scale, dropout (drop_mode 1: counter hash of (seed, element index), 0 <= drop_p < 1;
 *   2: explicit u8 keep-mask [rows][Nout]), + addend (residual, same indexing as Out; LDM ResnetBlock /
 *   AttnBlock skip connections, ldm/modules/diffusionmodules/model.py:141,202), then zero where gate <= 0 (saved activation:
 *   ReLU/dropout backward).  zero_page: >= 128 zero bytes.  Kc % (128/sizeof T) == 0, Nout % 8 == 0.
 *   colsum_ws (optional, [nclass * ceil(rows/128)][Nout] f32): per-tile column sums of the stored
 *   values -- the bias gradient, finished by rbvae_reduce_rows. */
int rbvae_gather_gemm(int dtype, const void* A, const void* W, void* Out, const float* bias, const void* gate,
                      const void* mask, const void* addend, const void* zero_page, int Nimg, int IH, int IW, int TH, int TW, int sa,
                      int OH, int OW, int so, int Kc, int Nout, int lda, int ldo, int taps_total, int nclass,
                      const int* class_desc, int relu, int drop_mode, float drop_p, float scale,
                      unsigned long long seed, const unsigned long long* seed_dev, float* colsum_ws,
                      void* stream);

/* ---- 3x3 stride-2 pad-1 convolution with the input patch resident in LDS (bf16) -----------------------------------
 * Out[n][r][c][co] = epi( sum_{kh,kw,ci} A[n][2r + kh - 1][2c + kw - 1][ci] * W[co][kh*3 + kw][ci] ), NHWC rows, IH and IW even,
 * OH = IH / 2, OW = IW / 2: rbvae_gather_gemm's result for the one-class descriptor of nn.Conv2d(c, c, 3, 2, 1)
 * (percep_RBVAE_model.py:54-57; the conv-form input gradient of nn.ConvTranspose2d(c, c, 3, 2, 1, 1), :76-81, autograd as run by
 * percep_RBVAE_train.py:552; the LDM encoder's Downsample, ldm/modules/diffusionmodules/model.py:60-79), with the same
 * epilogue element for element (+bias, relu, *scale, dropout by key / mask with the same element indices, ReLU gate) --
 * but a workgroup stages the 17 x 33 input patch of its 8 x 16 output pixels ONCE per 32-channel slice for all nine taps
 * (9.7 KB through the CU's L2 -> LDS path per MFLOP at 256 output channels per workgroup instead of 15.2).
 * rbvae_conv3x3s2_halo_ok: output channels per workgroup (256 / 128) when covered (bf16, Kc % 32 == 0, Nout % 128 == 0,
 * even IH / IW, operands below 2 GiB), else 0.  colsum_ws (optional): [rbvae_conv3x3s2_halo_colsum_rows(..)][Nout] f32
 * column sums of the stored values per pixel tile -- the bias gradient, finished by rbvae_reduce_rows / a row-reduce job. */
int rbvae_conv3x3s2_halo_ok(int dtype, int Nimg, int IH, int IW, int Kc, int Nout);
int rbvae_conv3x3s2_halo_colsum_rows(int Nimg, int IH, int IW);
int rbvae_conv3x3s2_halo(int dtype, const void* A, const void* W, void* Out, const float* bias, const void* gate, const void* mask,
                         int Nimg, int IH, int IW, int Kc, int Nout, int lda, int ldo, int relu, int drop_mode, float drop_p,
                         float scale, unsigned long long seed, const unsigned long long* seed_dev, float* colsum_ws, void* stream);

/* ---- the K = 64 / 128 products around the latent bottleneck (bf16) -------------------------------
 * Out[M][ldo] = A[M][lda] (K used columns) * W[N][K]^T (+ bias[N]) for a few hundred rows and thousands of columns:
 * the decoder's fc forward (Linear(latent_dim -> C3*h3*w3), percep_RBVAE_model.py:74, on the zero-padded codes) and
 * the input gradient of the encoder's fc (autograd of :61).  The arithmetic of rbvae_gather_gemm with one tap,
 * element for element; operands go from global memory straight into the MFMA layout (no tables, no LDS ring).
 * colsum_ws (may be NULL): [ceil(M/128)][N] column sums of the stored values per 128-row tile (rbvae_gather_gemm's
 * layout; the bias gradient of the layer below).  rbvae_fc_gemm_ok: 1 when the shape is covered (bf16, K == 64 or
 * 128 = latent_dim padded to the GEMMs' 64-column slices, N % 16 == 0). */
int rbvae_fc_gemm_ok(int dtype, int M, int K, int N, int lda, int ldo);
int rbvae_fc_gemm(int dtype, const void* A, const void* W, void* Out, const float* bias, float* colsum_ws, int M, int K,
                  int N, int lda, int ldo, void* stream);

/* ---- weight-gradient GEMM ---------------------------------------------------------
 * dW[ks][co][t][ci] = sum over K-slice ks of Dy[p][co] * In[idx[t][p]][ci]  (f32 slabs, one per
 * K-slice; sum them with rbvae_permute_reduce).  idx = rbvae_conv_gather_index table or NULL
 * (identity, 1 tap: Linear).  in_rows = rows of In: an index outside [0, in_rows) reads the zero row, so a
 * wrong table can give wrong sums but never an out-of-bounds access.  Autograd of the Conv2d/ConvTranspose2d/Linear weights
 * (percep_RBVAE_model.py:51-61,74-82). */
int rbvae_conv_gather_index(int* idx, int Nimg, int IH, int IW, int OH, int OW, int KH, int KW, int stride,
                            int pad, void* stream);
int rbvae_wgrad_gemm(int dtype, const void* Dy, const void* In, float* dW_slabs, const int* idx,
                     const void* zero_page, int P, int in_rows, int Co, int Ci, int ldy, int ldi, int taps, int ksplit,
                     void* stream);

/* ---- weight gradient of the 3x3 stride-2 pad-1 convolutions, nine taps per workgroup (bf16) ----------------------
 * dW[ks][a][t][b] = sum over the K-slice's pixels p = (n, r, c) of S[p][a] * G[(n, 2r + kh - 1, 2c + kw - 1)][b],
 * t = 3 kh + kw, rows outside the image zero: rbvae_wgrad_gemm's sum for idx = rbvae_conv_gather_index(.., 3, 3, 2, 1)
 * and taps = 9, in the same slab layout (the same reduction jobs follow), with S and the 9 x 17 patch of G around a
 * 4 x 8 pixel block fetched once for all nine taps instead of once per tap.  Conv2d(c, c, 3, 2, 1) weights: S = the output
 * gradient [Nimg*OH*OW][lds], G = the layer's input [Nimg*2OH*2OW][ldg] (percep_RBVAE_model.py:51-57);
 * ConvTranspose2d(c, c, 3, 2, 1, 1) weights: S = the layer's input, G = its output gradient (:76-81); autograd as run by
 * percep_RBVAE_train.py:552.  Covered (rbvae_wgrad3x3s2_halo_ok): bf16, Ca and Cb multiples of 64.  K-slices are runs
 * of rbvae_wgrad3x3s2_halo_blocks(..) / ksplit pixel blocks; grid = (Ca/64) * (Cb/64) * ksplit workgroups (ksplit rounded up
 * to a multiple of 8: one K-slice group per XCD). */
int rbvae_wgrad3x3s2_halo_ok(int dtype, int Nimg, int OH, int OW, int Ca, int Cb);
int rbvae_wgrad3x3s2_halo_blocks(int Nimg, int OH, int OW);
int rbvae_wgrad3x3s2_halo(int dtype, const void* S, const void* G, float* dW_slabs, const void* zero_page, int Nimg, int OH,
                          int OW, int Ca, int Cb, int lds, int ldg, int ksplit, void* stream);

/* ---- the same sum for wide layers (Ca, Cb multiples of 128, bf16): the three taps of ONE kernel row per workgroup ------
 * A workgroup owns a 128 (a) x 128 (b) tile of the taps kw = 0, 1, 2 of one kh; per block of 64 low-resolution pixels the
 * [64][128] tile of S arrives once and of G the rows 2r + kh - 1 with their 2W + 1 columns (kw = 0 and kw = 2 share the odd
 * columns): 50 KB per 6.3 MFLOP instead of rbvae_wgrad_gemm's 96 KB (three taps, three workgroups).  Replaces
 * rbvae_wgrad_gemm for the 256-channel Conv2d(.., 3, 2, 1) / ConvTranspose2d(.., 3, 2, 1, 1) weights of
 * percep_RBVAE_model.py:54-57,76-81 (autograd as run by percep_RBVAE_train.py:552); same operands, same slab layout
 * [ksplit][Ca][9][Cb] and the same reduction jobs as rbvae_wgrad3x3s2_halo.  K-slices are balanced runs of the
 * rbvae_wgrad3x3s2_row_blocks(..) pixel blocks; grid = (Ca/128) * (Cb/128) * 3 * ksplit workgroups (rounded up to a multiple
 * of 8: every XCD takes a contiguous eighth of the (K-slice, tile) items). */
int rbvae_wgrad3x3s2_row_ok(int dtype, int Nimg, int OH, int OW, int Ca, int Cb);
int rbvae_wgrad3x3s2_row_blocks(int Nimg, int OH, int OW);
int rbvae_wgrad3x3s2_row(int dtype, const void* S, const void* G, float* dW_slabs, const void* zero_page, int Nimg, int OH,
                         int OW, int Ca, int Cb, int lds, int ldg, int ksplit, void* stream);

/* ---- layout helpers --------------------------------------------------------------
 * pack3:          out[i0*s0+i1*s1+i2*s2] = (T) in[i0][i1][i2]        (torch f32 weight -> packed T)
 * permute_reduce: out[i0][i1][i2] (+)= scale * sum_k in[k*slab+i0*s0+i1*s1+i2*s2]  (slabs -> torch grad)
 * cast_pad:       f32 [rows][L] -> T [rows][Lpad], zero padded
 * colsum:         out[C] (+)= scale * sum_p X[p][c]  (bias gradients); ws >= colsum_ws_floats */
int rbvae_pack3(int dtype, const float* in, void* out, int d0, int d1, int d2, long s0, long s1, long s2,
                void* stream);
int rbvae_permute_reduce(const float* in, int nslab, long slab_stride, float* out, int d0, int d1, int d2, long s0,
                         long s1, long s2, float scale, int accumulate, void* stream);
int rbvae_cast_pad(int dtype, const float* in, void* out, int rows, int L, int Lpad, void* stream);
int rbvae_reduce_rows(const float* ws, int rows, int C, float* out, float scale, int accumulate, void* stream);
/* first half of colsum: ws[ceil(P/rpb)][C] partial sums (rbvae_colsum_ws_floats(P, C) floats) */
int rbvae_colsum_partial(int dtype, const void* X, int P, int C, int ld, float* ws, void* stream);
size_t rbvae_colsum_ws_floats(int P, int C);
int rbvae_colsum(int dtype, const void* X, int P, int C, int ld, float* out, float* ws, float scale, int accumulate,
                 void* stream);

/* Batched layout jobs: njobs rows of 16 x int64 in DEVICE memory
 *   [type, src, dst, d0, d1, d2, s0, s1, s2, nslab, slab_stride, dtype, accumulate,
 *    scale (f32 bits, low word) | fast index (high word), inner, dst2]
 * type 0 = pack3, 1 = permute_reduce, 2 = reduce_rows (out[c] = scale*sum_k src[k*slab+c], c < d0*d1*d2),
 * 3 = conv weight pack: src f32 [d0=co][d1=ci][d2=kk<=16] -> dst [co][t][ci] and dst2 [ci][t][co] of `dtype`
 * (nn.Conv2d / nn.ConvTranspose2d weights, percep_RBVAE_model.py:51-57,76-82, in the two GEMM operand orders),
 * 4 = conv weight-gradient reduce: src = rbvae_wgrad_gemm's K-slice slabs [nslab][d0=co][d2=kk<=16][d1=ci] (f32,
 * ci % 4 == 0), summed in slab order into dst [co][ci][kk] (the torch layout of the weight; scale, accumulate honoured).
 * 5 = batch gather (rbvae_gather_frames as a job: src = table, dst = out, d0 = rows, d1 = n_batches, d2 = float4 per frame,
 * s0 = plan pointer, s1 = counter pointer or 0, s2 = table rows) -- shares the launch of the step's weight repack.
 * 6 / 7 = torch.optim.Adam update (percep_RBVAE_train.py:553) of one parameter tensor inside the job launch: src points
 * into the flat parameter buffer, `inner` holds a pointer to the optimiser context (8 x int64: w, g, m, v base pointers,
 * hyper pointer [lr/(1-b1^t), sqrt(1-b2^t)], then f32 pairs (1-b1, b2), (1-b2, eps), (gscale, 0)); kind 6 also writes the
 * tensor's packed copies from the new values: dst with strides (s0, s1, s2) in type dtype & 255 and optionally dst2 with
 * strides (nslab, slab, accumulate) in type dtype >> 8.  Kind 3 with `inner` set updates the conv weight rows it packs.
 * A table of these jobs is the optimiser step AND the weight repack of a training step in one launch.
 * fast: the logical index consecutive threads walk; inner != 0 (fast == 1, short d2): a thread walks d2 itself.
 * Kind 3's dtype is exactly RBVAE_F32 or RBVAE_BF16; fields a kind does not name above are not read by it.
 * The kinds are JOB_PACK .. JOB_ADAM (0 .. 7) in csrc/jobs.hip and symbols-from-video_amd/jobs.py, whose `Col` names the 16
 * positions in the order above.
 * One launch (grid.y = job) replaces the per-tensor launches of a step. */
int rbvae_run_jobs(const void* jobs_dev, int njobs, int blocks_per_job, void* stream);
/* The same table launched with exactly the workgroups its jobs can use (a step's update launch: ~1 400 instead of 49 x 256).
 * rbvae_job_block_map (host): for the njobs rows at rows_host (host copy of the table) write map_host[4 * b] = (job, index of
 * workgroup b within its job, workgroups of the job <= max_blocks_per_job, 0) and return the number of workgroups (with
 * map_host == NULL: only count them); negative = error.  rbvae_run_jobs_sized: block_map_dev = that map in device memory
 * (16-byte aligned), total_blocks = its entries. */
int rbvae_job_block_map(const long* rows_host, int njobs, int max_blocks_per_job, int* map_host, int map_capacity);
int rbvae_run_jobs_sized(const void* jobs_dev, const void* block_map_dev, int total_blocks, void* stream);
/* The sized launch with its LDS taken from the table itself.  rbvae_run_jobs and rbvae_run_jobs_sized give every workgroup
 * the largest tile any job can need (36 992 bytes).  rbvae_run_jobs_table takes the host copy of the rows (rows_host,
 * njobs, max_blocks_per_job: what rbvae_job_block_map built block_map_dev from) next to the device rows and map, and works
 * out from the rows, inside the library, the workgroups (rbvae_job_block_map's count) and the dynamic LDS
 * (rbvae_job_lds_bytes).  Results are bit for bit those of rbvae_run_jobs_sized.  order_dev: NULL, or
 * rbvae_job_launch_order's permutation in device memory -- workgroup b then takes map entry order[b], so that the jobs
 * with the most bytes per workgroup start first and the one-workgroup jobs fill the slots they leave (a step's update
 * launch: 1 647 workgroups, 1 024 resident at a time).
 * rbvae_job_lds_bytes (host): the most LDS a job of the table touches, rounded up to 16 bytes; negative = error.
 * rbvae_job_launch_order (host): order_host[b] = a permutation of the map's entries, the jobs by falling bytes per
 * workgroup (ties in table order), each job's entries in their own order; a pure function of the rows; returns the
 * number of entries, negative = error. */
int rbvae_job_lds_bytes(const long* rows_host, int njobs);
int rbvae_job_launch_order(const long* rows_host, int njobs, int max_blocks_per_job, int* order_host, int capacity);
int rbvae_run_jobs_table(const long* rows_host, int njobs, int max_blocks_per_job, const void* jobs_dev,
                         const void* block_map_dev, const void* order_dev, void* stream);

/* im2col of a strided f32 image (element strides sn,sc,sh,sw) into col[N*OH*OW][Kpad], column
 * (kh*KW+kw)*C + c: the 3/4-channel first Conv2d (percep_RBVAE_model.py:51) and the last
 * ConvTranspose2d's backward run as plain GEMMs on it. */
int rbvae_im2col(int dtype, const float* src, long sn, long sc, long sh, long sw, int N, int C, int IH, int IW,
                 int OH, int OW, int KH, int KW, int stride, int pad, int Kpad, void* col, void* stream);
/* The first Conv2d(3x3, stride 2, pad 1; Cin <= 4 -> Nout <= 256) + bias + ReLU + Dropout (percep_RBVAE_model.py:51-53)
 * as ONE kernel, bf16: rbvae_im2col_frames (col [N*OH*OW][64] is written for rbvae_wgrad_gemm unless col == NULL) + the
 * single-slice rbvae_gather_gemm, with the patch gathered in LDS and results stored from the accumulators.  W is the
 * packed [Nout][64] im2col-order weight; x frames f32 [Cin][IH][IW] through the frame map (fd1 == 0: frame n at
 * n*fs2); drop_mode 0 / 1 with rbvae_gather_gemm's key and element indices. */
int rbvae_conv_first_fused_ok(int dtype, int Cin, int IH, int IW, int Nout, int N);
int rbvae_conv_first_fused(int dtype, const float* x, int fd1, int fd2, long fs0, long fs1, long fs2, const void* W,
                           const float* bias, const void* zero_page, void* col, void* out, int N, int Cin, int IH, int IW,
                           int Nout, int ldo, int relu, int drop_mode, float drop_p, float scale, unsigned long long seed,
                           const unsigned long long* seed_dev, void* stream);
/* Input gradient of the last ConvTranspose2d (autograd of percep_RBVAE_model.py:82; k3 s2 p1) as ONE kernel, bf16: the
 * 3x3 stride-2 convolution of dpre [N][OH][OW][Cout] f32 (rbvae_deconv_last_fused's d(loss)/d(pre-sigmoid)) with the packed
 * weight W [C1][64] (column (kh*3+kw)*Cout + co), times scale, kept where gate [rows][ldo] (the stored ReLU/dropout output
 * of the layer below) is > 0 -- rbvae_im2col + the single-slice rbvae_gather_gemm, bit-identical stored values.  col
 * [rows][64] receives the im2col rows (the last deconv's weight gradient reads them); colsum_ws
 * [rbvae_deconv_last_dgrad_blocks][C1] (optional) the per-workgroup column sums of the stored output (bias gradient of
 * the layer below).  rows = N * ceil(OH/2) * ceil(OW/2). */
int rbvae_deconv_last_dgrad_blocks(int dtype, int Cout, int OH, int OW, int C1, int N);
int rbvae_deconv_last_dgrad_fused(int dtype, const float* dpre, const void* W, const void* zero_page, void* col,
                                  const void* gate, void* out, int N, int Cout, int OH, int OW, int C1, int ldo, float scale,
                                  float* colsum_ws, void* stream);

/* Weight gradient of those two layers WITHOUT the im2col rows: dW[ks][co][k] = sum over the K-slice's output pixels p of
 * dY[p][co] * col(x)[p][k], k = (kh*3+kw)*Cin + ci zero padded to 64 -- rbvae_wgrad_gemm's sums over the [rows][64] im2col rows
 * (one tap), in its slab layout [ksplit][Nout][64], with the rows rebuilt in LDS from the 3/4-channel image instead of read
 * back (128 bytes per pixel for 12-16 bytes of image).  mode 0: x = the input frames through the frame map (as
 * rbvae_conv_first_fused), dY = the gradient at the first Conv2d's output (percep_RBVAE_model.py:51, autograd as run by
 * percep_RBVAE_train.py:552); mode 1: x = d(loss)/d(pre-sigmoid) [N][IH][IW][Cin] f32, dY = the stored activation in front of
 * the last ConvTranspose2d (:82).  With it the two kernels above take col = NULL.  K-slices are runs of
 * rbvae_wgrad_first_blocks(..) / ksplit blocks of 8 x 16 output pixels; grid = (Nout / 64) * ksplit workgroups. */
int rbvae_wgrad_first_blocks(int dtype, int Cin, int IH, int IW, int Nout, int N);
int rbvae_wgrad_first(int dtype, int mode, const float* x, int fd1, int fd2, long fs0, long fs1, long fs2, const void* dY,
                      float* dW_slabs, const void* zero_page, int N, int Cin, int IH, int IW, int Nout, int ldy, int ksplit,
                      void* stream);
/* Last ConvTranspose2d + Sigmoid (percep_RBVAE_model.py:82-83) fused with recon_loss
 * (percep_RBVAE_train.py:32-33): Y[(n,a,b)][t*Cout+co] = per-tap products; gathers them (col2im),
 * adds bias, applies sigmoid, writes x_recon NCHW f32; with target: sse_mean[0] = mse and
 * dpre[n][oh][ow][co] = gscale*gscale_dev*(xr-x)*xr*(1-xr).  ws >= col2im_ws_floats floats.
 * sse_mean == NULL with ws and target given: the rbvae_col2im_nparts(N*OH*OW*Cout) per-block partial sums of
 * squared error stay in ws for rbvae_combine_losses to finish (one launch fewer per training step). */
size_t rbvae_col2im_ws_floats(void);
int rbvae_col2im_nparts(long n_out);
/* 1 when the call (with target, ws and a 16-byte aligned dpre) also leaves per-block column sums of dpre -- the
 * last deconv's bias gradient -- at ws[nparts + 4*b + c], b < nparts, c < Cout (Cout <= 4, < 2^31 outputs). */
int rbvae_col2im_has_dcol(int N, int IH, int IW, int ldy, int OH, int OW, int Cout);
int rbvae_col2im_sigmoid(int dtype, const void* Y, int ldy, const float* bias, int N, int IH, int IW, int OH,
                         int OW, int Cout, int KH, int KW, int pad, float* xr, const float* target,
                         float* sse_mean, float* ws, float* dpre, float gscale, const float* gscale_dev,
                         void* stream);
/* The same with the frames addressed through a map instead of one stride: frame n starts at element
 * (n / fd1) * fs0 + ((n % fd1) / fd2) * fs1 + (n % fd2) * fs2 of src / target.  The fused trainer reads an item
 * batch [B][2][T][C][H][W] (percep_RBVAE_train.py:509-526: x_t = item[:, 0], x_t1 = item[:, 1]) as the 2B
 * sequences "all of view 0, then all of view 1" with fd1 = B*T, fd2 = T, fs0 = T*CHW, fs1 = 2*T*CHW, fs2 = CHW,
 * without first copying it into that order. */
int rbvae_im2col_frames(int dtype, const float* src, int fd1, int fd2, long fs0, long fs1, long fs2, long sc, long sh,
                        long sw, int N, int C, int IH, int IW, int OH, int OW, int KH, int KW, int stride, int pad,
                        int Kpad, void* col, void* stream);
int rbvae_col2im_sigmoid_frames(int dtype, const void* Y, int ldy, const float* bias, int N, int IH, int IW, int OH,
                                int OW, int Cout, int KH, int KW, int pad, float* xr, const float* target, int fd1,
                                int fd2, long fs0, long fs1, long fs2, float* sse_mean, float* ws, float* dpre,
                                float gscale, const float* gscale_dev, void* stream);
/* The same layer as ONE kernel (bf16, Cout <= 4, C1 % 64 == 0): per-tap products on the matrix cores from an
 * LDS-resident 9x17-pixel block of D2 [N*IH*IW][C1] and V [NYP][C1] (row = tap*Cout + co), f32 products kept in LDS,
 * then the gather / bias / sigmoid / squared error / d(loss)/d(pre) of rbvae_col2im_sigmoid_frames.  ws receives
 * `parts` squared-error sums and, behind them, parts x 4 column sums of dpre (parts = rbvae_deconv_last_fused_parts,
 * 0 = shape not covered: use rbvae_gather_gemm + rbvae_col2im_sigmoid_frames).  fd1 == 0: frames at n*fs2. */
int rbvae_deconv_last_fused_parts(int dtype, int N, int IH, int IW, int C1, int Cout);
int rbvae_deconv_last_fused(int dtype, const void* D2, const void* V, int NYP, const float* bias, const void* zero_page,
                            int N, int IH, int IW, int C1, int Cout, float* xr, const float* target, int fd1, int fd2,
                            long fs0, long fs1, long fs2, float* ws, float* dpre, float gscale, void* stream);
/* rbvae_deconv_last_fused followed by rbvae_deconv_last_dgrad_fused as ONE launch (bf16, Cout <= 4, C1 % 64 == 0,
 * C1 <= 256; target, ws and dpre required): a workgroup stages its 8x16 block of D2 (plus a one-pixel halo all round)
 * through LDS once, keeps the block's ReLU gate as bits, leaves xr, ws (parts + 4 x parts, as rbvae_deconv_last_fused_parts defines) and dpre exactly as the first call
 * does, recomputes dpre on the block's low-side rim instead of reading a neighbour's, and from the dpre patch in LDS
 * leaves dd2 [N*IH*IW][C1] (W [C1][64] the packed weight of the second call, times gs, kept where D2 > 0), the im2col rows
 * col [N*IH*IW][64] (NULL: not written) and colsum_ws [rbvae_deconv_last_dgrad_blocks][C1] exactly as the second call
 * does.  Every value and every partial sum is equal bit for bit to the two launches'.  _ok: 1 when the shape is covered. */
int rbvae_deconv_last_fwd_bwd_ok(int dtype, int N, int IH, int IW, int C1, int Cout);
int rbvae_deconv_last_fwd_bwd(int dtype, const void* D2, const void* V, int NYP, const void* W, const float* bias,
                              const void* zero_page, int N, int IH, int IW, int C1, int Cout, float* xr, const float* target,
                              int fd1, int fd2, long fs0, long fs1, long fs2, float* ws, float* dpre, float gscale, void* col,
                              void* dd2, float gs, float* colsum_ws, void* stream);
int rbvae_sigmoid_bwd_nhwc(const float* g_nchw, const float* xr_nchw, float* dpre_nhwc, int N, int C, int H, int W,
                           void* stream);
/* Linear with few outputs (percep_RBVAE_model.py:61 forward; :74 backward-data):
 * out[M][Nc] f32 = A[M][K] * B[Nc][K]^T + bias. */
int rbvae_skinny_linear(int dtype, const void* A, const void* B, const float* bias, float* out, int M, int Nc,
                        int K, int lda, int ldb, int ldo, void* stream);
/* K split over `ksplit` workgroup groups (the one-group form keeps 32 CUs busy at M = 256): slab q =
 * out_parts + q*M*ldo holds the partial product over K range q (+ bias in slab 0); the consumer sums the slabs. */
int rbvae_skinny_linear_parts(int dtype, const void* A, const void* B, const float* bias, float* out_parts, int M,
                              int Nc, int K, int lda, int ldb, int ldo, int ksplit, void* stream);

/* ---- stacked LSTM (percep_RBVAE_model.py:94-122) ------------------------------------
 * wblk: per layer w_ih[4L][L], w_hh[4L][L], b_ih[4L], b_hh[4L] (the reference's registration
 * order).  hs_all [layers+1][S][T][L]: slot 0 = input (caller fills), slot l+1 = layer l output.
 * Training also saves hprev/cs [layers][S][T][L] and acts [layers][S][T][4L].
 * wT (optional): transposed weight copies [layers][ih|hh][L][4L] for coalesced loads. */
int rbvae_lstm_fwd(const float* wblk, const float* wT, float* hs_all, float* hprev, float* acts, float* cs, int S,
                   int T, int L, int layers, void* stream);
int rbvae_lstm_bwd(const float* wblk, const float* wT, const float* acts, const float* cs, const float* g_top, float* dG,
                   float* dx, int S, int T, int L, int layers, void* stream);
/* Kernels by size: L <= 32 -- one thread group per LAYER with its weight rows in registers, cells along anti-diagonals
 * (T + layers - 1 dependent steps); 32 < L <= 128 (the reference's latent_dim 50 / 75 / 100, best_models.txt) -- layer by
 * layer, a gate row shared by two lanes (eight lanes per hidden unit in the backward pass), the input half W_ih x_t of
 * every time step computed in one batch off the dependent chain. */
/* rbvae_lstm_fwd_wave_ok / rbvae_lstm_bwd_wave_ok: 1 when the wavefront kernel serves the shape -- L <= 32,
 * layers * roundup64(4L) <= 1024, and the sequence's state within 64 KB of LDS: (layers+1)*T*L + layers*4L floats forward,
 * T*L + layers*(5*T*L + 12L) backward (at L = 32 with 4 layers: T <= 99 forward, T <= 22 backward).  The dispatchers ask
 * these functions themselves; longer sequences run layer by layer (plain rbvae_lstm_fwd / _bwd only). */
int rbvae_lstm_fwd_wave_ok(int T, int L, int layers);
int rbvae_lstm_bwd_wave_ok(int T, int L, int layers);
/* Extended forms that take over the small kernels around the stacks (wavefront kernel only: rbvae_lstm_fwd_wave_ok /
 * rbvae_lstm_bwd_wave_ok, else RBVAE_E_INVALID):
 *  - in_parts / g_top_parts: the stack input (forward) / top-layer gradient (backward) as `nparts` K-split slabs of
 *    the fc product that feeds them (rbvae_skinny_linear_parts; slab q at + q*part_stride floats), summed in slab
 *    order in the kernel's prologue; the forward also writes the sum to slot 0 of hs_all.  in_parts NULL /
 *    nparts 1: plain input as in rbvae_lstm_fwd / _bwd;
 *  - cast_out (may be NULL): the top layer's outputs (forward) / the input gradient dx (backward) once more as
 *    [S*T][cast_ld] rows of cast_dtype, zero padded -- the operand of the GEMM that follows (rbvae_cast_pad);
 *  - dx_colsum (backward, may be NULL): [S][L] per-sequence sums over t of dx -- summed over S they are the bias
 *    gradient of the Linear that feeds the stack (percep_RBVAE_model.py:61). */
int rbvae_lstm_fwd_ex(const float* wblk, const float* wT, float* hs_all, float* hprev, float* acts, float* cs, int S,
                      int T, int L, int layers, const float* in_parts, int nparts, long part_stride, void* cast_out,
                      int cast_dtype, int cast_ld, void* stream);
int rbvae_lstm_bwd_ex(const float* wblk, const float* acts, const float* cs, const float* g_top_parts, int nparts,
                      long part_stride, float* dG, float* dx, void* cast_out, int cast_dtype, int cast_ld,
                      float* dx_colsum, int S, int T, int L, int layers, void* stream);
/* Encoder stack -> binary_concrete_logits -> decoder stack (percep_RBVAE_model.py:155-163) as ONE wavefront
 * launch: the arithmetic of rbvae_lstm_fwd(enc) + rbvae_binarize_kl_fwd_parts + rbvae_lstm_fwd(dec), with the same
 * optional slab input / cast output as the _ex forms.  hs_dec slot 0 receives z; kl_parts[s] (may be NULL) = KL sum
 * of sequence s (S parts; mean = sum / (S*T)).  rbvae_lstm_pair_fwd_ok tells whether the shape is covered
 * (L <= 32, 2 * layers * roundup64(4L) <= 1024). */
int rbvae_lstm_pair_fwd_ok(int T, int L, int layers);
int rbvae_lstm_pair_fwd(const float* wblk_enc, const float* wT_enc, const float* wblk_dec, const float* wT_dec,
                        float* hs_enc, float* hprev_enc, float* acts_enc, float* cs_enc, float* hs_dec,
                        float* hprev_dec, float* acts_dec, float* cs_dec, const float* in_parts, int nparts,
                        long part_stride, const float* U, float* y_soft, float* kl_parts, float tau, const float* tau_dev,
                        float noise_ratio, float noise_eps, int hard, float kl_p, float kl_eps, int kl_clamp, unsigned long long seed,
                        const unsigned long long* seed_dev, void* cast_out, int cast_dtype, int cast_ld, int S, int T,
                        int L, int layers, void* stream);
/* The encoder stack's BPTT with rbvae_binarize_kl_bwd fused into its prologue (wavefront kernel only):
 *   g_top = g_hs + (g_z + kl_weight/(S*T) * dKL/dz(z)) * y_soft*(1-y_soft)/tau,   g_hs may be NULL;
 * cast_out / dx_colsum as in rbvae_lstm_bwd_ex. */
int rbvae_lstm_bwd_bin(const float* wblk, const float* acts, const float* cs, const float* g_z, const float* y_soft,
                       const float* z, const float* g_hs, float tau, const float* tau_dev, float kl_weight, float kl_p, float kl_eps,
                       int kl_clamp, float* dG, float* dx, void* cast_out, int cast_dtype, int cast_ld, float* dx_colsum,
                       int S, int T, int L, int layers, void* stream);
/* Both stacks' BPTT as ONE wavefront launch (autograd of percep_RBVAE_model.py:155-163 as run by
 * percep_RBVAE_train.py:552): rbvae_lstm_bwd_ex(decoder stack) -> rbvae_binarize_kl_bwd -> rbvae_lstm_bwd_ex(encoder
 * stack), T + 2*layers - 1 dependent steps instead of 2 * (T + layers - 1).  The decoder stack's input gradient (the
 * gradient of the codes) never leaves the chip; dz (may be NULL) receives a copy, gz_extra (may be NULL) is a second
 * gradient of the codes added to it before the binarise backward.  Everything else as in rbvae_lstm_bwd_ex /
 * rbvae_lstm_bwd_bin.  rbvae_lstm_pair_bwd_ok tells whether the shape is covered (L <= 32,
 * 2 * layers * roundup64(4L) <= 1024, saved gates of both stacks within 64 KB of LDS). */
int rbvae_lstm_pair_bwd_ok(int T, int L, int layers);
int rbvae_lstm_pair_bwd(const float* wblk_enc, const float* wblk_dec, const float* acts_enc, const float* cs_enc,
                        const float* acts_dec, const float* cs_dec, const float* g_top_parts, int nparts, long part_stride,
                        const float* gz_extra, const float* y_soft, const float* z, const float* g_hs, float tau,
                        const float* tau_dev, float kl_weight, float kl_p, float kl_eps, int kl_clamp, float* dG_enc,
                        float* dG_dec, float* dx, float* dz, void* cast_out, int cast_dtype, int cast_ld, float* dx_colsum,
                        int S, int T, int L, int layers, void* stream);
int rbvae_lstm_wgrad(const float* dG, const float* hs_all, const float* hprev, float* gblk, int S, int T, int L,
                     int layers, int accumulate, void* stream);
/* the same for two stacks of equal shape (the encoder and decoder LSTMs) in one launch */
int rbvae_lstm_wgrad_pair(const float* dG_a, const float* hs_a, const float* hprev_a, float* gblk_a, const float* dG_b,
                          const float* hs_b, const float* hprev_b, float* gblk_b, int S, int T, int L, int layers,
                          int accumulate, void* stream);

/* The trainer's DataLoader + item.to(device) (percep_RBVAE_train.py:509-518, ShuffledStatePairDataset.__getitem__
 * :312-360) for a latent table resident in HBM: out[r] = table[plan[batch][r]] for r < rows, frames of frame_elems
 * floats; plan is [n_batches][rows] table rows (int64, the epoch's shuffled batches laid out in advance) and
 * batch = *counter_dev % n_batches (the device step counter: the gather can sit inside the captured step graph) or 0. */
int rbvae_gather_frames(const float* table, long table_rows, const long* plan, int rows, int n_batches,
                        const unsigned long long* counter_dev, long frame_elems, float* out, void* stream);

/* The majority vote of calculate_state_consistency (percep_RBVAE_train.py:473-497: np.unique(axis=0, return_counts) +
 * argmax per state) on the device: codes [F][L] (binary, L <= 128) are packed to 128-bit keys (element 0 most
 * significant: key order = np.unique's row order, ties go to the smallest), out[s] = {frames of state s that carry the
 * state's most common code, frames of state s}.  labels [F] int32 in [0, n_states); keys_ws: 16 F bytes (16-byte
 * aligned), counts_ws: F ints. */
int rbvae_state_vote(const float* codes, const int* labels, int F, int L, int n_states, void* keys_ws, int* counts_ws,
                     int* out, void* stream);

/* torch.optim.Adam defaults (percep_RBVAE_train.py:753,553) on a flat f32 buffer; g is scaled by gscale
 * first.  The step number comes from `step` or, when step_dev != NULL, from a device counter that the call
 * first ADVANCES by one (then hyper_ws, 2 floats, receives the bias-correction terms): graph-replay safe.
 * step_dev == NULL with hyper_ws != NULL: hyper_ws already holds the terms (rbvae_combine_losses prepared them). */
int rbvae_adam_step(float* w, const float* g, float* m, float* v, long n, double lr, double beta1, double beta2,
                    double eps, int step, float gscale, unsigned long long* step_dev, float* hyper_ws,
                    void* stream);
/* The trainer's scalar bookkeeping in one launch (percep_RBVAE_train.py:531-549):
 * out4 = [recon + beta*kl + alpha*pair, recon, kl, pair]; recon from `recon` or, when sse_ws != NULL,
 * finished here as inv_n * sum(sse_ws[0..nparts)) (the col2im kernel's partial sums); kl = kl[0] or, when
 * kl_parts > 0, kl_scale * sum(kl[0..kl_parts)) (rbvae_binarize_kl_fwd_parts' per-block sums); pair = pair[0]
 * or, when pair_parts > 0, w_sim * sum(pair[2i]) + w_dis * sum(pair[2i+1]) (rbvae_contrast_term_fused).
 * step_dev != NULL: also advances the device step counter and leaves Adam's bias-correction terms for that step
 * in hyper_ws (2 floats); rbvae_adam_step(step_dev = NULL, hyper_ws) then uses them without a launch of its own.
 * lr_dev != NULL: the learning rate is read from that device double (a captured graph follows an lr schedule). */
int rbvae_combine_losses(const float* sse_ws, int nparts, float inv_n, const float* recon, const float* kl,
                         int kl_parts, float kl_scale, const float* pair, int pair_parts, float w_sim, float w_dis,
                         float beta, float alpha, float* out4, unsigned long long* step_dev, double lr,
                         const double* lr_dev, double beta1, double beta2, float* hyper_ws, void* stream);

/* ---- frozen LDM / Stable-Diffusion VAE encoder (cfg 5: on-the-fly latents) ------------------------
 * The convolutions, 1x1 projections and both attention products run on rbvae_gather_gemm (stride-1 and
 * asymmetric-pad stride-2 tap tables, residuals through `addend`); these are the remaining pieces.
 * GroupNorm(32, eps 1e-6, affine) + swish: src/stable-diffusion/ldm/modules/diffusionmodules/model.py:33-39
 * (stats_ws: 2*N*groups floats).  softmax_rows: AttnBlock :186-192.  posterior_sample:
 * ldm/modules/distributions/distributions.py:24-37 with ldm/models/diffusion/ddpm.py:542-549's scale:
 * latent[n][c][h][w] f32 = scale * (mean + exp(0.5*clamp(logvar,-30,20)) * eps); eps NULL = posterior mode. */
int rbvae_groupnorm_swish(int dtype, const void* x, void* y, const float* gamma, const float* beta, float* stats_ws,
                          int N, int HW, int C, int ldx, int ldy, int groups, float eps, int swish, void* stream);
/* The same with a workspace of rbvae_groupnorm_ws_floats(...) floats: statistics then come from whole pixel rows
 * (16-byte loads, per-block (mean, M2) merged by the parallel-variance formula) instead of one workgroup walking
 * an (image, group) twice; needs C % 8 == 0 (bf16) / C % 4 == 0 (f32) and 16-byte aligned rows, else falls back. */
size_t rbvae_groupnorm_ws_floats(int dtype, int N, int HW, int C, int groups);
int rbvae_groupnorm_swish_ws(int dtype, const void* x, void* y, const float* gamma, const float* beta, float* stats_ws,
                             size_t ws_floats, int N, int HW, int C, int ldx, int ldy, int groups, float eps, int swish,
                             void* stream);
/* the statistics alone (no normalised copy): mean = stats_ws[0 : N*groups], rstd = stats_ws[N*groups : 2*N*groups];
 * rbvae_gn_affine turns them into the scale / shift rbvae_conv3x3_halo applies while it stages its input. */
int rbvae_groupnorm_stats(int dtype, const void* x, float* stats_ws, size_t ws_floats, int N, int HW, int C, int ldx,
                          int groups, float eps, void* stream);
/* the apply pass alone from given statistics (e.g. rbvae_gn_finish_tiles' mean_out / rstd_out): for convolutions with
 * four or more 128-channel output tiles one standalone pass costs less than re-normalising the patch in every tile. */
int rbvae_groupnorm_apply(int dtype, const void* x, void* y, const float* mean, const float* rstd, const float* gamma,
                          const float* beta, int N, int HW, int C, int ldx, int ldy, int groups, int swish, void* stream);
int rbvae_softmax_rows(int dtype, const void* x, void* y, long rows, int n, int ld, void* stream);
/* AttnBlock.forward's q k^T * C^-0.5 -> softmax -> . v (ldm/modules/diffusionmodules/model.py:186-198) for N images
 * of hw tokens x C channels as ONE batched, tiled, online-softmax kernel: the hw x hw scores are never materialised.
 * Q, K, V, O: NHWC rows [N*hw][ld*] (may be column blocks of one fused q|k|v projection).  rbvae_attention_ok tells
 * whether the shape is covered (bf16, hw % 32 == 0, C in {64,128,256,512}); otherwise use the three-launch form
 * (rbvae_gather_gemm + rbvae_softmax_rows + rbvae_transpose2d). */
int rbvae_attention_ok(int dtype, int hw, int C);
int rbvae_attention(int dtype, const void* Q, const void* K, const void* V, void* O, int N, int hw, int C, int ldq,
                    int ldk, int ldv, int ldo, float scale, void* stream);
int rbvae_transpose2d(int dtype, const void* in, void* out, int R, int C, int ldi, int ldo, void* stream);
int rbvae_posterior_sample(int dtype, const void* moments, int ld, const float* eps, float* latent, int N, int Z,
                           int HW, float scale, void* stream);

/* ---- halo-resident 3x3 convolution, stride 1 (csrc/conv_halo.hip) ---------------------------------
 * The ResnetBlock / conv_out convolutions of the LDM encoder (ldm/modules/diffusionmodules/model.py:82-141, 368-459:
 * torch.nn.Conv2d(cin, cout, 3, 1, 1)) with the 18 x 18 input patch of a 16 x 16 pixel tile staged in LDS once per
 * 128-byte channel slice and shared by all nine taps (rbvae_gather_gemm re-gathers it per tap).
 *   Out[n][oh][ow][co] = bias[co] + addend + sum_{kh,kw,ci} f(A[n][oh+kh-pad_h][ow+kw-pad_w][ci]) * W[co][kh*3+kw][ci]
 * A / Out / addend NHWC rows of the storage type, W packed [Nout][9][Kc] (rbvae_pack3), zero_page >= 128 zero bytes.
 * f = identity, or with gn_scale / gn_shift ([Nimg][Kc] f32, from rbvae_gn_finish_tiles / rbvae_gn_affine) the
 * producer's GroupNorm (+ swish when gn_swish) applied while the patch is staged: model.py:38-39 + :33-35 as called at
 * :121-131 -- x -> swish(x * scale + shift); padding pixels stay zero (the reference pads AFTER the normalisation).
 * stats_part (may be NULL; rbvae_conv3x3_halo_stats_floats floats): per pixel tile and group of stats_cg output channels
 * the (mean, sum of squared deviations) of the STORED values (after bias / addend), which rbvae_gn_finish_tiles merges
 * into the next GroupNorm's statistics -- the consumer's normalisation costs no pass over the activation.
 * rbvae_conv3x3_halo_ok: 1 when the shape is covered (OW >= 16, OH >= 8, Kc % 64 (bf16) / 32 (f32) == 0, Nout % 128 == 0);
 * other shapes run on rbvae_gather_gemm. */
int rbvae_conv3x3_halo_ok(int dtype, int IH, int IW, int OH, int OW, int Kc, int Nout);
int rbvae_conv3x3_halo(int dtype, const void* A, const void* W, void* Out, const float* bias, const void* addend,
                       const void* zero_page, const float* gn_scale, const float* gn_shift, int gn_swish,
                       float* stats_part, int stats_cg, int Nimg, int IH, int IW, int OH, int OW, int pad_h, int pad_w,
                       int Kc, int Nout, int lda, int ldo, void* stream);
size_t rbvae_conv3x3_halo_stats_floats(int Nimg, int OH, int OW, int Nout, int cg);
/* GroupNorm(groups, eps, affine) statistics -> the per-(image, channel) scale / shift rbvae_conv3x3_halo applies
 * (model.py:38-39): from the producing convolution's per-tile partials (gn_finish_tiles; mean_out / rstd_out [Nimg*groups]
 * optional), or from the mean / rstd of rbvae_groupnorm_swish_ws's statistics kernels (gn_affine). */
int rbvae_gn_finish_tiles(const float* stats_part, const float* gamma, const float* beta, float* scale, float* shift,
                          float* mean_out, float* rstd_out, int Nimg, int OH, int OW, int C, int groups, float eps,
                          int tile_h, int tile_w, void* stream);   /* tile: 16 x 16 (rbvae_conv3x3_halo), 8 x 16 (rbvae_conv_in) */
/* The LDM encoder's conv_in, Conv2d(Cin <= 4 -> Nout <= 256, 3x3, stride 1, pad 1) on f32 NCHW frames (model.py:385-389,
 * :436), as ONE kernel in bf16 storage -- rbvae_im2col + the one-tap rbvae_gather_gemm, the same 64-deep MFMA chain per
 * output -- with the GroupNorm partial statistics of its output out of the epilogue: stats_part (may be NULL;
 * rbvae_conv_in_stats_floats floats) receives per 8 x 16 pixel tile and group of cg (4, 8 or 16) channels the (mean, sum of
 * squared deviations) of the stored values, merged by rbvae_gn_finish_tiles(.., 8, 16).  W [Nout][64] bf16, column
 * (kh*3+kw)*Cin + ci zero padded; out [N*H*W][ldo] bf16. */
int rbvae_conv_in_ok(int dtype, int Cin, int H, int W, int Nout, int N, int cg);
size_t rbvae_conv_in_stats_floats(int N, int H, int W, int Nout, int cg);
int rbvae_conv_in(int dtype, const float* x, const void* W, const float* bias, const void* zero_page, void* out, float* stats_part,
                  int cg, int N, int Cin, int H, int Wd, int Nout, int ldo, void* stream);
int rbvae_gn_affine(const float* mean, const float* rstd, const float* gamma, const float* beta, float* scale,
                    float* shift, int N, int C, int groups, void* stream);

/* ---- halo-resident transposed 3x3 convolution, stride 2 (csrc/deconv_halo.hip) --------------------------
 * ConvTranspose2d(cin, cout, 3, stride 2, padding 1, output_padding 1) forward of the RBVAE decoder
 * (models/percep_RBVAE/percep_RBVAE_model.py:76-81) and, with the data-gradient weight order, the input gradient of
 * the encoder's Conv2d(3, stride 2, padding 1) (autograd of :54-57 under total_loss.backward(), percep_RBVAE_train.py:552):
 * the four output-parity classes of rbvae_gather_gemm's "dgrad" descriptor in ONE workgroup per 128 (two workgroups per
 * CU) or 256 input-grid positions x 64 output channels, the input patch staged in LDS once per channel slice and shared by the nine taps.
 *   A [Nimg*TH*TW][lda] (the TH x TW input grid), Out [Nimg*2TH*2TW][ldo], W packed [Nout][9][Kc] (tap index kh*3+kw);
 *   epilogue = rbvae_gather_gemm's (bias, relu, scale, drop_mode 0 / 1 keyed hash / 2 explicit mask with the same element
 *   indices, gate, per-tile column sums of the stored values into colsum_ws [rbvae_deconv3x3s2_halo_colsum_rows][Nout]).
 * rbvae_deconv3x3s2_halo_ok: 1 when covered (TW % 4 == 0, Kc % 64 (bf16) / 32 (f32) == 0, Nout % 64 == 0, patch fits). */
int rbvae_deconv3x3s2_halo_ok(int dtype, int Nimg, int TH, int TW, int Kc, int Nout);
/* input-grid positions per workgroup the shape runs with: 128 (two 4-wave workgroups per CU), 256 (one 8-wave workgroup:
 * grids whose patch rows do not fit the 80 KB form, e.g. 4 x 4 and 11 x 20), 0 = not covered */
int rbvae_deconv3x3s2_halo_tile_rows(int dtype, int Nimg, int TH, int TW, int Kc, int Nout);
int rbvae_deconv3x3s2_halo_colsum_rows(int dtype, int Nimg, int TH, int TW, int Kc, int Nout);
int rbvae_deconv3x3s2_halo(int dtype, const void* A, const void* W, void* Out, const float* bias, const void* gate,
                           const void* mask, const void* zero_page, int Nimg, int TH, int TW, int Kc, int Nout, int lda,
                           int ldo, int relu, int drop_mode, float drop_p, float scale, unsigned long long seed,
                           const unsigned long long* seed_dev, float* colsum_ws, void* stream);

/* ---- LDM / Stable-Diffusion VAE decoder: latents -> frames (csrc/upconv.hip) --------------------------------
 * The decoder (ldm/modules/diffusionmodules/model.py:462-568 behind AutoencoderKL.decode, ldm/models/autoencoder.py:330-333,
 * and decode_first_stage, ldm/models/diffusion/ddpm.py:706-713) is built from the encoder's blocks and runs on the entry
 * points above; these are the pieces it adds.
 *
 * Upsample (model.py:42-57: F.interpolate(x, scale_factor=2.0, mode="nearest") then Conv2d(c, c, 3, 1, 1)) as four 2x2
 * convolutions of the LOW-resolution input, one per output parity class cls = 2p + q (p, q = output row, column & 1), tap =
 * 2th + tw:
 *   Out[n][2r+p][2c+q][co] = bias[co] + addend + sum_{th,tw,ci} A[n][r-1+p+th][c-1+q+tw][ci] * Wf[co][4 cls + tap][ci]
 *   Wf[co][4 cls + tap][ci] = sum_{kh in R(p,th)} sum_{kw in R(q,tw)} w[co][ci][kh][kw],
 *   R(0,0) = {0}, R(0,1) = {1,2}, R(1,0) = {0,1}, R(1,1) = {2};   A is zero outside the IH x IW map.
 * rbvae_upconv_fold: w f32 [Co][Ci][3][3] (the torch layout) -> Wf [Co][16][Kc] of the storage type: each entry the f32
 * sum over kh ascending and, inside it, kw ascending, starting from +0, rounded once; channels Ci..Kc zero.
 * rbvae_upconv3x3_halo: A [Nimg*IH*IW][lda], Out / addend [Nimg*2IH*2IW][ldo] NHWC rows of the storage type, zero_page >= 128
 * zero bytes (what padding lanes read), every pointer 16-byte aligned; a workgroup
 * owns a 16 x 16 block of low-resolution pixels x 128 output channels x one class, stages the block's 18 x 18 patch in LDS
 * once per 128-byte channel slice and takes the four folded tap tiles through a four-slot LDS-DMA ring.  The same sums
 * come from rbvae_gather_gemm with the four-class descriptor (sa = 1, so = 2, class (p, q): oh0 = p, ow0 = q, taps
 * (4 cls + tap, p - 1 + th, q - 1 + tw)).  rbvae_upconv3x3_halo_ok: 1 when the shape is covered (IH >= 5, IW >= 5,
 * Kc % 64 (bf16) / 32 (f32) == 0, Nout % 128 == 0, fewer than 2^30 output rows); a shape it refuses makes
 * rbvae_upconv3x3_halo return RBVAE_E_UNSUPPORTED without a launch.
 * rbvae_nearest2x_rows: the upsampled rows themselves, out[(n, 2r+p, 2c+q)][0..C) = in[(n, r, c)][0..C) (model.py:52; the
 * as-written baseline in front of a 3x3 convolution), C * sizeof(T) a multiple of 16. */
int rbvae_upconv_fold(int dtype, const float* w, void* out, int Co, int Ci, int Kc, void* stream);
int rbvae_upconv3x3_halo_ok(int dtype, int Nimg, int IH, int IW, int Kc, int Nout);
int rbvae_upconv3x3_halo(int dtype, const void* A, const void* Wf, void* Out, const float* bias, const void* addend,
                         const void* zero_page, int Nimg, int IH, int IW, int Kc, int Nout, int lda, int ldo, void* stream);
int rbvae_nearest2x_rows(int dtype, const void* in, void* out, int Nimg, int IH, int IW, int C, int ldi, int ldo,
                         void* stream);
/* decode_first_stage's z = 1. / scale_factor * z (ddpm.py:713) into the NHWC rows post_quant_conv (autoencoder.py:303,331)
 * reads as a one-tap rbvae_gather_gemm: z f32 [N][Z][HW] -> rows [N*HW][Kpad] of the storage type,
 * z * (float)(1.0 / scale_factor) in f32 (the double quotient rounded to f32 as torch rounds the scalar, then one f32
 * product), then the storage type; columns Z..Kpad zero. */
int rbvae_latent_rows(int dtype, const float* z, void* rows, int N, int Z, int HW, int Kpad, double scale_factor,
                      void* stream);
/* conv_out's rows [N*HW][ld] (3 used columns; model.py:565) -> img f32 [N][3][HW] (the decoder's output, may be NULL) and /
 * or u8 [N][HW][3] (may be NULL): trunc(255 * clamp((x + 1) / 2, 0, 1)) in f32, operation by operation as
 * scripts/pretrained_model_experiments/ldm_embedding_interpol.py:179-182 -- the u8 NHWC frames of csrc/frames.hip. */
int rbvae_decoded_to_image(int dtype, const void* rows, int ld, float* img, unsigned char* u8, int N, int HW, void* stream);

/* ---- raw frames in (csrc/frames.hip) ---------------------------------------------------------------
 * Frames are u8 RGB, NHWC (3 channels, contiguous), a batch of N (<= 65535) images.
 * rbvae_resample_u8: one separable pass of Pillow's 8-bit resampler (Image.resize as called by
 * src/stable-diffusion/get_percep_embeddings.py:59-66, LANCZOS, and by T.Resize in
 * models/contrastive_RBVAE/contrastive_RBVAE_train.py:110-114, BILINEAR; Pillow's Resample.c).  bounds [out][2] =
 * (first source index, taps) and kk [out][ksize] int32 coefficients with 22 fractional bits come from the host
 * (frames.py resample_coeffs); acc = (1 << 21) + sum_t src[first + t] * kk[o][t] in int32, result clamp(acc >> 22, 0, 255).
 *   vertical = 0: in [N][in_h][in_w][3] -> out [N][out_h][out_w][3], output row r = source row row0 + r resampled
 *                 along the width (row0 + out_h <= in_h: Pillow's horizontal pass covers only the rows the vertical pass
 *                 reads, ybox_first .. ybox_last);
 *   vertical = 1: in [N][in_h][W][3] -> out [N][out_h][W][3] (in_w == out_w == W), output row yy reads source rows
 *                 bounds[yy][0] - row0 + t (Pillow's shift of the vertical bounds by ybox_first).
 * Taps outside the source are skipped (a row whose taps all are gives 0), and at most ksize taps are read per row.
 * RBVAE_E_UNSUPPORTED when a horizontal pass's two rows exceed 64 KB of LDS: ((3 in_w + 7) & ~3) + ((3 out_w + 7) & ~3)
 * > 65536, e.g. 10921 -> 10921 pixels runs and 10921 -> 10922 does not. */
int rbvae_resample_u8(const unsigned char* in, unsigned char* out, int N, int in_h, int in_w, int out_h, int out_w,
                      int vertical, int row0, const int* bounds, const int* kk, int ksize, void* stream);
/* ToTensor -> add_gaussian_noise (kind 1) / add_occlusion (kind 2) -> ToPILImage
 * (scripts/evaluation/state_consistency_eval/embedding_matching.py:141-193 as called at :241-248), u8 in, u8 out, f32
 * operations in the reference's order: x = u8 / 255; kind 1: x = clamp(x + (noise * std + mean), 0, 1) with noise f32
 * [N][3][H][W] (randn_like of each frame's [1,3,H,W] tensor); kind 2: x = 0.5 inside the square boxes[n] = (x, y, size),
 * int32 [N][3]; then trunc(x * 255) (.mul(255).byte()). */
int rbvae_perturb_u8(const unsigned char* in, unsigned char* out, int N, int H, int W, int kind, const float* noise,
                     float std_, float mean_, const int* boxes, void* stream);
/* u8 [N][H][W][3] -> f32 [N][3][H][W]: mode 0 = T.ToTensor (x / 255, contrastive_RBVAE_train.py:110-114); mode 1 =
 * load_img's np.float32(x) / 255 then 2x - 1 (get_percep_embeddings.py:68-71, embedding_matching.py:335-338). */
int rbvae_u8_to_input(const unsigned char* in, float* out, int N, int H, int W, int mode, void* stream);

/* ---- linear probe evaluation (csrc/probe.hip) -----------------------------------------------------------
 * scripts/evaluation/linear_projection_eval/linear_regression_eval.py:123-144: LinearRegression().fit on the train rows,
 * predict on the test rows, r2_score / explained_variance_score (uniform average), mean_squared_error and
 * mean_absolute_error, for an embedding of L <= 128 values and P targets per row, all in f64.
 * Targets Y are resident on the device as u8 (RBVAE_PROBE_U8: [N][P] bytes, e.g. frames [N][H][W][3]; a value is
 * ToTensor's (float)v / 255.0f widened to f64) or f32 (RBVAE_PROBE_F32: [N][P]).  Rows are addressed through int32 lists
 * on the device, in any order; an index outside [0, N) contributes nothing.  row0 (in [0, N)) is the row every target is
 * shifted by, which makes a target that is constant over the rows come out exactly.
 *
 * rbvae_probe_xty (:126, fit): C [M][P] = B^T (Y[rows] - Y[row0]) on the f64 matrix cores, B [n_rows][M] f64 the host's
 * fit factor (2 <= M <= 129; for the fit M = L + 1: the minimum-norm least-squares operator's transpose and a column
 * 1 / n_rows, so rows 0..L-1 of C are the coefficients and row L the shifted target mean).  Long row lists are split
 * over rbvae_probe_xty_slabs K slabs, written to ws (rbvae_probe_xty_ws_bytes bytes, may be NULL when that is 0) and
 * summed in slab order: two runs agree bit for bit. */
#define RBVAE_PROBE_U8 0
#define RBVAE_PROBE_F32 1
int rbvae_probe_xty_slabs(int n_rows, int M, long P);
size_t rbvae_probe_xty_ws_bytes(int n_rows, int M, long P);
int rbvae_probe_xty(int y_dtype, const void* Y, long N, long P, const int* rows, int n_rows, int row0,
                    const double* B, int M, double* C, double* ws, void* stream);
/* linear_regression_eval.py:126 (model.intercept_): intercept [P] = (C[L] - sum_l mean_x[l] C[l]) + Y[row0], l ascending;
 * C [L + 1][P] from rbvae_probe_xty, mean_x [L] the train mean of the embedding. */
int rbvae_probe_intercept(int y_dtype, const void* Y, long N, long P, int row0, const double* C, const double* mean_x,
                          int L, double* intercept, void* stream);
/* linear_regression_eval.py:129-144 (predict and the sums behind the four metrics) over the rows of the list: with
 * e = y - (intercept + sum_l Xr[r][l] C[l]) and d = y - Y[row0], sums [5][P] = sum e, sum e^2, sum |e|, sum d, sum d^2.
 * Xr [n_rows][L] f64 holds the embedding of row rows[r] in row r. */
int rbvae_probe_residual_sums(int y_dtype, const void* Y, long N, long P, const int* rows, int n_rows, int row0,
                              const double* Xr, const double* C, const double* intercept, int L, double* sums,
                              void* stream);
/* linear_regression_eval.py:135-144: per target r2 [P] = 1 - sum e^2 / SStot, SStot = sum d^2 - (sum d)^2 / m, and
 * evs [P] = 1 - (sum e^2 / m - (sum e / m)^2) / (SStot / m), a zero denominator scoring 1 with a zero numerator and 0
 * otherwise (scikit-learn's force_finite); metrics [4] = (mean r2, mse, mae, mean evs), n_constant [1] = targets with
 * SStot == 0.  m = the number of test rows behind sums; part: workspace of rbvae_probe_finish_parts(P) * 5 doubles.
 * The reductions run in a fixed order (no atomics). */
int rbvae_probe_finish_parts(long P);
int rbvae_probe_finish(const double* sums, long P, int m, double* r2, double* evs, double* part, double* metrics,
                       int* n_constant, void* stream);

/* ---- latent-space projections (csrc/project.hip) --------------------------------------------------------
 * scripts/evaluation/clustering_eval/embedding_umap.py: the soft latents of the test frames (:214, :224) projected to 2-D
 * by PCA (:111-112), t-SNE (:87-88) and UMAP (:63-64).  PCA and t-SNE run here as scikit-learn 1.7.2 computes them
 * (DESIGN.md section 7 names the two deliberate differences); UMAP's fuzzy graph and layout follow below (csrc/umap.hip).
 * Every reduction has a fixed order (no atomics): two runs agree bit for bit.
 *
 * rbvae_knn (:63 n_neighbors = 24, :87 perplexity = 30 -> k = 91): the exact k nearest neighbours of every row of
 * X f32 [N][L], 2 <= N <= 16384 (all N distances of a row sit in LDS as f64), 1 <= L <= 128, 1 <= k <= min(N - 1, 128).
 * d2 [N][k] = sum_l (x_il - x_jl)^2 in f64, l ascending, each difference exact and each square rounded once; idx [N][k];
 * row i is never its own neighbour; a row's neighbours are sorted by (d2, j) ascending, ties to the lower index.
 * X must be finite: the entry point does not look (projection.knn_graph does); where NaN or infinite rows leave a query
 * fewer than k finite distances, the rest of its row is d2 = inf with idx = 0x7fffffff, and nothing is written elsewhere.
 * rbvae_knn_ok: 1 when (N, L, k) is covered; anything else makes rbvae_knn return RBVAE_E_INVALID without a launch. */
int rbvae_knn_ok(int N, int L, int k);
int rbvae_knn(const float* X, int N, int L, int k, int* idx, double* d2, void* stream);
/* :87-88 (TSNE.fit_transform -> _joint_probabilities_nn -> sklearn.manifold._utils._binary_search_perplexity): per row,
 * over the k <= 128 distances d2 [N][k] rounded to f32, the f64 bisection on beta (start 1, doubling / halving until
 * bracketed, at most 100 entropy evaluations, tolerance (double)1e-5f, a zero sum replaced by (double)1e-8f) towards
 * entropy log((double)perplexity), 0 < perplexity < k.  P [N][k] the conditional probabilities, beta [N] the value P
 * was evaluated at, steps [N] the number of entropy evaluations.  One wave per row; the two sums of an evaluation are
 * butterfly sums over the wave. */
int rbvae_tsne_perplexity(const double* d2, int N, int k, float perplexity, double* P, double* beta, int* steps,
                          void* stream);
/* :88, one gradient iteration of TSNE._tsne (sklearn.manifold._t_sne._gradient_descent over _kl_divergence_bh, with the
 * exact repulsion that angle = 0 gives) as three launches.  Y f32 [N][2], 8-byte aligned.
 * rbvae_tsne_repulse: part [splits][N][3] f32 = (R_x, R_y, Z_i) over the j slice s, R_i = sum_{j != i} q^2 (y_i - y_j),
 * Z_i = sum_{j != i} q, q = 1 / (1 + |y_i - y_j|^2) in f32 (hardware reciprocal), splits = rbvae_tsne_repulse_splits(N).
 * rbvae_tsne_zsum: Z [1] f64 = the sum of every part[s][i][2] (one workgroup: thread t of 1024 adds the elements t,
 * t + 1024, ... of the [splits][N] array in ascending order, then a halving tree).
 * rbvae_tsne_step: the joint P as CSR (indptr int32 [N + 1], indices int32, data f32), sched = device floats
 * (exaggeration, momentum, learning rate), N >= 2.  Per row, p = exaggeration * data in f32:
 *   A = sum_e p q (y_i - y_j),  R = sum_s part[s][i] (s ascending),  g = 4 (float)((double)A - (double)R / Z)
 *   gains = update * g < 0 ? gains + 0.2 : gains * 0.8, at least 0.01;  update = momentum * update - lr * (gains * g)
 *   Y_out = Y + update (Y_out != Y: rows read their neighbours' old positions)
 * and stats [rbvae_tsne_step_parts(N)][3] f64 = the workgroup's sums of |g|^2, |gains g|^2 (the vector whose norm
 * _gradient_descent compares with min_grad_norm) and p log(max(p, FLT_MIN) / max(q / Z, FLT_MIN)) (the error of
 * _barnes_hut_tsne's compute_gradient_positive). */
int rbvae_tsne_repulse_splits(int N);
int rbvae_tsne_repulse(const float* Y, int N, float* part, void* stream);
int rbvae_tsne_zsum(const float* part, int N, double* Z, void* stream);
int rbvae_tsne_step_parts(int N);
int rbvae_tsne_step(const float* Y, float* Y_out, float* update, float* gains, const int* indptr, const int* indices,
                    const float* data, const float* part, const double* Z, const float* sched, int N, double* stats,
                    void* stream);
/* :111-112 (PCA(n_components=2).fit_transform; the covariance_eigh solver): mean f64 [L] = (sum_rows x) / N and
 * cov f64 [L][L] = sum_rows (x_a - mean_a)(x_b - mean_b) / (N - 1), symmetric by construction, N >= 2, L <= 128; the host
 * takes the eigenvectors.  rbvae_pca_project: out f64 [N][n_components] = (X - mean) V^T, V f64 [n_components][L],
 * n_components <= min(L, 8), l ascending. */
int rbvae_pca_moments(const float* X, int N, int L, double* mean, double* cov, void* stream);
int rbvae_pca_project(const float* X, int N, int L, const double* mean, const double* V, int n_components, double* out,
                      void* stream);

/* ---- UMAP (csrc/umap.hip) ---------------------------------------------------------------------------------
 * embedding_umap.py:63-64, umap.UMAP(n_neighbors=24, min_dist=0.25, metric='euclidean', random_state=42), after McInnes,
 * Healy, Melville 2018 (Algorithms 2-5) and umap-learn's published defaults; DESIGN.md section 7 has the formulation and
 * the two deliberate differences (the initial map, the synchronous epoch).  n_neighbors = k counts the point itself: the
 * graph is rbvae_knn with K1 = k - 1 <= 127 columns, d = (double)(float)sqrt(d2).  Every sum has one fixed order.
 *
 * rbvae_umap_smooth_knn, all arithmetic f64: dsum [1] = the sum of every d (one workgroup: thread t of 1024 adds the
 * elements t, t + 1024, ... in ascending order, then a halving tree).  Per row (one wave, two neighbours per lane):
 * rho = the smallest d > 0, or 0; the bisection on sigma from lo = 0, hi = inf, mid = 1, at most 64 evaluations of
 *   psum = sum_r (d_r - rho > 0 ? exp(-(d_r - rho) / mid) : 1)           (a butterfly sum over the wave)
 * stopping at |psum - log2 k| < 1e-5; psum > log2 k: hi = mid, mid = (lo + hi) / 2; otherwise lo = mid and mid doubles
 * while hi = inf, else (lo + hi) / 2.  steps [N] = the evaluations.  sigma = max(mid, 1e-3 m), m = (sum_r d_r) / k where
 * rho > 0 and dsum / (N k) where rho = 0.  w [N][K1] = 1 where d_r - rho <= 0 or sigma = 0, else exp(-(d_r - rho) / sigma).
 * rho [N], sigma [N] and w are stored as f32.  rbvae_umap_smooth_knn_ok: 1 when N >= 1 and 1 <= K1 <= 127; anything else
 * makes the call return RBVAE_E_INVALID without a launch.
 *
 * rbvae_umap_epoch: epoch n of n_epochs on the symmetric fuzzy graph as CSR (indptr int32 [N + 1], indices int32 [E]) with
 * the schedule period f32 [E] = max(W) / W_e and the state next, next_neg f32 [E] (initially period and period /
 * neg_rate), updated in place.  Y, Y_out f32 [N][2], 8-byte aligned, Y_out != Y: every vertex moves from the epoch-start
 * map.  2 <= N <= 16384.  alpha = 1 - (float)n / (float)n_epochs.  One wave per vertex i, its row's edges in chunks of 64,
 * one per lane; an edge e = (i -> j) with next_e <= n adds, in f32,
 *   2 clip(c D, +-4),  D = y_i - y_j,  r2 = |D|^2,  c = r2 > 0 ? fl(-2ab) pow(r2, b - 1) / (a pow(r2, b) + 1) : 0
 * (twice: the mirror edge j -> i shares weight and schedule, and its move of the other end is this same vector), then for
 * q = clamp((int)((n - next_neg_e) / neg_period_e), 0, 32), neg_period_e = period_e / neg_rate, and p = 0 .. q - 1
 *   m = ((uint64)hash_u32(seed, (uint64)n << 40 | (uint64)e << 8 | p) * N) >> 32,  skipped when m = i,
 *   clip(c D, +-4),  D = y_i - y_m,  c = r2 > 0 ? fl(2 gamma b) / ((0.001 + r2)(a pow(r2, b) + 1)) : 0
 * and next_e += period_e, next_neg_e += q neg_period_e.  A butterfly adds a chunk, the chunks are added in order,
 * Y_out_i = y_i + alpha sum.  An edge whose index is outside [0, N) is left alone.  hash_u32 is csrc/common.h's.
 * rbvae_umap_epoch_samples: the same schedule arithmetic and draws for the epoch the state stands before, written out and
 * not applied: count int32 [E] = q (0 for an edge that is not active), samples int32 [E][32] = m, -1 in a slot that is not
 * drawn or drew i itself.
 * rbvae_umap_epoch_ok: 1 when (N, n_epochs <= 2^20, 1 <= neg_rate <= 64) is covered; refused arguments (also epoch outside
 * 0 .. n_epochs - 1, a or b <= 0, gamma < 0, Y_out = Y) return RBVAE_E_INVALID without a launch. */
int rbvae_umap_smooth_knn_ok(int N, int K1);
int rbvae_umap_smooth_knn(const double* d2, int N, int K1, double* dsum, float* rho, float* sigma, float* w, int* steps,
                          void* stream);
int rbvae_umap_epoch_ok(int N, int n_epochs, int neg_rate);
int rbvae_umap_epoch(const float* Y, float* Y_out, const int* indptr, const int* indices, const float* period, float* next,
                     float* next_neg, int N, int epoch, int n_epochs, float a, float b, float gamma, int neg_rate,
                     unsigned long long seed, void* stream);
int rbvae_umap_epoch_samples(const int* indptr, const float* period, const float* next, const float* next_neg, int N,
                             int epoch, int n_epochs, int neg_rate, unsigned long long seed, int* count, int* samples,
                             void* stream);

/* ---- latent scores (csrc/scores.hip) ---------------------------------------------------------------------
 * What embedding_umap.py leaves to the eye, as numbers: how faithful a 2-D map is (trustworthiness, continuity) and how
 * well the labelled latents separate (silhouette), as scikit-learn 1.7.2 computes them; scores.py finishes both on the
 * host.  Counts are integers and every f64 sum has one fixed order (no atomics): two runs agree bit for bit.
 * d2(i, j) = sum_l (x_il - x_jl)^2 is rbvae_knn's, from the same device function: f64, l ascending, each difference exact,
 * each square rounded once.
 *
 * rbvae_nbr_ranks (sklearn.manifold.trustworthiness): X f32 [N][L] and nbr int32 [N][k], row i's neighbours in some other
 * space (rbvae_knn of the map); limits as rbvae_knn: 2 <= N <= 16384 (a row's N distances sit in LDS as f64),
 * 1 <= L <= 128, 1 <= k <= min(N - 1, 128).  rank [N][k]: the 1-based position of j = nbr[i][r] among the N - 1 other rows
 * of X ordered by (d2(i, .), index) ascending, rank = 1 + #{m != i : d2(i,m) < d2(i,j) or (d2(i,m) == d2(i,j) and m < j)};
 * excess [N] = sum_r max(0, rank[i][r] - k).  An entry of nbr outside [0, N) (rbvae_knn's 0x7fffffff) or equal to i gets
 * rank -1, adds nothing to excess and reads nothing outside X.  X must be finite.
 * rbvae_nbr_ranks_ok: 1 when (N, L, k) is covered; anything else makes rbvae_nbr_ranks return RBVAE_E_INVALID without a
 * launch. */
int rbvae_nbr_ranks_ok(int N, int L, int k);
int rbvae_nbr_ranks(const float* X, int N, int L, const int* nbr, int k, int* rank, int* excess, void* stream);
/* sklearn.metrics.silhouette_samples' reduction: the rows grouped by state, order int32 [N] (a stable sort by label: rows
 * ascend within a state) and seg int32 [S + 1] (the states' offsets into order; an empty state has an empty segment);
 * 1 <= N <= 16384, 1 <= L <= 128, 1 <= S <= 256.  sums [N][S], indexed by the original row i:
 *   rbvae_label_dist_sums     f64: sum over the rows j of segment s, in segment order, of sqrt(d2(i, j)) (an IEEE square
 *                             root; the j = i term is an exact 0)
 *   rbvae_label_hamming_sums  int32: sum_j popcount(key_i xor key_j), the 128-bit keys packed as rbvae_state_vote packs
 *                             them (bit = value > 0.5)
 * Entries of order outside [0, N) are skipped and seg is clamped to [0, N]: nothing is read outside X or order.
 * rbvae_label_sums_ok: 1 when (N, L, S) is covered; anything else returns RBVAE_E_INVALID without a launch. */
int rbvae_label_sums_ok(int N, int L, int S);
int rbvae_label_dist_sums(const float* X, int N, int L, const int* order, const int* seg, int S, double* sums,
                          void* stream);
int rbvae_label_hamming_sums(const float* codes, int N, int L, const int* order, const int* seg, int S, int* sums,
                             void* stream);

/* ---- unsupervised symbols (csrc/kmeans.hip) ------------------------------------------------------------------
 * Do the latents fall into the states by themselves?  Lloyd's k-means with k-means++ seeding as scikit-learn 1.7.2's
 * KMeans(n_init=1, algorithm="lloyd") runs it, and the per-cluster sums behind the Davies-Bouldin and Calinski-Harabasz
 * indices; symbols.py keeps the RandomState draws and finishes the scores on the host.  X f32 [N][L], centres f64 [K][L];
 * 1 <= L <= 128, 1 <= K <= 256, K <= N <= 1048576 (rbvae_kmeans_ok); anything else makes every entry return
 * RBVAE_E_UNSUPPORTED without a launch.  All arithmetic is f64, never contracted; d2_ik = sum_l (x_il - c_kl)^2 with l
 * ascending (the difference now rounds: c is any f64 value).  No floating-point atomics: every sum has one fixed order.
 *
 * state int32 [4] = {done, n_iter, why (1 strict, 2 tol, 3 max_iter), changed}, zero before the first iteration; may be
 * NULL in rbvae_kmeans_assign and rbvae_kmeans_update.  With done set, assign, update and decide return without writing
 * anything, so iterations may be enqueued ahead of the decision.
 * rbvae_kmeans_assign: label int32 [N] = the k with the smallest (d2, k) (ties to the lower centre), d2 f64 [N] = that
 * distance; the number of rows with label != label_prev (NULL: every row) is added to state[3].  The centres pass through
 * LDS rbvae_kmeans_chunk_centres(L) = 4096 / round_up(L, 8) at a time.  With own int32 [N] given, label = own and d2 =
 * the distance to the row's own centre (label -1, d2 inf where own is no centre).
 * rbvae_kmeans_update: centres_k = (sum of the rows labelled k) / count_k in place, shift2 [K] = |new - old|^2,
 * within [K] = sum of d2 and spread [K] = sum of sqrt(d2) over the cluster's rows (0 with d2 = NULL), count int32 [K].
 * Stage one: min(256, ceil(N / 256)) blocks of consecutive rows, each cell of a block's partial added in ascending row
 * order; stage two adds the partials in block order.  An empty cluster keeps its centre: shift2 = 0, count = 0 (scikit-learn
 * moves it to the row farthest from its centre).  A label outside [0, K) is skipped.  ws: rbvae_kmeans_ws_bytes(N, L, K).
 * rbvae_kmeans_decide: n_iter += 1; changed == 0: done, strict; else sum_k shift2 (k ascending) <= tol_abs: done, tol; else
 * n_iter >= max_iter: done; changed = 0.
 * rbvae_kmeans_pp_trials: cand int32 [T], T <= 8 -> out f64 [T][N] = min(closest_i, d2(x_i, x_cand_t)) and pot f64 [T] =
 * its sum (a halving tree per 256 rows, then over the workgroups' sums); a candidate outside [0, N) leaves closest. */
int rbvae_kmeans_ok(int N, int L, int K);
int rbvae_kmeans_chunk_centres(int L);
size_t rbvae_kmeans_ws_bytes(int N, int L, int K);
int rbvae_kmeans_assign(const float* X, int N, int L, const double* centres, int K, const int* label_prev, const int* own,
                        int* label, double* d2, int* state, void* stream);
int rbvae_kmeans_update(const float* X, int N, int L, const int* label, const double* d2, int K, double* centres, int* count,
                        double* shift2, double* within, double* spread, double* ws, const int* state, void* stream);
int rbvae_kmeans_decide(const double* shift2, int K, double tol_abs, int max_iter, int* state, void* stream);
int rbvae_kmeans_pp_trials(const float* X, int N, int L, const int* cand, int T, const double* closest, double* out,
                           double* pot, double* ws, void* stream);

/* ---- Gaussian mixture (csrc/gmm.hip) -------------------------------------------------------------------------
 * How many states are there, and how sure is each frame's?  A diagonal-covariance Gaussian mixture of X f32 [N][L] fitted
 * by EM as scikit-learn 1.7.2's GaussianMixture(covariance_type="diag", n_init=1) fits it; mixture.py enqueues the
 * iterations and finishes BIC and AIC on the host.  means, covars, prec_chol f64 [K][L] (prec_chol: s_kl = 1 / sqrt(var_kl),
 * scikit-learn's precisions_cholesky_), weights, logc f64 [K], resp f64 [K][N] (component-major).  1 <= L <= 128,
 * 1 <= K <= 256, K <= N <= 1048576 and N K <= 2^26, since resp is materialised (rbvae_gmm_ok); anything else makes every
 * entry return RBVAE_E_UNSUPPORTED without a launch.  All arithmetic is f64, never contracted; exp, log and sqrt are the
 * device library's.  No floating-point atomics: every sum has one fixed order and two runs agree bit for bit.
 *
 * state int32 [4] = {done, n_iter, why (1 converged, 2 max_iter), 0}, zero before the first iteration; may be NULL in
 * rbvae_gmm_estep and rbvae_gmm_mstep.  With done set, estep, mstep and decide return without writing anything, so
 * iterations may be enqueued ahead of the decision.  Only rbvae_gmm_decide writes state.
 * rbvae_gmm_estep: lp_ik = logc_k - (1 / 2) q_ik, q_ik = sum_l t^2 with t = (x_il - mu_kl) s_kl and l ascending from zero
 * (the difference, the product and the square round once each), logc_k = log w_k + sum_l log s_kl - (1 / 2) L log 2 pi as
 * rbvae_gmm_mstep writes it; m_i = max_k lp_ik; lognorm_i = m_i + log(sum_k exp(lp_ik - m_i)) with k ascending from zero;
 * resp_ki = exp(lp_ik - lognorm_i); label_i = the k of the largest lp_ik (a tie goes to the lower k).  lognorm f64 [N];
 * resp and label int32 [N] may be NULL (scoring, prediction).  The means and roots pass through LDS
 * rbvae_gmm_chunk_components(L) = 2048 / round_up(L, 8) components at a time.  resp is first used to hold lp.
 * rbvae_gmm_mstep: two-pass and centred, each pass in two stages.  min(256, ceil(N / 256)) blocks of ceil(N / blocks)
 * consecutive rows; each cell's partial is added in ascending row order from zero, the partials then in block order from
 * zero.  nk_k = sum_i resp_ki + 10 * 2^-52; mu_kl = (sum_i resp_ki x_il) / nk_k; var_kl = (sum_i resp_ki d^2) / nk_k +
 * reg_covar with d = x_il - mu_kl (d, d^2 and the product round once each); weights_k = nk_k / sum_k nk_k (k ascending from
 * zero); s_kl = 1 / sqrt(var_kl); logc_k = (log weights_k + sum_l log s_kl) - (1 / 2) L log 2 pi (l ascending from zero,
 * log 2 pi = 1.8378770664093453).  A component without mass follows the same formulas: nk = 10 * 2^-52, mean 0, variance
 * reg_covar.  ws: rbvae_gmm_ws_bytes(N, L, K) = 16 blocks K (L + 1) bytes, the two passes' block partials f64
 * [2][blocks][K][L + 1]: cell (k, l) of the first holds the block's sum of resp_ki x_il and cell (k, L) that of resp_ki, cell
 * (k, l) of the second that of resp_ki d^2 and cell (k, L) zero.
 * rbvae_gmm_decide: now = (sum_i lognorm_i) / N in rbvae_spectral_dots' order (blocks of 1024 rows: thread t of 256 adds its
 * rows 1024 b + t + 256 s, s = 0..3, from zero, a butterfly adds each wave's 64 threads, the four waves' sums are added in
 * wave order from zero, the blocks' sums in block order from zero); n_iter += 1; history[n_iter - 1] = now (history f64
 * [max_iter]); |now - lb[0]| < tol: done, converged; else n_iter >= max_iter: done; lb[0] = now.  lb f64 [1] holds -inf before
 * the first iteration. */
int rbvae_gmm_ok(int N, int L, int K);
int rbvae_gmm_chunk_components(int L);
size_t rbvae_gmm_ws_bytes(int N, int L, int K);
int rbvae_gmm_estep(const float* X, int N, int L, const double* means, const double* prec_chol, const double* logc, int K,
                    double* resp, double* lognorm, int* label, const int* state, void* stream);
int rbvae_gmm_mstep(const float* X, int N, int L, const double* resp, int K, double reg_covar, double* weights,
                    double* means, double* covars, double* prec_chol, double* logc, double* ws, const int* state,
                    void* stream);
int rbvae_gmm_decide(const double* lognorm, int N, double tol, int max_iter, double* lb, double* history, int* state,
                     void* stream);

/* ---- state boundaries (csrc/segment.hip) ---------------------------------------------------------------------
 * Where do the states change?  The optimal partition of the N rows of X f32 [N][L] (in time order) into K contiguous
 * segments with the least within-segment sum of squared deviations, by the exact dynamic programme over (segments, end
 * row); segments.py traces and scores it.  2 <= N <= 65536, 1 <= L <= 128, 1 <= K <= 256, min_size >= 1,
 * K min_size <= N (rbvae_segment_ok); anything else makes every entry return RBVAE_E_UNSUPPORTED without a launch.  All
 * arithmetic is f64, never contracted, l ascending.  No floating-point atomics: two runs agree bit for bit.
 *
 * rbvae_segment_prefix: P f64 [N + 1][L] and Q f64 [N + 1], the running sums of the rows and of r_i = sum_l x_il^2, with
 * P[0] = 0 and Q[0] = 0.  Rows are taken in blocks of 256: inside block b the local running sums start from the block's
 * first row and add one row at a time, P[256 b + i + 1] = off_b + local_i, off_{b + 1} = off_b + local_last, off_0 = 0
 * (numpy: off + np.cumsum(block, axis=0)).  X is not centred: on 0/1 codes every sum is an exact integer.
 * rbvae_segment_layer: cost(s, t) = (Q[t] - Q[s]) - d2(P[t], P[s]) / (double)(t - s), d2 = sum_l (a_l - b_l)^2 (not clamped
 * where rounding leaves it slightly negative).  For every end 0 <= t <= N the candidates are prev[s] + cost(s, t) over
 * 0 <= s <= t - min_size with prev[s] finite (prev f64 [N + 1]); out f64 [N + 1] is the smallest in the order (value, s)
 * ascending, arg int32 [N + 1] its s (a tie goes to the lower s), and (+inf, -1) where there is no candidate.  The minimum
 * is exact: the result does not depend on how the starts are split over workgroups.  ws: rbvae_segment_ws_bytes(N, L).
 * The table of K layers is D_1 = layer(prev = [0, +inf, ...]), D_k = layer(D_{k - 1}); D_k[N] is the cost of the best
 * k-segmentation.
 * rbvae_segment_trace: cost f64 [K][N + 1] and arg int32 [K][N + 1] are the table; cuts int32 [K][K]: row k - 1 holds the
 * k - 1 interior boundaries of the best k-segmentation (each the position of the first row of a new segment) ascending,
 * padded with -1; all -1 where D_k[N] is not finite.  A thread per k walks t <- arg[j][t] from t = N, j = k down to 2. */
int rbvae_segment_ok(int N, int L, int K, int min_size);
size_t rbvae_segment_ws_bytes(int N, int L);
int rbvae_segment_prefix(const float* X, int N, int L, double* P, double* Q, void* stream);
int rbvae_segment_layer(const double* P, const double* Q, int N, int L, const double* prev, int min_size, double* out,
                        int* arg, void* ws, void* stream);
int rbvae_segment_trace(const int* arg, int N, int K, const double* cost, int* cuts, void* stream);

/* ---- spectral layout (csrc/spectral.hip) ---------------------------------------------------------------------
 * The lowest eigenvectors of L = I - S, S = D^-1/2 W D^-1/2, of a symmetric graph W in CSR (indptr int32 [N + 1], indices
 * int32 [E], data f32 [E]; the fuzzy graph of rbvae_umap_smooth_knn's memberships), by Lanczos with full
 * reorthogonalisation against a basis on the device; spectral.py enqueues the steps, solves the tridiagonal problem on the
 * host and applies umap-learn's and scikit-learn's conventions.  2 <= N <= 1048576, E <= 2^31 - 1, 1 <= m_max <= 1024,
 * 0 <= q <= 8 (rbvae_spectral_ok); anything else makes every entry return RBVAE_E_UNSUPPORTED without a launch, a NULL
 * pointer or a workspace below rbvae_spectral_ws_bytes(N, m_max, q) RBVAE_E_INVALID.  All arithmetic is f64, never
 * contracted.  No floating-point atomics: every sum has one fixed order and two runs agree bit for bit.
 *
 * rbvae_spectral_degree: deg_i = sum_e (double)data[e] over row i, e ascending from zero; isd_i = 1 / sqrt(deg_i), 0 where
 * deg_i = 0.  An entry whose column is outside [0, N) is skipped, here and in the product.
 * rbvae_spectral_matvec: y_i = isd_i * sum_e t_e, t_e = (double)data[e] * (isd_j * x_j), j = indices[e].  A wave per row:
 * lane l of chunk n holds the row's edge 64 n + l (0 beyond the row), the chunk is added by a butterfly (lane l adds lane
 * l ^ 32, then ^ 16, ... ^ 1), the chunk sums are added in order from zero.  y must not be x.
 * rbvae_spectral_dots: c_k = V_k . w for the nv <= 1025 vectors V f64 [nv][N], in two stages.  Rows are taken in blocks of
 * rbvae_spectral_block_rows() = 1024: in block b thread t (of 256) adds the products of its rows 1024 b + t + 256 s,
 * s = 0..3, from zero (rows beyond N count 0), a butterfly adds each wave's 64 threads, the four waves' sums are added in
 * wave order; c_k adds the blocks' partials in block order from zero.  ws: rbvae_spectral_ws_bytes(N, max(nv - 1, 1), 0).
 * rbvae_spectral_update: w_i = w_i - s_i, s_i = sum_k c_k V_k[i] with k ascending from zero.
 * rbvae_spectral_step: Lanczos step j on the basis V f64 [q + m_max + 1][N], whose first q rows are locked orthonormal
 * vectors and whose row q + j is v_j (row q: the caller's unit start vector, orthogonal to the locked ones).  In order:
 * w = S v_j into row q + j + 1 (the product above); twice: c = V_{0 .. q + j}^T w (the dots above), w -= V^T c (the update
 * above); alpha[j] = the two passes' c_{q + j} added; beta[j] = sqrt(w . w) (the dots' sum); v_{j + 1} = w / beta[j].
 * state int32 [2] = {broken, steps}, zero before step 0: steps = j + 1 once alpha[j] and beta[j] are written; beta[j] <=
 * 2^-40 (or not a number) sets broken: the Krylov space is invariant, row q + j + 1 keeps the unnormalised remainder and is
 * no basis vector, and every later step returns without writing anything, so steps may be enqueued ahead of the read.
 * rbvae_spectral_ritz: Y f64 [cols][N], Y_c[i] = sum_j V[q + j][i] s[j][c] with j ascending from zero, for s f64 [m][cols]
 * on the device, 1 <= cols <= 32, 1 <= m <= 1024.
 * rbvae_spectral_residuals: res[c] = |S y_c - theta[c] y_c|_2 for Y f64 [cols][N], theta f64 [cols] on the device: the
 * product above, r_i = (S y)_i - theta y_i, and sqrt(r . r) by the dots' sum.  ws: rbvae_spectral_ws_bytes(N, 1, 0). */
int rbvae_spectral_ok(int N, int m_max, int q);
int rbvae_spectral_block_rows(void);
size_t rbvae_spectral_ws_bytes(int N, int m_max, int q);
int rbvae_spectral_degree(const int* indptr, const int* indices, const float* data, int N, double* deg, double* isd,
                          void* stream);
int rbvae_spectral_matvec(const int* indptr, const int* indices, const float* data, const double* isd, int N,
                          const double* x, double* y, void* stream);
int rbvae_spectral_dots(const double* V, int nv, int N, const double* w, double* c, void* ws, size_t ws_bytes,
                        void* stream);
int rbvae_spectral_update(const double* V, int nv, int N, const double* c, double* w, void* stream);
int rbvae_spectral_step(const int* indptr, const int* indices, const float* data, const double* isd, int N, double* V,
                        int q, int j, int m_max, double* alpha, double* beta, int* state, void* ws, size_t ws_bytes,
                        void* stream);
int rbvae_spectral_ritz(const double* V, int q, int m, int N, const double* s, int cols, double* Y, void* stream);
int rbvae_spectral_residuals(const int* indptr, const int* indices, const float* data, const double* isd, int N,
                             const double* Y, int cols, const double* theta, double* res, void* ws, size_t ws_bytes,
                             void* stream);

/* ---- hidden Markov model (csrc/hmm.hip) ----------------------------------------------------------------------
 * Which state is each frame in, given its neighbours in time?  One sequence X f32 [N][L] in time order, K states with the
 * mixture's diagonal Gaussian emissions (means, prec_chol f64 [K][L]), pi f64 [K] and a row-stochastic A f64 [K][K] (zeros
 * allowed); hmm.py drives Baum-Welch with rbvae_gmm_mstep and rbvae_gmm_decide.  1 <= L <= 128, 1 <= K <= 64,
 * max(K, 2) <= N <= 1048576 and N K <= 2^26 (rbvae_hmm_ok; inside rbvae_gmm_ok): anything else makes every entry return
 * RBVAE_E_UNSUPPORTED without a launch; a NULL pointer, block_rows < 1 or a workspace below
 * rbvae_hmm_ws_bytes(N, K, block_rows) RBVAE_E_INVALID.  All arithmetic is f64, never contracted; exp and log are the device
 * library's.  No floating-point atomics: every sum has one fixed order and two runs agree bit for bit.
 *
 * state is the mixture's int32 [4] = {done, n_iter, why, 0} and may be NULL; with done set every entry returns without
 * writing anything.  status int32 [2] = {the number of normalisers that are 0 or not finite, the first row with one}: the
 * caller sets it to {0, 2^31 - 1} and the entries add to the count and lower the row (integer atomics); nothing else is
 * done about such a row, whose quotients are what IEEE division gives.
 * rbvae_hmm_emit: lb_kt = c_k - q_kt / 2 with q_kt as rbvae_gmm_estep's and c_k = (sum_l log s_kl) - (1 / 2) L log 2 pi, l
 * ascending from zero (no mixture weight).  logb f64 [K][N] = lb; rowmax f64 [N]: m_t = max_k lb_kt; e f64 [N][K]:
 * e_tk = exp(lb_kt - m_t).
 * The recurrence.  SUM(y) over the states is a butterfly over 64 lanes, lane j holding y_j and the lanes from K on zero:
 * lane l adds lane l ^ 32, then ^ 16, ... ^ 1 (a halving tree: 0..31 + 32..63, then 0..15 + 16..31, ...).  DOT_j(x, M) =
 * sum_i x_i M_ij with i ascending from zero, every product rounded before it is added.
 * rbvae_hmm_forward: y_0 = pi e_0 (element-wise), y_t = DOT(alpha_(t-1), A) e_t, c_t = SUM(y_t), alpha_t = y_t / c_t,
 * ll_t = log c_t + m_t.  alpha f64 [N][K], ll f64 [N].
 * rbvae_hmm_backward: beta_(N-1) = 1 / K, x = e_(t+1) beta_(t+1) (element-wise), y_ti = sum_j A_ij x_j with j ascending from
 * zero, beta_t = y_t / SUM(y_t): its own normalisation, independent of c.  beta f64 [N][K].
 * Both run over blocks of block_rows consecutive rows (rbvae_hmm_block_rows() = 64 is the default; ceil(N / block_rows)
 * blocks; block_rows >= N is the plain recursion in one launch), in three launches.  (i) For every block but the last
 * (backward: the first) and every state i, the unit vector of state i is carried through the block's rows by the step above,
 * u = y / SUM(y) after every row (zeros once SUM(y) = 0) with s_i = the sum of log SUM(y) over the rows in the order they are
 * taken (-inf once dead); the block that holds the recursion's first row carries the recursion itself.  (ii) One wave walks
 * the blocks in order: the vector v that enters block b leaves it as y / SUM(y) (zeros where that is 0) with
 * y_j = sum_i w_i u_ij, i ascending from zero, w_i = v_i exp(s_i - max_i s_i), 0 where s_i = -inf.  (iii) Every block takes
 * the plain recursion from the vector that enters it and writes its rows.  ws: rbvae_hmm_ws_bytes(N, K, block_rows) =
 * 8 max(blocks (K K + 2 K), N + xblocks K K) bytes, xblocks = min(256, ceil(N / 256)).
 * rbvae_hmm_posterior: gamma_kt = (alpha_tk beta_tk) / g_t, g_t = sum_k alpha_tk beta_tk with k ascending from zero; gamma
 * f64 [K][N] (component-major, as rbvae_gmm_mstep reads it).  n_t(i, j) = (alpha_ti A_ij) (e_(t+1)j beta_(t+1)j),
 * Z_t = sum_i sum_j n_t(i, j), one running sum from zero with i ascending and j ascending inside it.  xi f64 [K][K]:
 * Xi_ij = sum_t n_t(i, j) / Z_t over t = 0 .. N - 2 in two stages like the M-step: xblocks blocks of ceil(N / xblocks)
 * consecutive rows, a cell's partial added in ascending row order from zero, the partials in block order from zero.
 * A_new_ij = (Xi_ij + eps / K) / (sum_j Xi_ij + eps), j ascending from zero, eps = 10 * 2^-52 (a state without mass gets a
 * uniform row); pi_new_k = gamma_k0.  A_new may be A and pi_new pi.  Every g_t and Z_t that is 0 or not finite counts into
 * status.
 * rbvae_hmm_viterbi: log_pi f64 [K] and log_A f64 [K][K] come from the host (log 0 = -inf).  d_0j = log_pi_j + lb_j0;
 * d_tj = max_i(d_(t-1)i + log_A_ij) + lb_jt, back_tj = the lowest i that attains the maximum (back_0j = 0); the last state
 * is the lowest j that attains max_j d_(N-1)j, score[0] that maximum; path_(t-1) = back_t[path_t].  back uint8 [N][K],
 * path int32 [N].  Only additions and comparisons. */
int rbvae_hmm_ok(int N, int L, int K);
int rbvae_hmm_block_rows(void);
size_t rbvae_hmm_ws_bytes(int N, int K, int block_rows);
int rbvae_hmm_emit(const float* X, int N, int L, const double* means, const double* prec_chol, int K, double* logb,
                   double* rowmax, double* e, const int* state, void* stream);
int rbvae_hmm_forward(const double* e, const double* rowmax, int N, int K, const double* pi, const double* A, int block_rows,
                      double* alpha, double* ll, int* status, void* ws, size_t ws_bytes, const int* state, void* stream);
int rbvae_hmm_backward(const double* e, int N, int K, const double* A, int block_rows, double* beta, int* status, void* ws,
                       size_t ws_bytes, const int* state, void* stream);
int rbvae_hmm_posterior(const double* alpha, const double* beta, const double* e, int N, int K, const double* A,
                        double* gamma, double* xi, double* A_new, double* pi_new, int* status, void* ws, size_t ws_bytes,
                        const int* state, void* stream);
int rbvae_hmm_viterbi(const double* logb, int N, int K, const double* log_pi, const double* log_A, unsigned char* back,
                      int* path, double* score, const int* state, void* stream);

/* ---- hidden Markov model over several sequences (csrc/hmm.hip) -----------------------------------------------
 * Several recordings of one task share one model.  The rows of S sequences are stacked in time order, X f32 [N][L] and every
 * per-row array as above; lengths int32 [S] with every length >= 1 and sum N.  rbvae_hmm_ok(N, L, K) holds for the stacked N
 * and 1 <= S <= N (rbvae_hmm_seq_ok); a single sequence may be shorter than K, down to one row.  Refusals, state, status (rows
 * counted from the start of the stack) and the arithmetic are the single-sequence entries': f64, never contracted, no
 * floating-point atomics, every sum in one fixed order, two runs bit-identical.  rbvae_hmm_emit and rbvae_bern_emit are per
 * row and serve unchanged.
 * Blocks restart at every sequence: sequence s, of n_s rows, is cut into ceil(n_s / block_rows) blocks counted from its own
 * first row (block_rows above N is taken as N), and the three launches of the recurrence treat every sequence as the
 * single-sequence entries treat theirs.  So on the rows of sequence s alpha, ll, beta, back, path and score[s] are bit-equal
 * to what rbvae_hmm_forward / _backward / _viterbi write for that sequence alone at the same block_rows (wherever they accept
 * it: n_s >= max(K, 2)), rows of one sequence never depend on another's values, and with S = 1 every output of every entry
 * here has the single-sequence entry's bytes.
 * rbvae_hmm_seq_forward: the first row of every sequence is y = pi e_t (element-wise); otherwise rbvae_hmm_forward's step;
 * ll_t as there.  rbvae_hmm_seq_backward: the last row of every sequence is beta = 1 / K, and the row before it reads e and
 * beta of that row only.  Launch (i) runs over the blocks of all sequences, a sequence's own first (backward: last) block
 * carrying its recursion; launch (ii) is one wave per sequence, walking that sequence's blocks (a sequence of one block has
 * nothing to pass on, one of two blocks nothing to combine: its second block takes the first's own recursion); launch (iii)
 * again over all blocks.
 * rbvae_hmm_seq_posterior: gamma as rbvae_hmm_posterior for every row.  Xi_ij is its two-stage sum over the stacked rows
 * (xblocks blocks of ceil(N / xblocks) rows, t ascending, the partials in block order) with the terms t that are the last row
 * of a sequence skipped: not computed, no Z_t, and status counts a bad Z_t only for the terms that exist.  A_new as there.
 * pi_new_k = (sum_s gamma_k,first(s)) / S: one running sum from zero with s ascending, then one division.
 * rbvae_hmm_seq_viterbi: rbvae_hmm_viterbi per sequence, one wave each: back of a first row is 0, the last state of sequence
 * s is the lowest j that attains the maximum of its last row, score f64 [S] holds those maxima.
 * The plan.  rbvae_hmm_seq_plan checks the host lengths (a length below 1, a sum other than N, a NULL pointer or a plan below
 * rbvae_hmm_seq_plan_bytes(N, S, block_rows): RBVAE_E_INVALID; S outside [1, N]: RBVAE_E_UNSUPPORTED; nothing is written),
 * builds the plan on the host and copies it to plan_dev on the stream, which it waits for.  int32, in this order:
 *   {S, N, block_rows, B}   B = sum_s ceil(n_s / block_rows), the blocks in use
 *   row [S + 1]             the first row of sequence s; row[S] = N
 *   end [N]                 1 where row t is the last of its sequence, else 0
 *   blk [S + 1]             the first block of sequence s; blk[S] = B
 *   seq [maxb]              the sequence of block b; maxb = min(N, ceil(N / block_rows) + S) >= B is the grid of launches (i), (iii)
 * rbvae_hmm_seq_plan_bytes = 4 (6 + 2 S + N + maxb).  The entries take the plan made for their N, S and block_rows (posterior
 * and Viterbi read row and end only, which do not depend on block_rows).  A kernel clamps every row, block and sequence index
 * it reads from the plan to the arrays' extent before it uses it (rows to [0, N), blocks to [0, maxb), sequences to [0, S)):
 * a stale or foreign plan gives wrong numbers but no access outside the arrays.
 * ws: rbvae_hmm_seq_ws_bytes(N, K, S, block_rows) = 8 max(maxb (K K + 2 K), N + xblocks K K) bytes for the block_rows of the
 * recurrence; every block of the grid has its slot, also those of one-block sequences, which use none (S = 30 000 short
 * sequences at K = 64 reserve 1 GB: choose block_rows >= the longest sequence there, or fewer states).  The posterior asks for
 * 8 (N + xblocks K K) bytes only, whatever block_rows. */
int rbvae_hmm_seq_ok(int N, int L, int K, int S);
size_t rbvae_hmm_seq_plan_bytes(int N, int S, int block_rows);
int rbvae_hmm_seq_plan(const int* lengths_host, int S, int N, int block_rows, void* plan_dev, size_t plan_bytes, void* stream);
size_t rbvae_hmm_seq_ws_bytes(int N, int K, int S, int block_rows);
int rbvae_hmm_seq_forward(const double* e, const double* rowmax, int N, int K, const double* pi, const double* A,
                          int block_rows, const void* plan, int S, double* alpha, double* ll, int* status, void* ws,
                          size_t ws_bytes, const int* state, void* stream);
int rbvae_hmm_seq_backward(const double* e, int N, int K, const double* A, int block_rows, const void* plan, int S,
                           double* beta, int* status, void* ws, size_t ws_bytes, const int* state, void* stream);
int rbvae_hmm_seq_posterior(const double* alpha, const double* beta, const double* e, int N, int K, const void* plan, int S,
                            const double* A, double* gamma, double* xi, double* A_new, double* pi_new, int* status, void* ws,
                            size_t ws_bytes, const int* state, void* stream);
int rbvae_hmm_seq_viterbi(const double* logb, int N, int K, const void* plan, int S, const double* log_pi, const double* log_A,
                          unsigned char* back, int* path, double* score, const int* state, void* stream);

/* ---- Bernoulli models of the hard codes (csrc/bernoulli.hip) -------------------------------------------------
 * A state is a vector of bit probabilities: theta f64 [K][L], with logt = log theta and logf = log(1 - theta) as the M-step
 * writes them.  The codes are bit-packed, bits uint32 [N][4] (16-byte aligned): bit l of row i sits in word l / 32 at
 * position l % 32, bits from L upward are zero.  bernoulli.py drives a mixture with rbvae_bern_estep / _mstep and
 * rbvae_gmm_decide, and a hidden Markov model with rbvae_bern_emit, rbvae_hmm_forward / _backward / _posterior,
 * rbvae_bern_mstep on the posterior and rbvae_gmm_decide.  The limits are the mixture's: 1 <= L <= 128, 1 <= K <= 256,
 * K <= N <= 1048576 and N K <= 2^26 (rbvae_bern_ok = rbvae_gmm_ok; rbvae_bern_pack takes K = 1); rbvae_bern_emit also needs
 * rbvae_hmm_ok(N, L, K).  Anything else makes every entry return RBVAE_E_UNSUPPORTED without a launch; a NULL pointer or a
 * prior that is not > 0 (NaN included) RBVAE_E_INVALID.  All arithmetic is f64, never contracted; exp and log are the device
 * library's.  No floating-point atomics: every sum has one fixed order and two runs agree bit for bit.
 *
 * state is the mixture's int32 [4] = {done, n_iter, why, 0} and may be NULL; with done set emit, estep and mstep return
 * without writing anything.  rbvae_bern_pack takes no state.
 * rbvae_bern_pack: bit l of row i = codes[i][l] > 0.5 (symbols.code_symbols' rule; NaN gives 0); codes f32 [N][L]; each row is
 * one 16-byte store.
 * rbvae_bern_emit: lb_kt = sum_l (bit_tl ? logt_kl : logf_kl) with l ascending from zero, a running sum from zero: selections
 * and additions only.  logb f64 [K][N] = lb; rowmax f64 [N]: m_t = max_k lb_kt; e f64 [N][K]: e_tk = exp(lb_kt - m_t):
 * rbvae_hmm_emit's layouts, so the recursions run unchanged.
 * rbvae_bern_estep: lp_ik = (the sum above) + logw_k, added last; m_i = max_k lp_ik; lognorm_i = m_i + log(sum_k exp(lp_ik -
 * m_i)) with k ascending from zero; resp_ki = exp(lp_ik - lognorm_i), resp f64 [K][N] (component-major); label_i = the k of the
 * largest lp_ik (a tie goes to the lower k).  lognorm f64 [N]; resp and label int32 [N] may be NULL.  resp is first used to
 * hold lp.  In both entries the two log tables pass through LDS rbvae_bern_chunk_components(L) = 2048 / L components at a time.
 * rbvae_bern_mstep: two stages, blocked as rbvae_gmm_mstep's first pass: min(256, ceil(N / 256)) blocks of ceil(N / blocks)
 * consecutive rows; each cell's partial is added in ascending row order from zero, the partials then in block order from
 * zero.  S_kl = sum_i resp_ki over the rows whose bit l is set (no product: the term is added or not); nk_k = sum_i resp_ki;
 * theta_kl = (S_kl + prior) / (nk_k + 2 prior); logt_kl = log theta_kl; logf_kl = log(((nk_k - S_kl) + prior) / (nk_k + 2 prior));
 * weights_k = nk'_k / sum_k nk'_k with nk'_k = nk_k + 10 * 2^-52 and k ascending from zero; logw_k = log weights_k.  A component
 * without mass follows the same formulas: theta = 1 / 2.  ws: rbvae_bern_ws_bytes(N, L, K) = 8 blocks K (L + 1) bytes, the
 * block partials f64 [blocks][K][L + 1]: cell (k, l) holds the block's part of S_kl and cell (k, L) that of nk_k. */
int rbvae_bern_ok(int N, int L, int K);
int rbvae_bern_chunk_components(int L);
size_t rbvae_bern_ws_bytes(int N, int L, int K);
int rbvae_bern_pack(const float* codes, int N, int L, uint32_t* bits, void* stream);
int rbvae_bern_emit(const uint32_t* bits, int N, int L, const double* logt, const double* logf, int K, double* logb,
                    double* rowmax, double* e, const int* state, void* stream);
int rbvae_bern_estep(const uint32_t* bits, int N, int L, const double* logt, const double* logf, const double* logw, int K,
                     double* resp, double* lognorm, int* label, const int* state, void* stream);
int rbvae_bern_mstep(const uint32_t* bits, int N, int L, const double* resp, int K, double prior, double* weights,
                     double* logw, double* theta, double* logt, double* logf, double* ws, const int* state, void* stream);

/* ---- Density clustering on a bit-packed radius graph: DBSCAN (csrc/dbscan.hip) ---------------------------------
 * scikit-learn 1.7.2's DBSCAN in its order-free form: j is in N(i) iff d(i, j) <= eps (i itself included); row i is core iff
 * |N(i)| >= min_samples; the clusters are the connected components of the core rows under j in N(i), numbered in ascending
 * order of their smallest core index; a non-core row with a core neighbour takes the lowest id among its core neighbours'
 * clusters; every other non-core row is -1.  The graph is a bit matrix adj uint64 [N][W], W = rbvae_dbscan_words(N) =
 * ceil(N / 64): bit j % 64 of word j / 64 of row i says j in N(i); bits of columns >= N are zero.  The limits are
 * 2 <= N <= 65536 and 1 <= L <= 128 (rbvae_dbscan_ok; the entries without L take L = 1); anything else makes every entry
 * return RBVAE_E_UNSUPPORTED without a launch, a NULL pointer, min_samples < 1, eps2 negative or NaN, or max_bits outside
 * [0, L] RBVAE_E_INVALID.  Distances are f64 from rbvae_knn's device function; everything behind the comparison is integer.
 * No floating-point atomics; the integer atomicMin of a round gives the same buffer in any order, so two runs agree bit for
 * bit, the number of rounds included.
 *
 * rbvae_dbscan_adj: X f32 [N][L]; the bit is set iff d2(i, j) = sum_l (x_il - x_jl)^2 <= eps2 with l ascending, each
 * difference exact in f64, each square and each addition rounded once (rbvae_knn's d2, which is symmetric in i and j); a NaN
 * compares false.  A workgroup owns one word (64 columns, a lane each, held in LDS as f32 [L][65]) and 256 query rows, which
 * pass through LDS as f64 sixteen at a time; a wave's ballot is the word.  cnt int32 [N]: the row's popcount, from a second
 * launch over adj.
 * rbvae_dbscan_adj_bits: bits uint32 [N][4] as rbvae_bern_pack writes them (bits from L upward zero); the bit is set iff
 * popcount(bits_i xor bits_j) <= max_bits.  cnt as above.
 * rbvae_dbscan_core: core_mask uint64 [W]: bit i is cnt[i] >= min_samples (bits >= N zero); f int32 [N]: i for a core row,
 * N for the others.
 * rbvae_dbscan_round: one synchronous (Jacobi) round of FastSV over the core rows, edges adj[u] & core_mask:
 *   gf[u] = f_in[f_in[u]]; mn[u] = min of gf[v] over the core v in N(u), v != u (N without one); f_out = f_in; then
 *   atomicMin(f_out[f_in[u]], mn[u]), atomicMin(f_out[u], mn[u]), atomicMin(f_out[u], gf[u]) for every core u.
 * Three launches: the copy, the minima, and one workgroup that compares.  state int32 [4] = {done, n_rounds, changed, 0}:
 * with done set nothing is written; otherwise n_rounds += 1, changed = (any f_out[u] != f_in[u]) and done = !changed.  The
 * fixed point is f[u] = the smallest core index of u's component.  f_in and f_out are distinct int32 [N]; an entry of f_in
 * outside [0, N) is read as N and never followed.
 * rbvae_dbscan_labels: f is the fixed point.  Roots are the core rows with f[i] == i; cid(r) = the number of roots below r,
 * from the popcounts of a root mask and a scan of its at most 1024 word totals in one workgroup; n_clusters[0] = the number
 * of roots.  labels int32 [N]: cid(f[i]) for a core row; for the others cid(min f[j] over the core j in N(i)), or -1
 * without one (cid is monotone in the root, so the smallest root gives the lowest id).  ws: rbvae_dbscan_ws_bytes(N) = 16 W
 * bytes, 8-byte aligned: the root mask uint64 [W], then the words' exclusive totals int32 [W]. */
int rbvae_dbscan_ok(int N, int L);
int rbvae_dbscan_words(int N);
size_t rbvae_dbscan_ws_bytes(int N);
int rbvae_dbscan_adj(const float* X, int N, int L, double eps2, unsigned long long* adj, int* cnt, void* stream);
int rbvae_dbscan_adj_bits(const uint32_t* bits, int N, int L, int max_bits, unsigned long long* adj, int* cnt,
                          void* stream);
int rbvae_dbscan_core(const int* cnt, int N, int min_samples, unsigned long long* core_mask, int* f, void* stream);
int rbvae_dbscan_round(const unsigned long long* adj, const unsigned long long* core_mask, int N, const int* f_in,
                       int* f_out, int* state, void* stream);
int rbvae_dbscan_labels(const unsigned long long* adj, const unsigned long long* core_mask, const int* f, int N,
                        int* labels, int* n_clusters, void* ws, void* stream);

/* ---- Density clustering at every radius: HDBSCAN* (csrc/hdbscan.hip) -------------------------------------------
 * Campello, Moulavi, Zimek and Sander 2015, Algorithm 1 with "edges of equal weight are removed simultaneously", in an
 * order-free form (DESIGN.md section 7 says why scikit-learn's HDBSCAN cannot be the specification where weights tie).
 * d2(i, j) is rbvae_knn's; core2[i] is the (m - 1)-th smallest d2(i, j) over j != i, column m - 2 of rbvae_knn(X, k = m - 1),
 * and 0 for m = 1 (min_samples = m counts the row itself); w2(i, j) = max(core2[i], core2[j], d2(i, j)).  Edges are totally
 * ordered by the key (w2, lo, hi), lo = min(i, j), hi = max(i, j); under a strict total order the minimum spanning tree is
 * unique, and that edge set is what the device computes.  The limits are 2 <= N <= 16384 and 1 <= L <= 128 (rbvae_mst_ok;
 * rbvae_mst_start takes L = 1); anything else makes the two device entries return RBVAE_E_UNSUPPORTED without a launch; a
 * NULL pointer, a buffer that is not aligned to its element (ws, core2, w2: 8 bytes), or two buffers that overlap (X and core2,
 * which are only read, excepted) RBVAE_E_INVALID.  A refused call writes nothing.  X and core2 must be finite: the entries do
 * not look (density.py does).  No floating-point atomics.
 *
 * rbvae_mst_ws_bytes(N): the size of ws, 128 N bytes (0 outside the limits); 8-byte aligned; its content between the calls
 * belongs to the library.
 * rbvae_mst_start: comp int32 [N] = 0 .. N - 1 (every row its own component), state int32 [4] = {done = 0, n_rounds = 0,
 * n_components = N, n_edges = 0}, and the per-component minima in ws cleared.
 * rbvae_mst_round: one Boruvka round, five launches; with done set every kernel returns at once and nothing is written.
 *   search   for every row i the least (w2(i, j), j) over the rows j with comp[j] != comp[i] -- for a fixed i that is the
 *            order of the key.  A workgroup owns 32 query rows (f64 in LDS, read as a broadcast) and one of up to 8 slices of
 *            the columns, which pass through LDS 64 at a time as f32 [L][65]; a lane owns a column of the tile, carries four
 *            query rows side by side and keeps each row's running minimum in registers; one butterfly per row at the end.
 *   minima   a thread per row merges the slices in their order, then atomicMin of the bits of w2 (a non-negative f64 orders
 *            as a uint64) into its component; then, among the rows that hold that minimum, atomicMin of (lo << 32 | hi).
 *            Both results are the same in whatever order the atomics land.
 *   hook     component c (c = comp[c]) hooks onto the component t at the other end of its edge, unless t chose the same edge
 *            and c < t; every component appends its edge at n_edges++, but of two that chose the same edge only the side
 *            that holds lo does, so that edge is emitted once.  (The keys do not increase along c -> t(c) -> ...; around a cycle
 *            they are equal, the order is strict, so the cycle is one edge and has two members.)
 *   merge    one workgroup: pointer jumping to the roots, comp[i] = the smallest row of i's new component, n_rounds += 1,
 *            n_components, and done = (n_components == 1).
 * edges int32 [N - 1][2] (lo < hi) and w2 f64 [N - 1] fill up over the rounds, at most ceil(log2 N) of them; their order is
 * the one in which the counter was handed out.  THE CALLER SORTS them by (w2, lo, hi) (density.mutual_reachability_mst does,
 * on the device): the key is a strict total order, so the sorted list, like n_rounds, is the same bit for bit in every run. */
int rbvae_mst_ok(int N, int L);
size_t rbvae_mst_ws_bytes(int N);
int rbvae_mst_start(int N, int* comp, int* state, void* ws, void* stream);
int rbvae_mst_round(const float* X, const double* core2, int N, int L, int* comp, int* edges, double* w2, int* state,
                    void* ws, void* stream);
/* The first launch of rbvae_mst_round alone, for timing it (tools/run_hdbscan.py): same arguments and checks; it writes the
 * slices' minima into ws and nothing else, so it may be repeated before the round proper. */
int rbvae_mst_search(const float* X, const double* core2, int N, int L, int* comp, int* edges, double* w2, int* state,
                     void* ws, void* stream);
/* The host half: HOST pointers, no stream, no GPU call (they run on a machine without one), nothing retained.
 * edges int32 [N - 1][2] and d f64 [N - 1] = sqrt(w2), sorted by the key.  They must span 0 .. N - 1 as a tree (checked by
 * union-find) and d must be finite, non-negative and ascending; anything else, min_cluster_size outside [2, N], a method other
 * than 0 (excess of mass) or 1 (leaves), a negative or NaN cut_distance or a NULL pointer returns RBVAE_E_INVALID, N outside
 * [2, 16384] RBVAE_E_UNSUPPORTED, and nothing is written.  Iterative throughout (a chain's dendrogram is N deep); O(N log N).
 *
 * rbvae_hdbscan_tree.  Levels: the distinct values of d, ascending; lambda = 1 / d, +inf at d = 0.  Dendrogram: all edges of
 * one level are added at once, and every component that absorbed r >= 2 older ones is one node with r children.  Condensed
 * tree, top down: the root cluster is born at lambda = 0; at a node visited as part of cluster C at lambda, a child is big
 * when it has >= min_cluster_size rows; with >= 2 big children C ends and each is a new cluster born at lambda, with exactly
 * one C continues into it, with none C ends; the rows of the other children leave C at lambda.  stability(C) = the sum over
 * C's levels, lambda ascending, of (lambda - birth(C)) * n, n the whole number of rows leaving C there (those of the big
 * children of a split included): one product and one addition per level.  lambda_max(C) is C's last level.  method 0: the
 * clusters deepest first, the root left out: with children whose stabilities (propagated, added in table order from 0) sum to
 * MORE than C's, C is dropped and takes that sum; otherwise C is selected and its descendants are dropped.  method 1: the
 * clusters without children, the root left out.  A row takes the nearest selected cluster from the one it left upwards, else
 * -1; the selected clusters are numbered by their smallest row, ascending.  prob = 0 for -1; 1 where lambda_max(C) == 0 or
 * the row's lambda is inf; otherwise min(lambda_row, lambda_max(C)) / lambda_max(C).
 * The cluster table (every cl_* buffer holds N entries; n_table[0] = the number written, at least 1): the root first, then
 * (birth, smallest row) ascending, so a parent stands before its children; cl_parent (-1 for the root), cl_birth,
 * cl_lambda_max, cl_stability (a cluster's own, not the propagated one), cl_size, cl_selected (0 / 1), cl_min_row.
 * rbvae_hdbscan_cut (DBSCAN* at one radius): the components of the edges with d <= cut_distance; those with fewer than
 * min_cluster_size rows are -1, the others numbered by their smallest row; n_clusters[0] their number. */
int rbvae_hdbscan_tree(const int* edges, const double* d, int N, int min_cluster_size, int method, int* labels, double* prob,
                       int* cl_parent, double* cl_birth, double* cl_lambda_max, double* cl_stability, int* cl_size,
                       int* cl_selected, int* cl_min_row, int* n_table);
int rbvae_hdbscan_cut(const int* edges, const double* d, int N, double cut_distance, int min_cluster_size, int* labels,
                      int* n_clusters);

/* ---- Two sequences aligned: dynamic time warping (csrc/dtw.hip) -------------------------------------------------
 * Sakoe and Chiba 1978 with the symmetric step pattern of unit weights, as dtw-python's "symmetric1" and tslearn's dtw_path
 * state it; tests/_dtw_ref.py restates every operation.  X has N rows and Y has M rows, both in time order; 1 <= N, M <= 16384,
 * 1 <= L <= 128, metric in 0 .. 2, window = -1 or |N - M| <= window (and then subsequence = 0), subsequence in {0, 1}
 * (rbvae_dtw_ok); anything else makes every entry return RBVAE_E_UNSUPPORTED without a launch, a NULL pointer (table
 * excepted) RBVAE_E_INVALID.  X and Y must be finite: the entries do not look (alignment.py does).
 *
 * Cell cost d(i, j).  metric 0 (sqeuclidean), X f32 [N][L] and Y f32 [M][L]: sum_l (x_il - y_jl)^2 in f64 with l ascending,
 * each difference exact, each square and each addition rounded once, never contracted (rbvae_knn's d2).  metric 1
 * (euclidean): the correctly rounded f64 square root of that sum.  metric 2 (hamming, rbvae_dtw_fill_bits), uint32 [.][4] as
 * rbvae_bern_pack writes them: the popcount of the XOR of the two rows, an exact f64; L is only checked.
 * Table.  D[0][0] = d(0, 0); D[i][j] = d(i, j) + min(D[i-1][j-1], D[i-1][j], D[i][j-1]), a predecessor outside the table
 * being absent: one f64 addition per cell.  The predecessor is the first of diagonal, up (i - 1, j), left (i, j - 1) whose
 * value is <= the other two.  dirs uint8 [N][ceil(M / 4)] holds it in 2 bits per cell, cell j in bits 2 (j mod 4) of byte
 * j / 4 of row i: 0 diagonal, 1 up, 2 left, 3 start / none; the bits of the columns from M on in a row's last byte are 3.
 * Band.  window = w >= 0: a cell with |i - j| > w holds +inf and direction 3 and is no predecessor; window = -1: no band.
 * Subsequence (open begin and end on Y).  D[0][j] = d(0, j) with direction 3 for every j; the other rows as above; the end is
 * the j with the smallest D[N-1][j], the lowest j on a tie; the path runs from there back to row 0.
 *
 * rbvae_dtw_tile_rows / _cols: the edges of the tile a workgroup owns (tests place shapes on them).
 * rbvae_dtw_ws_bytes(N, M): the size of ws, 8-byte aligned (0 outside the limits): a frontier row f64 [M], a frontier column
 * f64 [N] and one corner per tile.  rbvae_dtw_dirs_bytes(N, M) = N ceil(M / 4).
 * rbvae_dtw_fill / rbvae_dtw_fill_bits: one launch per anti-diagonal of tiles on the caller's stream -- the launch order is
 * the only dependency between workgroups, none waits for another -- behind one fill launch where there is a band, whose
 * tiles wholly outside it are not launched.  They write dirs and last_row f64 [M] = D[N-1][.], and, where table is not NULL,
 * the whole D f64 [N][M] (tests and small inputs; the product path passes NULL and never stores N M doubles).
 * rbvae_dtw_trace: one workgroup walks dirs from the end cell (N - 1, M - 1), or (N - 1, end_j) in subsequence mode, to the
 * cell with direction 3.  path int32 [N + M - 1][2] (8-byte aligned): the pairs (i, j) ascending in rows 0 .. len - 1; the
 * rows from len on are scratch and hold no meaning afterwards.  state int32 [3] = {len, start_j, end_j}; cost f64 [1] =
 * last_row[end_j].  dirs that do not lead to row 0 (and column 0 without subsequence) inside N + M - 1 cells give len =
 * start_j = -1 and no path. */
int rbvae_dtw_ok(int N, int M, int L, int metric, int window, int subsequence);
int rbvae_dtw_tile_rows(void);
int rbvae_dtw_tile_cols(void);
size_t rbvae_dtw_ws_bytes(int N, int M);
size_t rbvae_dtw_dirs_bytes(int N, int M);
int rbvae_dtw_fill(const float* X, int N, const float* Y, int M, int L, int metric, int window, int subsequence,
                   unsigned char* dirs, double* last_row, double* table, void* ws, void* stream);
int rbvae_dtw_fill_bits(const uint32_t* xbits, int N, const uint32_t* ybits, int M, int L, int window, int subsequence,
                        unsigned char* dirs, double* last_row, double* table, void* ws, void* stream);
int rbvae_dtw_trace(const unsigned char* dirs, const double* last_row, int N, int M, int subsequence, int* path, int* state,
                    double* cost, void* stream);

/* ---- Many sequences aligned: batched pairs, path ranges and the DBA update (csrc/dtw.hip; since version 111) ----
 * Two stacks and a pair list.  X is f32 [sum_a len_x[a]][L] with len_x int32 [Sx], Y f32 [sum_b len_y[b]][L] with len_y
 * int32 [Sy]: the rows of a sequence are contiguous and in time order, sequence s starts at the row that the lengths before
 * it add up to.  For metric 2 the stacks are uint32 [.][4] as rbvae_bern_pack writes them.  pairs int32 [P][2] holds
 * (a, b): sequence a of the X stack (the table's N = len_x[a] rows) against sequence b of the Y stack (its M = len_y[b]
 * columns).  All pairs of one stack pass the stack twice; self pairs and repeated pairs are allowed.  len_x, len_y and
 * pairs are HOST arrays everywhere below.  Limits (rbvae_dtw_pairs_ok = 1): Sx, Sy >= 1, 1 <= every length <= 16384, each
 * stack at most 2^31 - 1 rows, 1 <= L <= 128, 1 <= P <= 65535, metric 0 .. 2, 0 <= a < Sx, 0 <= b < Sy.  There is no
 * band and no subsequence mode.  Anything outside makes the entries that take the lengths return RBVAE_E_UNSUPPORTED
 * without a launch and without a write; a NULL pointer RBVAE_E_INVALID.
 *
 * The promise.  For every pair, dirs, last_row, path, state and cost are bit for bit what rbvae_dtw_fill(_bits) followed by
 * rbvae_dtw_trace (window = -1, subsequence = 0, table = NULL) write for that pair alone: the same cell cost, table, tie
 * order and packing as stated above.  They do not depend on which other pairs are in the batch or on their order; P = 1
 * gives the single-pair entries' bytes.
 *
 * Layout.  Pair p's block of each output has exactly the single-pair entry's layout -- dirs uint8 [N][ceil(M / 4)],
 * last_row f64 [M], path int32 [N + M - 1][2], ws as rbvae_dtw_ws_bytes(N, M) (frontier row [M], frontier column [N], one
 * corner per tile: each pair has its own) -- and the blocks follow each other in pair order.  A dirs block starts at a
 * multiple of 16 bytes: its size is N ceil(M / 4) rounded up to 16, and the padding bytes are never written.
 * rbvae_dtw_pairs_sizes writes the host arrays int64 [P + 1] dirs_off (bytes), last_off (doubles), ws_off (bytes) and
 * path_off (rows of two int32): entry p is where pair p's block starts and entry P the total; totals size_t [4] =
 * {bytes of dirs, doubles of last_row, bytes of ws, rows of path}.  state is int32 [P][3] and cost f64 [P], pair p's at 3 p
 * and p, each as rbvae_dtw_trace writes it.
 *
 * Plan.  rbvae_dtw_pairs_plan checks the lengths and pairs as above, needs plan_bytes >= rbvae_dtw_pairs_plan_bytes(P) =
 * 8 (4 + 10 P) (0 for P outside its limits; RBVAE_E_INVALID when smaller), builds the plan on the host, copies it to
 * plan_dev on the stream and waits for the copy.  The plan is int64: {P, rows of the X stack, rows of the Y stack, 0}, then per
 * pair {first row in X, first row in Y, N, M, tiles down, tiles across, dirs_off, last_off, ws_off / 8, path_off}.  launch
 * (host int32 [2]) receives what the fill loops over: the number of tile anti-diagonals of the largest pair, max_p (tiles
 * down + tiles across - 1), and the most tiles any pair has on one anti-diagonal, max_p min(tiles down, tiles across).
 *
 * rbvae_dtw_pairs_fill / _fill_bits: X [Nx][L], Y [Ny][L] (or the packed stacks), the plan of these stacks and pairs,
 * n_diag and max_tiles as the plan returned them, dirs of dirs_bytes bytes, last_row of last_n doubles, ws of ws_bytes
 * bytes, all at least the totals above.  ONE launch per tile anti-diagonal d = 0 .. n_diag - 1 for all pairs together, grid
 * (min(d + 1, max_tiles), P): workgroup (x, p) owns the x-th tile of pair p on diagonal d and returns before any work where
 * the pair has fewer.  The launch order on the stream is the only dependency between workgroups: no flags in memory, no
 * workgroup waits for another, no cooperative launch, no floating-point atomics.  Nx, Ny < 1, L, metric, P outside the
 * limits, n_diag outside [1, 511], max_tiles outside [1, 256] or metric 2 given to rbvae_dtw_pairs_fill:
 * RBVAE_E_UNSUPPORTED.  Every index a kernel reads from the plan is clamped to Nx, Ny, dirs_bytes, last_n, ws_bytes (and
 * path_rows below), and a pair whose block fits nowhere is skipped: a plan made for other arrays gives wrong numbers and no
 * access outside the arrays given.
 * rbvae_dtw_pairs_trace: one workgroup per pair walks its dirs block from (N - 1, M - 1) as rbvae_dtw_trace does and writes
 * its block of path (path_rows rows in all, 8-byte aligned), state [p] and cost [p].
 *
 * rbvae_dtw_path_ranges: from one pair's ascending path (as the trace left it, state its int32 [3] on the device: the length
 * is read there, not on the host), lo int32 [n] and hi int32 [n]: the first and the last j aligned with row i.  One thread
 * per path element writes lo[i] where the previous element has another i (or there is none) and hi[i] where the next one
 * has; every row of a global path has exactly one of each, so no atomics.  state[0] < 1 writes nothing.  (n, m) outside
 * 1 .. 16384: RBVAE_E_UNSUPPORTED.
 *
 * rbvae_dtw_barycenter_update: one step of DTW barycenter averaging (Petitjean, Ketterlin and Gancarski 2011) under squared
 * Euclidean distance.  The template is the X side of the P pairs of the plan (T rows; the plan's pairs in order are the
 * sequences s = 0 .. P - 1 whose Y rows are averaged), lo and hi are int32 [P][T] as rbvae_dtw_path_ranges wrote them for
 * each pair.  For every row i < T and coordinate l < L: acc = 0.0 in f64; for p ascending, for j from lo[p][i] to hi[p][i]
 * ascending, acc += (double)y_p[j][l], every addition rounded once; cnt_i = sum_p (hi[p][i] - lo[p][i] + 1) (>= P on
 * global paths); out[i][l] = (float)(acc / (double)cnt_i): one f64 division, then one rounding to f32; count int32 [T] =
 * cnt_i.  One thread per (i, l), l fastest; no atomics.  lo and hi are clamped to the pair's rows.  Ny < 1, L outside
 * 1 .. 128, P outside 1 .. 65535, T outside 1 .. 16384: RBVAE_E_UNSUPPORTED. */
int rbvae_dtw_pairs_ok(const int* len_x, int Sx, const int* len_y, int Sy, const int* pairs, int P, int L, int metric);
int rbvae_dtw_pairs_sizes(const int* len_x, int Sx, const int* len_y, int Sy, const int* pairs, int P, int64_t* dirs_off,
                          int64_t* last_off, int64_t* ws_off, int64_t* path_off, size_t* totals);
size_t rbvae_dtw_pairs_plan_bytes(int P);
int rbvae_dtw_pairs_plan(const int* len_x, int Sx, const int* len_y, int Sy, const int* pairs, int P, void* plan_dev,
                         size_t plan_bytes, int* launch, void* stream);
int rbvae_dtw_pairs_fill(const float* X, int Nx, const float* Y, int Ny, int L, int metric, const void* plan, int P, int n_diag,
                         int max_tiles, unsigned char* dirs, size_t dirs_bytes, double* last_row, size_t last_n, void* ws,
                         size_t ws_bytes, void* stream);
int rbvae_dtw_pairs_fill_bits(const uint32_t* xbits, int Nx, const uint32_t* ybits, int Ny, int L, const void* plan, int P,
                              int n_diag, int max_tiles, unsigned char* dirs, size_t dirs_bytes, double* last_row,
                              size_t last_n, void* ws, size_t ws_bytes, void* stream);
int rbvae_dtw_pairs_trace(const unsigned char* dirs, size_t dirs_bytes, const double* last_row, size_t last_n, const void* plan,
                          int P, int* path, size_t path_rows, int* state, double* cost, void* stream);
int rbvae_dtw_path_ranges(const int* path, const int* state, int n, int m, int* lo, int* hi, void* stream);
int rbvae_dtw_barycenter_update(const float* Y, int Ny, int L, const void* plan, int P, const int* lo, const int* hi, int T,
                                float* out, int* count, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RBVAE_HIP_H */
