/* librbvae_dbg -- selectors of kernel forms that compute the same result (bit-identity tests, same-GPU A/B timing), beside
 * the ones in include/rbvae_dbg.h.  Not part of the product ABI (include/rbvae_hip.h). */
#ifndef RBVAE_DBG_VARIANTS_H
#define RBVAE_DBG_VARIANTS_H
#ifdef __cplusplus
extern "C" {
#endif
/* which form of wgrad_gemm_k rbvae_wgrad_gemm (librbvae_hip) launches for its one-workgroup-per-CU bf16 problems (at most 256
 * workgroups; the two-per-CU double-buffer launches and the f32 kernels have one form): 0 (default) the product dispatch
 * (the 12-wave form for K loops of at least 16 steps, the 8-wave form below), 1 the 8-wave form (every wave stages and
 * multiplies), 2 the 12-wave form (waves 0-7 multiply, waves 8-11 issue the LDS-DMA) -- the same sums in the same order, so
 * the slabs are equal bit for bit.  Returns the previous value. */
int rbvae_dbg_wgrad_gemm_variant(int v);

/* which path rbvae_deconv_last_fwd_bwd_ok (librbvae_hip) offers its callers: 0 (default) the one-launch kernel where it
 * covers the shape, 1 never (the query answers 0: rbvae_deconv_last_fused + rbvae_deconv_last_dgrad_fused) -- the same
 * values and sums bit for bit.  Returns the previous value. */
int rbvae_dbg_deconv_last_variant(int v);

#ifdef __cplusplus
}
#endif
#endif /* RBVAE_DBG_VARIANTS_H */
