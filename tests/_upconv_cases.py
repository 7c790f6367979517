"""The cases of tests/test_ldm_decoder_gpu.py for csrc/upconv.hip: case tables, the host restatement of the dispatch
(rbvae_upconv3x3_halo_ok, the work items of upconv_halo_k), and the float64 operands and references (CPU only: the GPU
tests upload what is built here).

  rbvae_upconv_fold        w f32 [Co][Ci][3][3] -> Wf [Co][16][Kc], bit for bit _ldm_decoder_ref.fold_upconv in float32
  rbvae_upconv3x3_halo     16 x 16 low-resolution pixels x 128 channels x one parity class per workgroup; the reference is
                           the four-class form in float64 from the DEVICE's folded weights, K = 4 Kc products per output
  rbvae_gather_gemm        the same sums through the four-class descriptor (the fallback and the baseline)
  rbvae_latent_rows / rbvae_decoded_to_image   byte for byte against torch float32 on the CPU"""
import torch

import _bounds as B
import _ldm_decoder_ref as DR
from _conv_cases import DTYPE_ID, KE, TDT, cdiv      # noqa: F401  (re-exported for the test module)

UC_T, UC_BN = 16, 128


def uc_ok(dtype, N, h, w, Kc, Nout):
    """rbvae_upconv3x3_halo_ok (csrc/upconv.hip): both map sides >= 5, whole K slices, whole 128-channel tiles, < 2^30
    output rows and work items."""
    if dtype not in KE or Kc <= 0 or Kc % KE[dtype] or Nout <= 0 or Nout % UC_BN:
        return False
    if N < 1 or h < 5 or w < 5 or N * 4 * h * w >= 1 << 30:
        return False
    return uc_items(N, h, w, Nout) < 1 << 30


def uc_items(N, h, w, Nout):
    """workgroups of a launch: pixel blocks x channel tiles x 4 classes"""
    return N * cdiv(h, UC_T) * cdiv(w, UC_T) * (Nout // UC_BN) * 4


def uc(id, dtype, N, h, w, Kc, Nout, lda=0, ldo=0, bias=1, addend=0):
    return dict(id=id, dtype=dtype, N=N, h=h, w=w, Kc=Kc, Nout=Nout, lda=Kc + lda, ldo=Nout + ldo, bias=bias, addend=addend)


UC_CASES = [
    uc("bf16_8x8_s1", "bf16", 1, 8, 8, 64, 128),
    uc("bf16_5x11_ragged_s2", "bf16", 2, 5, 11, 128, 128, lda=8, ldo=8),
    uc("bf16_17x9_past_tile_edge_n256", "bf16", 1, 17, 9, 64, 256, ldo=8),
    uc("bf16_8x8_s8_n512", "bf16", 1, 8, 8, 512, 512, bias=0),
    uc("bf16_16x16_addend", "bf16", 3, 16, 16, 128, 128, lda=64, addend=1),
    uc("bf16_5x5_smallest", "bf16", 1, 5, 5, 64, 128),
    uc("bf16_33x18_two_col_tiles", "bf16", 1, 33, 18, 64, 128, addend=1),
    uc("f32_8x8_s1", "f32", 1, 8, 8, 32, 128, lda=4),
    uc("f32_8x8_s2", "f32", 1, 8, 8, 64, 128, ldo=4, addend=1),
    uc("f32_8x8_s3", "f32", 1, 8, 8, 96, 128),
    uc("f32_5x5_smallest", "f32", 1, 5, 5, 32, 128, bias=0),
    uc("f32_17x9_n256", "f32", 2, 17, 9, 32, 256, addend=1),
]

# the first shape rbvae_upconv3x3_halo_ok refuses on each side of (5, 5, KE, 128): (dtype, N, h, w, Kc, Nout)
UC_REFUSED = [("bf16", 1, 4, 5, 64, 128), ("bf16", 1, 5, 4, 64, 128), ("bf16", 1, 8, 8, 32, 128), ("bf16", 1, 8, 8, 96, 128),
              ("bf16", 1, 8, 8, 64, 64), ("bf16", 1, 8, 8, 64, 192), ("f32", 1, 4, 12, 32, 128), ("f32", 1, 8, 8, 16, 128),
              ("f32", 1, 8, 8, 48, 128), ("f32", 1, 8, 8, 32, 120)]

# shapes only the gather form serves (narrow maps; Nout % 8 only)
GATHER_ONLY = [uc("bf16_4x12_narrow", "bf16", 1, 4, 12, 64, 128), uc("f32_2x3_n72", "f32", 2, 2, 3, 32, 72, ldo=4, addend=1),
               uc("bf16_1x1", "bf16", 3, 1, 1, 64, 64)]

FOLD_CASES = [(128, 64, 64), (256, 192, 192), (128, 4, 64)]          # (Co, Ci, Kc)


def uc_build(c):
    """Operands of a case, storage-rounded, on the CPU: x [N][Kc][h][w], A rows, w f32 [Nout][Kc][3][3] (what
    rbvae_upconv_fold reads), bias, addend rows."""
    tdt, N, Kc, Nout = TDT[c["dtype"]], c["N"], c["Kc"], c["Nout"]
    g = torch.Generator().manual_seed(sum(map(ord, c["id"])))
    x = torch.randn(N, Kc, c["h"], c["w"], generator=g).to(tdt)
    w = torch.randn(Nout, Kc, 3, 3, generator=g) / (9 * Kc) ** 0.5
    out = dict(x=x, A=B.rows(x), w=w, bias=None, addend=None, nhw=(N, 2 * c["h"], 2 * c["w"]), K=4 * Kc)
    if c["bias"]:
        out["bias"] = torch.randn(Nout, generator=g) * 0.5
    if c["addend"]:
        out["addend"] = torch.randn(N * 4 * c["h"] * c["w"], Nout, generator=g).to(tdt)
    return out


def uc_reference(c, d, wf, defect=None):
    """(ref, S, pre) rows [N 2h 2w][Nout] in float64 from the operands as stored and the folded weights wf [Nout][16][Kc] as
    the device wrote them.  defect: one of _ldm_decoder_ref.upconv_folded's, or "unfolded_w1" (CPU fold of w with the
    two-row sums cut to their first row, rounded like the device's)."""
    x = d["x"].double()
    if defect == "unfolded_w1":
        wf, defect = DR.fold_upconv(d["w"], defect="unfolded_w1").to(TDT[c["dtype"]]), None
    wf = wf.detach().cpu().double()
    ref = B.rows(DR.upconv_folded(x, wf, defect))
    S = B.rows(DR.upconv_folded(x.abs(), wf.abs(), defect))
    pre = None
    if d["bias"] is not None:
        ref, S = ref + d["bias"].double(), S + d["bias"].double().abs()
    if d["addend"] is not None:
        pre = ref                    # the addend meets the tile already rounded to the storage type: a second rounding
        ref = ref + d["addend"].double()
    return ref, S, pre


def image_values(dtype):
    """Inputs of rbvae_decoded_to_image [M][3]: -1, 1, 0, every 2k/255 - 1 with its float32 neighbours on both sides, and
    values far outside [-1, 1]; rounded to the storage type (the kernel sees stored values)."""
    k = torch.arange(256, dtype=torch.float64)
    edge = (2 * k / 255 - 1).float()
    inf = torch.tensor(float("inf"))
    vals = torch.cat([edge, torch.nextafter(edge, inf), torch.nextafter(edge, -inf),
                      torch.tensor([-1.0, 1.0, 0.0, -0.0, 1e3, -1e3, 3e38, -3e38, 1.0000001, -1.0000001, 0.999999, 2.5])])
    pad = (-vals.numel()) % 3
    vals = torch.cat([vals, torch.zeros(pad)])
    return vals.reshape(-1, 3).to(TDT[dtype])
