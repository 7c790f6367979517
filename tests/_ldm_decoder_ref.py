"""CPU restatement of the frozen LDM / Stable-Diffusion VAE decoder (TEST INFRASTRUCTURE, not product code), the
counterpart of oracle/ldm_oracle.py for the other direction.

Plain torch, any float dtype (the tests run it in float32 and float64):
  decode_first_stage           src/stable-diffusion/ldm/models/diffusion/ddpm.py:706-713 (z / 0.18215)
  AutoencoderKL.decode         src/stable-diffusion/ldm/models/autoencoder.py:330-333 (post_quant_conv 1x1, then the decoder)
  Decoder.forward              src/stable-diffusion/ldm/modules/diffusionmodules/model.py:535-568
  Upsample                     same file :42-57 (nearest x2, Conv2d 3x3 pad 1)
ResnetBlock / AttnBlock / Normalize / nonlinearity are ldm_oracle's.  Pinned by tests/golden/ldm_decoder.npz, which
tools/make_ldm_decoder_golden.py writes by running the reference's own Decoder class (random init: the pretrained weights
are not available offline).

Also here: the parity fold of Upsample (fold_upconv: the weights rbvae_upconv_fold writes, bit for bit in float32), the
four-class reference built from folded weights (upconv_folded), and rbvae_gather_gemm's class descriptor of it.
"""
from typing import Dict, Optional

import torch
import torch.nn.functional as F

import ldm_oracle as LO

Tensor = torch.Tensor
DDCONFIG = LO.DDCONFIG
SCALE_FACTOR = LO.SCALE_FACTOR


def block_plan(cfg=DDCONFIG):
    """[(prefix, kind, cin, cout)] in EXECUTION order (model.py:535-568)."""
    ch, mult = cfg["ch"], cfg["ch_mult"]
    nres = len(mult)
    block_in = ch * mult[nres - 1]
    plan = [("decoder.conv_in", "conv3", cfg["z_channels"], block_in),
            ("decoder.mid.block_1", "res", block_in, block_in), ("decoder.mid.attn_1", "attn", block_in, block_in),
            ("decoder.mid.block_2", "res", block_in, block_in)]
    for lvl in reversed(range(nres)):
        block_out = ch * mult[lvl]
        for b in range(cfg["num_res_blocks"] + 1):
            plan.append((f"decoder.up.{lvl}.block.{b}", "res", block_in, block_out))
            block_in = block_out
        if lvl != 0:
            plan.append((f"decoder.up.{lvl}.upsample.conv", "up", block_in, block_in))
    plan += [("decoder.norm_out", "norm", block_in, block_in), ("decoder.conv_out", "conv3", block_in, 3)]
    return plan


def init_params(seed: Optional[int] = None, cfg=DDCONFIG) -> Dict[str, Tensor]:
    """torch default initialisers drawn in the reference Decoder's CONSTRUCTION order (model.py:478-533: conv_in, mid, the
    levels from the last one down, norm_out, conv_out), then post_quant_conv = nn.Conv2d(4, 4, 1) (autoencoder.py:303);
    returned in state_dict order (`up` is prepended: level 0 first)."""
    import torch.nn as nn
    if seed is not None:
        torch.manual_seed(seed)
    drawn: Dict[str, Tensor] = {}

    def add(prefix, m):
        for n, p in m.named_parameters():
            drawn[f"{prefix}.{n}"] = p.detach().clone()

    def res(prefix, cin, cout):
        add(f"{prefix}.norm1", nn.GroupNorm(32, cin, eps=1e-6))
        add(f"{prefix}.conv1", nn.Conv2d(cin, cout, 3, 1, 1))
        add(f"{prefix}.norm2", nn.GroupNorm(32, cout, eps=1e-6))
        add(f"{prefix}.conv2", nn.Conv2d(cout, cout, 3, 1, 1))
        if cin != cout:
            add(f"{prefix}.nin_shortcut", nn.Conv2d(cin, cout, 1, 1, 0))

    ch, mult = cfg["ch"], cfg["ch_mult"]
    nres = len(mult)
    block_in = ch * mult[nres - 1]
    add("decoder.conv_in", nn.Conv2d(cfg["z_channels"], block_in, 3, 1, 1))
    res("decoder.mid.block_1", block_in, block_in)
    add("decoder.mid.attn_1.norm", nn.GroupNorm(32, block_in, eps=1e-6))
    for nm in ("q", "k", "v", "proj_out"):
        add(f"decoder.mid.attn_1.{nm}", nn.Conv2d(block_in, block_in, 1))
    res("decoder.mid.block_2", block_in, block_in)
    for lvl in reversed(range(nres)):
        block_out = ch * mult[lvl]
        for b in range(cfg["num_res_blocks"] + 1):
            res(f"decoder.up.{lvl}.block.{b}", block_in, block_out)
            block_in = block_out
        if lvl != 0:
            add(f"decoder.up.{lvl}.upsample.conv", nn.Conv2d(block_in, block_in, 3, 1, 1))
    add("decoder.norm_out", nn.GroupNorm(32, block_in, eps=1e-6))
    add("decoder.conv_out", nn.Conv2d(block_in, 3, 3, 1, 1))
    add("post_quant_conv", nn.Conv2d(cfg["embed_dim"], cfg["z_channels"], 1))

    def level(k):
        return int(k.split(".")[2]) if k.startswith("decoder.up.") else -1

    keys = list(drawn)
    first_up = next(i for i, k in enumerate(keys) if level(k) >= 0)
    last_up = max(i for i, k in enumerate(keys) if level(k) >= 0)
    ups = sorted(keys[first_up:last_up + 1], key=level)            # stable: construction order inside a level
    return {k: drawn[k] for k in keys[:first_up] + ups + keys[last_up + 1:]}


def decode(p: Dict[str, Tensor], z: Tensor, cfg=DDCONFIG) -> Tensor:
    """latent [N,4,h,w] (scaled by 0.18215) -> frame [N,3,8h,8w] in z's dtype: decode_first_stage."""
    dt = z.dtype
    p = {k: v.to(dt) for k, v in p.items()}
    h = 1. / SCALE_FACTOR * z                           # ddpm.py:713 (torch rounds the scalar to z's dtype)
    h = F.conv2d(h, p["post_quant_conv.weight"], p["post_quant_conv.bias"])
    for prefix, kind, cin, cout in block_plan(cfg):
        if kind == "conv3":
            h = F.conv2d(h, p[f"{prefix}.weight"], p[f"{prefix}.bias"], padding=1)
        elif kind == "up":
            h = F.interpolate(h, scale_factor=2.0, mode="nearest")
            h = F.conv2d(h, p[f"{prefix}.weight"], p[f"{prefix}.bias"], padding=1)
        elif kind == "norm":
            h = LO._swish(LO._gn(p, prefix, h))
        elif kind == "res":
            h = LO._res(p, prefix, h, cin, cout)
        elif kind == "attn":
            h = LO._attn(p, prefix, h)
    return h


def to_u8(x: Tensor):
    """ldm_embedding_interpol.py:179-182: u8 NHWC of a decoded f32 NCHW batch."""
    import numpy as np
    t = torch.clamp((x + 1.0) / 2.0, min=0.0, max=1.0).cpu().numpy()
    return (255. * t.transpose(0, 2, 3, 1)).astype(np.uint8)


# ---- the parity fold of Upsample ------------------------------------------------------------------------------------

# kernel rows (or columns) summed into tap t of parity p: R[p][t]
R = (((0,), (1, 2)), ((0, 1), (2,)))


def fold_upconv(w: Tensor, Kc: Optional[int] = None, defect: Optional[str] = None) -> Tensor:
    """w [Co][Ci][3][3] -> Wf [Co][16][Kc] in w's dtype: slot 4 (2p + q) + 2 th + tw holds the sum over kh in R[p][th]
    (ascending) and inside it kw in R[q][tw] (ascending), accumulated from +0 in that order (rbvae_upconv_fold's order: in
    float32 the results are bit-identical); channels Ci..Kc zero.
    defect "unfolded_w1": the two-row sums keep their first row only (w[1] where w[1] + w[2] belongs)."""
    Co, Ci = w.shape[:2]
    Kc = Ci if Kc is None else Kc
    out = torch.zeros(Co, 16, Kc, dtype=w.dtype)
    for p in range(2):
        for q in range(2):
            for th in range(2):
                for tw in range(2):
                    rows = R[p][th][:1] if defect == "unfolded_w1" else R[p][th]
                    acc = torch.zeros(Co, Ci, dtype=w.dtype)
                    for kh in rows:
                        for kw in R[q][tw]:
                            acc = acc + w[:, :, kh, kw]
                    out[:, 4 * (2 * p + q) + 2 * th + tw, :Ci] = acc
    return out


def upconv_folded(x: Tensor, wf: Tensor, defect: Optional[str] = None) -> Tensor:
    """The four-class form: x [N][Ci][h][w], wf [Co][16][Kc] (Kc >= Ci) -> [N][Co][2h][2w] in x's dtype, no bias:
    out[n][co][2r+p][2c+q] = sum_{th,tw,ci} x[n][ci][r-1+p+th][c-1+q+tw] wf[co][4(2p+q) + 2th+tw][ci], zero outside.
    defects (each must break the bound): "dropped_tap" (tap (1, 1) of every class missing), "swapped_classes" (class
    (p, q) written where (q, p) belongs), "wrong_edge" (rows read from r - p - th + 1: the halo row of the other side)."""
    N, Ci, h, w = x.shape
    Co = wf.shape[0]
    out = torch.zeros(N, Co, 2 * h, 2 * w, dtype=x.dtype)
    xp = F.pad(x, (1, 1, 1, 1))
    for p in range(2):
        for q in range(2):
            acc = torch.zeros(N, Co, h, w, dtype=x.dtype)
            for th in range(2):
                for tw in range(2):
                    if defect == "dropped_tap" and th == 1 and tw == 1:
                        continue
                    dh = p + th                                   # offset into the padded map: r - 1 + p + th + 1
                    if defect == "wrong_edge":
                        dh = 2 - dh
                    win = xp[:, :, dh:dh + h, q + tw:q + tw + w]
                    acc = acc + torch.einsum("nchw,oc->nohw", win, wf[:, 4 * (2 * p + q) + 2 * th + tw, :Ci])
            if defect == "swapped_classes":
                out[:, :, q::2, p::2] = acc
            else:
                out[:, :, p::2, q::2] = acc
    return out


def gather_classes(x: Tensor, wf: Tensor, desc, so: int = 2) -> Tensor:
    """rbvae_gather_gemm's sums for a class descriptor (include/rbvae_hip.h: per class [ntaps, oh0, ow0, ntaps x (widx, dh,
    dw)], sa = 1): out[n][co][a so + oh0][b so + ow0] = sum_taps sum_ci x[n][ci][a + dh][b + dw] wf[co][widx][ci], x zero
    outside its map.  x [N][Ci][h][w], wf [Co][taps_total][Kc >= Ci] -> [N][Co][so h][so w] in x's dtype."""
    N, Ci, h, w = x.shape
    out = torch.zeros(N, wf.shape[0], so * h, so * w, dtype=x.dtype)
    desc, i = list(desc), 0
    while i < len(desc):
        ntaps, oh0, ow0 = desc[i:i + 3]
        acc = torch.zeros(N, wf.shape[0], h, w, dtype=x.dtype)
        for widx, dh, dw in (desc[i + 3 + 3 * j:i + 6 + 3 * j] for j in range(ntaps)):
            pad = max(abs(dh), abs(dw), 1)
            win = F.pad(x, (pad,) * 4)[:, :, pad + dh:pad + dh + h, pad + dw:pad + dw + w]
            acc = acc + torch.einsum("nchw,oc->nohw", win, wf[:, widx, :Ci])
        out[:, :, oh0::so, ow0::so] = acc
        i += 3 + 3 * ntaps
    return out


def upconv_class_desc():
    """rbvae_gather_gemm's descriptor of the four classes: per class [4, p, q, 4 x (slot, p - 1 + th, q - 1 + tw)]."""
    d = []
    for p in range(2):
        for q in range(2):
            d += [4, p, q]
            for th in range(2):
                for tw in range(2):
                    d += [4 * (2 * p + q) + 2 * th + tw, p - 1 + th, q - 1 + tw]
    return d
