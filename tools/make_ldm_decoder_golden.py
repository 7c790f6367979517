#!/usr/bin/env python3
"""Generate tests/golden/ldm_decoder.npz by RUNNING THE REFERENCE on the CPU (needs a checkout of the reference, named by
RBVAE_REFERENCE; nothing of its text is copied: only arrays it computes are recorded).

  - the reference's own Decoder class (src/stable-diffusion/ldm/modules/diffusionmodules/model.py:462-568, random init under
    the seed) followed in construction by nn.Conv2d(4, 4, 1) = post_quant_conv (ldm/models/autoencoder.py:303); decode =
    decoder(post_quant_conv(1. / 0.18215 * z)) (ldm/models/diffusion/ddpm.py:713, autoencoder.py:330-333);
  - slerp / interpolate_embeddings of scripts/pretrained_model_experiments/ldm_embedding_interpol.py:46-72, taken out of
    the script's syntax tree at run time (the script itself imports packages that are not installed).

Recorded: meta/seed, meta/keys (state_dict order), paramsum/<key> = (sum, sum |.|) in float64, z_a [2,4,8,8] -> out_a
[2,3,64,64], z_b [1,4,4,12] -> out_b [1,3,32,96], interp/z0, interp/z1, interp/linear [5,...], interp/spherical [5,...],
interp/same_spherical (identical inputs: the LERP branch)."""
import ast
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("RBVAE_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))     # a checkout beside this one
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def reference_interpolation():
    path = os.path.join(REF, "scripts", "pretrained_model_experiments", "ldm_embedding_interpol.py")
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("slerp", "interpolate_embeddings")]
    assert len(keep) == 2
    ns = {"torch": torch}
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return ns["interpolate_embeddings"]


def main():
    assert os.path.isdir(REF), "needs the reference checkout"
    sys.path.insert(0, os.path.join(REF, "src", "stable-diffusion"))
    import importlib
    mdl = importlib.import_module("ldm.modules.diffusionmodules.model")
    import _ldm_decoder_ref as DR
    seed = 37
    cfg = DR.DDCONFIG
    torch.manual_seed(seed)
    dec = mdl.Decoder(ch=cfg["ch"], out_ch=3, ch_mult=cfg["ch_mult"], num_res_blocks=cfg["num_res_blocks"],
                      attn_resolutions=[], dropout=0.0, in_channels=3, resolution=256, z_channels=4)
    pq = nn.Conv2d(4, 4, 1)
    sd = {f"decoder.{k}": v for k, v in dec.state_dict().items()}
    sd.update({f"post_quant_conv.{k}": v for k, v in pq.state_dict().items()})
    mine = DR.init_params(seed)
    assert list(sd.keys()) == list(mine.keys()), "construction order drifted"
    for k in sd:
        assert torch.equal(sd[k], mine[k]), k
    dec.eval()
    g = torch.Generator().manual_seed(seed + 1)
    out = {"meta/seed": seed, "meta/keys": np.array(list(sd.keys()))}
    for tag, shape in (("a", (2, 4, 8, 8)), ("b", (1, 4, 4, 12))):
        z = torch.randn(shape, generator=g) * 0.18215 * 4.0          # the scale of encoded frames' latents
        with torch.no_grad():
            x = dec(pq(1. / 0.18215 * z))
        out[f"z_{tag}"], out[f"out_{tag}"] = z.numpy(), x.numpy()
        print(f"case {tag}: {tuple(z.shape)} -> {tuple(x.shape)}, |out| max {float(x.abs().max()):.3f}")
    for k, v in sd.items():
        out[f"paramsum/{k}"] = np.array([float(v.double().sum()), float(v.double().abs().sum())])
    interp = reference_interpolation()
    z0, z1 = torch.randn((4, 8, 8), generator=g), torch.randn((4, 8, 8), generator=g)
    out["interp/z0"], out["interp/z1"] = z0.numpy(), z1.numpy()
    out["interp/linear"] = torch.stack(interp(z0, z1, steps=5, method="linear")).numpy()
    out["interp/spherical"] = torch.stack(interp(z0, z1, steps=5, method="spherical")).numpy()
    out["interp/same_spherical"] = torch.stack(interp(z0, z0.clone(), steps=5, method="spherical")).numpy()
    path = os.path.join(OUT, "ldm_decoder.npz")
    np.savez_compressed(path, **out)
    print(f"ldm_decoder: {len(sd)} tensors bit-identical to the reference Decoder; {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
