"""Robustness and code-distance evaluation on raw frames (the reference's headline evaluation):
  calculate_state_consistency(perturbation=...)   scripts/evaluation/state_consistency_eval/embedding_matching.py:
                                                   141-193 (add_gaussian_noise, add_occlusion), 209-299, 380-470
  find_most_common_vector + adjacent Hamming       scripts/evaluation/clustering_eval/embedding_hamming_distance.py:
                                                   53-87, 170-240
The reference prepares, encodes and votes one frame at a time on the host.  Here the frames are u8 on the device and
every stage is batched: perturbation and resizes (frames.py, csrc/frames.hip), the LDM encode (ldm.py), the RBVAE
encode (model.py) and the vote (csrc/eval.hip).  With the same noise draws (u, eps, noise, boxes; reference_draws()
replays a torch.manual_seed run) the codes are the reference's bit for bit.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from .data import assign_label, consistency_from_codes
from .frames import occlusion_boxes, perturb_u8, resize_u8, sd_input, sd_target, u8_to_input

PERTURBATIONS = ("gaussian_noise", "occlusion")


def _slice(t, s, e):
    return None if t is None else t[s:e]


def _check_draw(name, t, shape):
    if t is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")


@torch.no_grad()
def state_codes_under(model, frames: torch.Tensor, frame_indices: Sequence[int], flags: Sequence[int],
                      perturbation: Optional[str] = None, params: Optional[dict] = None, ldm_encoder=None,
                      temperature: float = 0.2, noise_ratio: float = 0.1, batch: int = 64, u=None, noise=None,
                      boxes=None, eps=None, target=(1280, 720), resolution: int = 256, generator=None):
    """The encode loop of calculate_state_consistency (embedding_matching.py:209-267) over u8 frames [F,H,W,3] (the
    source frames of `frame_indices`, on the device), `batch` frames per step.  Stage order is the reference's:
      perceptual (ldm_encoder given): perturb at source size -> sd_input(target) -> LDM encode -> model.encode
      contrastive:                    Resize((resolution,)*2) -> perturb at that size -> ToTensor -> model.encode
    so the occlusion square is sized from the source frame in one path and from resolution^2 in the other.
    perturbation: None, "gaussian_noise" (params std, mean) or "occlusion" (params coverage).
    Draws (default as in perturb_u8 / LDMEncoder.encode / Seq2SeqBinaryVAE.encode): u [F,L] binarisation uniforms,
    noise [F,3,h,w] at the perturbed size, boxes [F,3] (x, y, size), eps [F,4,h/8,w/8] posterior draws.
    -> (codes f32 [F,L] on the device, labels int64 [F])."""
    if perturbation is not None and perturbation not in PERTURBATIONS:
        raise ValueError(f"perturbation must be None or one of {PERTURBATIONS}, got {perturbation!r}")
    params = dict(params or {})
    F = frames.shape[0] if isinstance(frames, torch.Tensor) else 0
    if F == 0 or len(frame_indices) != F:
        raise ValueError(f"need one frame index per frame: {len(frame_indices)} indices, {F} frames")
    perceptual = ldm_encoder is not None
    H, W = frames.shape[1], frames.shape[2]
    if perceptual:
        ph, pw = H, W
        sw, sh = sd_target(target)
        Z = ldm_encoder.cfg["embed_dim"]
        _check_draw("eps", eps, (F, Z, sh // 8, sw // 8))
    else:
        ph = pw = int(resolution)
    Ld = model.latent_dim
    _check_draw("u", u, (F, Ld))
    if perturbation == "gaussian_noise":
        _check_draw("noise", noise, (F, 3, ph, pw))
    if perturbation == "occlusion":
        if boxes is None:
            boxes = occlusion_boxes(F, (ph, pw), params.get("coverage", 0.2))
        boxes = torch.as_tensor(np.asarray(boxes.cpu() if isinstance(boxes, torch.Tensor) else boxes),
                                dtype=torch.int32)
        _check_draw("boxes", boxes, (F, 3))
    if u is None:
        u = torch.rand((F, Ld))                                  # host draws, like the reference's encode (:33)
    labels = np.array([assign_label(int(i), flags) for i in frame_indices], dtype=np.int64)
    codes = torch.empty((F, Ld), dtype=torch.float32, device=frames.device)
    batch = max(1, int(batch))
    for s in range(0, F, batch):
        e = min(F, s + batch)
        x = frames[s:e]
        if not perceptual:
            x = resize_u8(x, (pw, ph), "bilinear")
        if perturbation == "gaussian_noise":
            x = perturb_u8(x, "gaussian_noise", std=params.get("std", 0.1), mean=params.get("mean", 0.0),
                           noise=_slice(noise, s, e), generator=generator)
        elif perturbation == "occlusion":
            x = perturb_u8(x, "occlusion", boxes=boxes[s:e])
        if perceptual:
            ep = None if eps is None else eps[s:e].to(frames.device)
            lat = ldm_encoder.encode(sd_input(x, target), eps=ep)
            inp = lat[:, None]
        else:
            inp = u8_to_input(x, "totensor")[:, None]
        z = model.encode(inp, temperature=temperature, hard=True, noise_ratio=noise_ratio,
                         u=u[s:e].to(frames.device))
        codes[s:e] = z[:, 0]
    return codes, labels


def state_consistency_under(model, frames, frame_indices, flags, perturbation=None, params=None, **kw):
    """calculate_state_consistency (embedding_matching.py:209-299): state_codes_under + the device vote
    (consistency_from_codes).  -> (weighted_avg, percentages), the reference's semantics (ties of the vote go to the
    lexicographically smallest code, as np.unique)."""
    codes, labels = state_codes_under(model, frames, frame_indices, flags, perturbation, params, **kw)
    return consistency_from_codes(codes, labels, len(flags) + 1)


def most_common_codes(codes: torch.Tensor, labels, n_states: int, tie: str = "lexicographic"):
    """Per state, the most common code of its frames, from the 128-bit keys and per-frame counts of rbvae_state_vote.
      tie="lexicographic": np.unique + argmax (the consistency metric, embedding_matching.py:279-282);
      tie="first":         Counter.most_common(1), the code seen first among the tied
                           (embedding_hamming_distance.py:78-87).
    -> (winners int64 [n_states, L] numpy, counts [n_states]); a state without frames gets zeros and count 0 (the
    Hamming script's placeholder, :204-212)."""
    if tie not in ("lexicographic", "first"):
        raise ValueError(f"tie must be 'lexicographic' or 'first', got {tie!r}")
    codes = torch.as_tensor(codes)
    if codes.dim() != 2 or codes.shape[1] < 1 or codes.shape[1] > 128:
        raise ValueError(f"codes must be [F, L] with 1 <= L <= 128, got {tuple(codes.shape)}")
    F, Ld = codes.shape
    winners = np.zeros((n_states, Ld), dtype=np.int64)
    wcount = np.zeros(n_states, dtype=np.int64)
    if F == 0:
        return winners, wcount
    dev = codes.device if codes.is_cuda else torch.device("cuda")
    c = codes.to(dev).float().contiguous()
    lab = torch.as_tensor(np.asarray(labels), dtype=torch.int32).to(dev)
    keys = torch.empty(F, 4, dtype=torch.int32, device=dev)
    cnt = torch.empty(F, dtype=torch.int32, device=dev)
    out = torch.empty(n_states, 2, dtype=torch.int32, device=dev)
    L.call("rbvae_state_vote", c, lab, F, Ld, n_states, keys, cnt, out)
    k = keys.cpu().numpy().view(np.uint32).astype(np.uint64)
    n = cnt.cpu().numpy()
    lb = lab.cpu().numpy()
    for s in range(n_states):
        rows = np.nonzero(lb == s)[0]
        if rows.size == 0:
            continue
        best = n[rows].max()
        cand = rows[n[rows] == best]
        if tie == "first":
            f = int(cand[0])
        else:                                   # smallest key = np.unique's first row among the tied
            f = int(min(cand, key=lambda i: tuple(k[i])))
        winners[s] = (codes[f].detach().cpu().numpy() > 0.5).astype(np.int64)
        wcount[s] = int(best)
    return winners, wcount


def adjacent_hamming(winners):
    """Hamming distances between the winning codes of adjacent states and their mean
    (embedding_hamming_distance.py:53-57, 214-232).  -> (distances int64 [S-1], mean)."""
    w = np.asarray(winners)
    if w.ndim != 2 or w.shape[0] < 2:
        raise ValueError(f"need [S >= 2, L] winning codes, got {w.shape}")
    d = np.sum(w[1:] != w[:-1], axis=1).astype(np.int64)
    return d, float(np.mean(d))


def reference_draws(n_frames: int, latent_dim: int, noise_hw=None, latent_hw=None, latent_channels: int = 4):
    """The reference's random draws of one calculate_state_consistency run, from the global CPU generator (seed it
    with torch.manual_seed) in its per-frame order: the perturbation's randn_like [1,3,H,W] (noise_hw = (H, W) when
    the perturbation is gaussian noise; embedding_matching.py:141-158), the LDM posterior's randn [1,4,h,w] (latent_hw
    = (h, w) for a perceptual model; distributions.py:35-37), the binarisation's rand [1,L] (percep_RBVAE_model.py:33).
    -> dict(noise [F,3,H,W] or None, eps [F,4,h,w] or None, u [F,L]) for state_codes_under."""
    noise, eps, u = [], [], []
    for _ in range(int(n_frames)):
        if noise_hw is not None:
            noise.append(torch.randn((1, 3, int(noise_hw[0]), int(noise_hw[1]))))
        if latent_hw is not None:
            eps.append(torch.randn((1, int(latent_channels), int(latent_hw[0]), int(latent_hw[1]))))
        u.append(torch.rand((1, int(latent_dim))))
    return {"noise": torch.cat(noise) if noise else None, "eps": torch.cat(eps) if eps else None,
            "u": torch.cat(u) if u else torch.zeros(0, int(latent_dim))}
