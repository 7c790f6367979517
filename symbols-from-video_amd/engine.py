"""Hand-scheduled forward/backward of the RBVAE path over librbvae_hip.

The engine owns no parameters: it is given the model's flat f32 parameter buffer
(the reference's registration order, see `ParamLayout`) and writes gradients into a
flat buffer of the same layout.  Activations are NHWC in the engine's storage dtype
("f32" parity mode / "bf16" performance mode); LSTM, binarise and the losses are f32.

Reference path restated by the kernels this file sequences:
  Seq2SeqBinaryVAE.forward / encode   models/percep_RBVAE/percep_RBVAE_model.py:143-191
  (contrastive / triplet / simple variants: the matching *_model.py files)
"""
from __future__ import annotations

import contextlib
import ctypes
import math
from collections import namedtuple
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib as L
from .jobs import JOB_CONV_PACK, JOB_PACK, JOB_PERMUTE, JOB_ROWS, Col, JobList, JobTable, adam_context
from .jobs import job_block_map          # re-exported: tests and tools call engine.job_block_map

F32, BF16 = 0, 1


@dataclass(frozen=True)
class Variant:
    name: str
    channels: Tuple[int, int, int]
    kernel: int
    lstm_layers: int
    dropout: float
    noise_ratio_arg: bool
    eps: float
    simple_order: bool          # conv -> binarise -> rnn -> rnn -> deconv, ReLU after conv3
    default_hw: Tuple[int, int]


VARIANTS = {
    # models/percep_RBVAE/percep_RBVAE_model.py:46-141
    "percep": Variant("percep", (256, 256, 256), 3, 4, 0.2, True, 1e-8, False, (88, 160)),
    # models/contrastive_RBVAE/contrastive_RBVAE_model.py:45-140
    "contrastive": Variant("contrastive", (64, 64, 64), 3, 2, 0.2, True, 1e-8, False, (256, 256)),
    # models/triplet_RBVAE/triplet_RBVAE_model.py:18-45,144-171 (noise is never scaled)
    "triplet": Variant("triplet", (64, 64, 64), 3, 2, 0.2, False, 1e-8, False, (256, 256)),
    # models/simple_RBVAE/simple_RBVAE_model.py:77-193
    "simple": Variant("simple", (64, 128, 256), 4, 1, 0.0, False, 1e-10, True, (64, 64)),
}


def conv_out(n: int, k: int) -> int:
    return (n + 2 - k) // 2 + 1


def _ru(x: int, m: int) -> int:
    return (x + m - 1) // m * m


class ParamLayout:
    """Names, shapes and flat offsets of the parameters in the reference's
    registration order (state_dict order of Seq2SeqBinaryVAE)."""

    def __init__(self, v: Variant, in_ch: int, out_ch: int, latent: int, hw: Tuple[int, int]):
        c1, c2, c3 = v.channels
        k = v.kernel
        h, w = hw
        for _ in range(3):
            h, w = conv_out(h, k), conv_out(w, k)
        self.bott = (h, w)
        flat = c3 * h * w
        idx = (0, 2, 4) if v.name == "simple" else (0, 3, 6)
        shapes: List[Tuple[str, Tuple[int, ...]]] = []
        for i, (ci, co) in zip(idx, [(in_ch, c1), (c1, c2), (c2, c3)]):
            shapes += [(f"encoder_cnn.conv.{i}.weight", (co, ci, k, k)), (f"encoder_cnn.conv.{i}.bias", (co,))]
        shapes += [("encoder_cnn.fc.weight", (latent, flat)), ("encoder_cnn.fc.bias", (latent,)),
                   ("decoder_cnn.fc.weight", (flat, latent)), ("decoder_cnn.fc.bias", (flat,))]
        for i, (ci, co) in zip(idx, [(c3, c2), (c2, c1), (c1, out_ch)]):
            shapes += [(f"decoder_cnn.deconv.{i}.weight", (ci, co, k, k)), (f"decoder_cnn.deconv.{i}.bias", (co,))]
        for stack in ("encoder_rnn", "decoder_rnn"):
            for l in range(v.lstm_layers):
                shapes += [(f"{stack}.lstm.weight_ih_l{l}", (4 * latent, latent)),
                           (f"{stack}.lstm.weight_hh_l{l}", (4 * latent, latent)),
                           (f"{stack}.lstm.bias_ih_l{l}", (4 * latent,)),
                           (f"{stack}.lstm.bias_hh_l{l}", (4 * latent,))]
        self.names = [n for n, _ in shapes]
        self.shapes = dict(shapes)
        self.offsets: Dict[str, int] = {}
        off = 0
        for n, s in shapes:
            # keep every tensor 16-byte aligned inside the flat buffer
            off = _ru(off, 4)
            self.offsets[n] = off
            off += math.prod(s)
        self.total = _ru(off, 4)
        self.conv_idx = idx
        # the LSTM blocks must be gap-free (the kernel walks w_ih, w_hh, b_ih, b_hh per layer)
        for stack in ("encoder_rnn", "decoder_rnn"):
            base = self.offsets[f"{stack}.lstm.weight_ih_l0"]
            per = 8 * latent * latent + 8 * latent
            for l in range(v.lstm_layers):
                assert self.offsets[f"{stack}.lstm.weight_ih_l{l}"] == base + l * per, "lstm block not contiguous"

    def view(self, flat: torch.Tensor, name: str) -> torch.Tensor:
        o = self.offsets[name]
        s = self.shapes[name]
        return flat[o:o + math.prod(s)].view(s)


def conv_classes(k: int) -> List[int]:
    """gather_gemm descriptor of Conv2d(k, stride 2, pad 1): one class, k*k taps."""
    d = [k * k, 0, 0]
    for kh in range(k):
        for kw in range(k):
            d += [kh * k + kw, kh - 1, kw - 1]
    return d


def dgrad_classes(k: int) -> Tuple[List[int], int]:
    """Descriptor of the conv's input gradient (= ConvTranspose2d(k,2,1) forward): four
    output-parity classes, heaviest first so the long workgroups start early."""
    per = []
    for ch in (0, 1):
        for cw in (0, 1):
            taps = []
            for kh in range(k):
                if (ch + 1 - kh) % 2:
                    continue
                for kw in range(k):
                    if (cw + 1 - kw) % 2:
                        continue
                    taps += [kh * k + kw, (ch + 1 - kh) // 2, (cw + 1 - kw) // 2]
            per.append((len(taps) // 3, ch, cw, taps))
    per.sort(key=lambda t: -t[0])
    d: List[int] = []
    for n, ch, cw, taps in per:
        d += [n, ch, cw] + taps
    return d, len(per)


ONE_TAP = [1, 0, 0, 0, 0, 0]

Names = namedtuple("Names", "weight bias")      # parameter names of a layer that has no Stride2 record (conv1, last deconv)
# A k x k stride-2 layer as the GEMMs see it: a small grid with `cs` channels and a big grid (twice the extent) with `cb`
# channels.  An encoder Conv2d (big -> small) and a decoder ConvTranspose2d (small -> big) are the same layer: the parameter
# `weight` is [cs][cb][k][k] in both, the forward of one is the input gradient of the other.  f = its packed copy
# [cs][t][cb] (big -> small launches read it), d = [cb][t][cs] (small -> big); big / small = the two grids (h, w)
Stride2 = namedtuple("Stride2", "weight bias f d cs cb big small")


class Saved:
    """Activations one forward call keeps for its backward."""
    __slots__ = ("N", "S", "T", "hw", "train", "tau", "tau_dev", "hard", "col1", "x_in", "fm_in", "a1", "a2", "a3", "e", "hs_enc", "hp_enc",
                 "acts_enc", "cs_enc", "y", "z", "hs_dec", "hp_dec", "acts_dec", "cs_dec", "ds_pad", "f", "d1", "d2",
                 "xr", "gate_scale", "dpre3", "b3_parts", "dd2_fused")


class _Pass:
    """What the stages of one forward() / backward() call share: the frame counts, the row counts of the three grids, views
    into the flat buffers and the persistent temporaries of this frame count.  A stage hangs what later stages read on it."""

    def __init__(self, eng: "Engine", sv: Saved, flat: torch.Tensor, gflat: Optional[torch.Tensor] = None):
        self.eng, self.sv, self.flat, self.gflat = eng, sv, flat, gflat
        self.N, self.S, self.T = sv.N, sv.S, sv.T
        self.H, self.W = sv.hw
        self.P1, self.P2, self.P3 = (sv.N * h * w for h, w in (eng.g1, eng.g2, eng.g3))
        self.P = lambda name: eng.layout.view(flat, name)         # a parameter / its gradient by name
        self.G = lambda name: eng.layout.view(gflat, name)

    def tmp(self, tag, *shape, dtype=None):
        return self.eng._buf((self.N, tag), math.prod(shape), dtype or self.eng.tdt).view(*shape)

    def fm(self, ch):       # the caller's frame_map, or the dense one of frames with `ch` channels
        return self.frame_map if self.frame_map is not None else (0, 0, 0, 0, ch * self.H * self.W)


class Engine:
    def __init__(self, variant: str, in_ch: int, out_ch: int, latent: int, hw: Tuple[int, int],
                 dtype: str = "f32", device: Optional[torch.device] = None):
        if variant not in VARIANTS:
            raise ValueError(f"unknown variant {variant!r}")
        if dtype not in ("f32", "bf16"):
            raise ValueError("dtype must be 'f32' or 'bf16'")
        self.v = VARIANTS[variant]
        self.in_ch, self.out_ch, self.latent = in_ch, out_ch, latent
        self.hw = tuple(hw)
        if self.hw[0] % 8 or self.hw[1] % 8:
            raise ValueError(f"frame size {self.hw} must be divisible by 8 (three stride-2 stages)")
        if latent > 128:
            raise ValueError("latent_dim > 128 is not supported by the LSTM kernel")
        self.dt = F32 if dtype == "f32" else BF16
        self.tdt = torch.float32 if dtype == "f32" else torch.bfloat16
        self.es = 4 if dtype == "f32" else 2
        self.ke = 128 // self.es
        self.layout = ParamLayout(self.v, in_ch, out_ch, latent, self.hw)
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        k = self.v.kernel
        self.k, self.kk = k, k * k
        H, W = self.hw
        self.g1 = (conv_out(H, k), conv_out(W, k))
        self.g2 = (conv_out(self.g1[0], k), conv_out(self.g1[1], k))
        self.g3 = (conv_out(self.g2[0], k), conv_out(self.g2[1], k))
        c1, c2, c3 = self.v.channels
        self.F3 = c3 * self.g3[0] * self.g3[1]
        self.K1 = _ru(k * k * in_ch, self.ke)          # im2col width of the first conv
        self.K3 = _ru(k * k * out_ch, self.ke)         # im2col width of d(loss)/d(pre) for the last deconv
        self.NY = _ru(k * k * out_ch, 8)               # per-tap product width of the last deconv
        self.Lp = _ru(latent, self.ke)
        self.zero = torch.zeros(256, dtype=torch.uint8, device=self.device)
        carr = lambda ints: (ctypes.c_int * len(ints))(*ints)
        dg, ncls_dg = dgrad_classes(k)
        # gather_gemm class descriptors by _gemm's cls_key: (C int array, number of classes)
        self._descs = {"one": (carr(ONE_TAP), 1), "conv": (carr(conv_classes(k)), 1), "dgrad": (carr(dg), ncls_dg)}
        self._idx_cache: Dict[Tuple, torch.Tensor] = {}
        self.seed_dev = None           # optional device step counter (int64 tensor) for graph-replayed steps
        self._pack_tab: Dict = {}      # uploaded JobTables of pack() (keyed by the flat buffer) and update_jobs() (by its arguments)
        self._bufs: Dict = {}          # persistent backward temporaries, keyed by (N, tag)
        self._bwd_tab: Dict = {}       # uploaded reduce-job JobTables, keyed by their signature
        self._tables: Dict[int, JobTable] = {}     # every uploaded JobTable by the address of its device rows (which it holds)
        self._jobs: Optional[JobList] = None
        self.last_wgrad_kernel = None  # kernel family the last _wgrad() call launched (bench.py's roofline leg keys its timers by it)
        self._job_blocks = 256      # workgroups per job of a batched job launch (at most)
        # the engine's uploaded job tables are launched with exactly the workgroups they can use ...
        self.table_launch = True    # ... through rbvae_run_jobs_table (LDS from the rows); False: rbvae_run_jobs_sized
        # ... their heaviest jobs' workgroups first (rbvae_job_launch_order): 0 none, 1 the update table, 2 all.  The reduce
        # launches keep the map's order: heaviest first gives them nothing at the bench shape and costs the native step 12 us
        # ("Update launch")
        self.jobs_heavy_first = 1
        self._side: Optional[torch.cuda.Stream] = None
        # Side stream (graph capture turns the fork / join into graph edges; `overlap = False`: everything in issue order on
        # one stream -- bench.py's `isolated` leg).  What rides it was settled by same-GPU sweeps in rounds 1-2 (ms/step):
        # pair term + decoder weight gradients + their reductions 0.547; also the loss bookkeeping / the LSTM weight
        # gradients as forks of their own / the final reductions 0.553-0.568; nothing 0.591.  Full-chip side kernels beside
        # full-chip main kernels only contend.  Program order at a fork: the main stream's continuation is issued BEFORE the
        # side work (graph capture hands the forking node's queue to the branch created first; created second, the main
        # chain paid a cross-queue hand-off of ~10 us at every fork).
        self.overlap = True
        # dedicated kernel for the K = 64 fc products (bench.py's roofline leg reads this to label the fc launches)
        self.fc_gemm = True
        # halo-resident kernel for the transposed 3x3 / stride-2 launches (csrc/deconv_halo.hip) from this many workgroups up
        self.deconv_halo = True
        self._dh_min_wgs = 1024
        # halo-resident kernel for the 3x3 stride-2 forward-type launches (csrc/conv_s2.hip) from this many workgroups up, when
        # its 8 x 16-pixel tiles cover at most this many times the image's pixels (measured, tools/time_conv_s2.py: 128 images
        # 88 x 160 -> 44 x 80, 256 channels: 662 vs 844 us for the gather GEMM; the native 44 x 80 -> 22 x 40 layer, whose 22 x 40
        # map the tiles cover 1.31 times: 229 vs 174 us, so it stays on the gather GEMM)
        self.conv_s2_halo = True
        self._cs_min_wgs = 512
        self._cs_max_waste = 1.15
        # nine-taps-per-workgroup weight gradient of the 3x3 stride-2 layers (csrc/wgrad_halo.hip) when every workgroup
        # gets at least this many 4 x 8 pixel blocks
        self.wgrad_halo = True
        self._wh_min_steps = 8
        self._wh_max_tiles = 2
        # three-taps-per-workgroup weight gradient of the wide (multiples of 128 channels) 3x3 stride-2 layers
        # (csrc/wgrad_row.hip): K-slices of at least _wr_min_steps 64-pixel blocks, at most _wr_slab_mb MB of f32 slabs
        self.wgrad_row = True
        self._wr_min_steps = 4
        self._wr_slab_mb = 64
        # K-slices ~ sqrt(coef * blocks): a K-slice more costs its f32 slab (2.4 MB written, read again by the reduction job:
        # ~1.2 us of memory time at 256 x 256 channels), a K-slice less lengthens every workgroup's loop by blocks / ks^2 steps
        # of ~1.1 us.  Bench shape (256 blocks), same box, ms per step: 7 slices 0.4447, 10 0.4392, 14 0.4549, 21 0.4689
        # (rbvae_wgrad_gemm: 0.4451); native 4 x 88 x 160 (1 760 blocks) wants every CU: 21 slices 2.00 (gemm 2.14)
        self._wr_ks_coef = 0.4
        self._wr_min_blocks = 128      # fewer 64-pixel blocks than this (the bench shape's 4 x 4 layers: 64): rbvae_wgrad_gemm
        # weight gradients of the two 3/4-channel ends from the image itself instead of from im2col rows in HBM
        # (rbvae_wgrad_first, csrc/conv_first.hip) when every workgroup gets at least this many 8 x 16 pixel blocks
        self.wgrad_first = True
        self._wf_min_steps = 8
        # The fc products on either side of the LSTM stacks (M = frames, 32 outputs, K = thousands) run K-split over
        # several workgroup groups, and the LSTM kernels sum the slabs while staging their input (one group: 32 CUs busy at
        # 256 frames).  Needs the wavefront LSTM kernels (latent <= 32).  16 groups for the large fc layers (at F3 = 56 320 /
        # 65 536 four groups were 64 workgroups streaming 21-42 MB: 31-36 us per launch at 0.6 TB/s), else the largest of
        # 16 / 8 / 4 that divides F3 into whole K units
        ks_unit = 32 if dtype == "bf16" else 16
        # ... and write the bf16 / padded copy of their output that the next GEMM reads (rbvae_cast_pad otherwise), run the
        # binarisation inside their launch and, where a pass runs both stacks, go as one launch (each if the call's T fits)
        self.wave_ok = latent <= 32 and self.v.lstm_layers * _ru(4 * latent, 64) <= 1024 and not self.v.simple_order
        self.fc_split = 1
        if self.wave_ok and self.F3 >= 2048:
            for want in ((16, 8, 4) if self.F3 >= 16384 else (4,)):
                if self.F3 % (want * ks_unit) == 0:
                    self.fc_split = want
                    break
        # last deconv forward + loss + input gradient as one launch (csrc/deconv_last_bwd.hip) where forward() is told that
        # backward() will take dpre3 from it; off: rbvae_deconv_last_fused, then rbvae_deconv_last_dgrad_fused in backward()
        self.deconv_last_bwd_fused = True
        self._alloc_packed()

    # ---- packed weights -------------------------------------------------------
    def _alloc_packed(self):
        c1, c2, c3 = self.v.channels
        kk = self.k * self.k
        z = lambda *s: torch.zeros(*s, dtype=self.tdt, device=self.device)
        self.W1p = z(c1, self.K1)                      # conv1 as a 1-tap GEMM over im2col columns
        self.W2f, self.W2d = z(c2, kk, c1), z(c1, kk, c2)
        self.W3f, self.W3d = z(c3, kk, c2), z(c2, kk, c3)
        self.Wfc = z(self.latent, self.F3)             # [L][NHWC-flat]
        self.WfcT = z(self.F3, self.Lp)                # [NHWC-flat][Lp]
        self.Wdfc = z(self.F3, self.Lp)                # [NHWC-flat][Lp]
        self.WdfcT = z(self.latent, self.F3)
        self.bdfc = torch.zeros(self.F3, dtype=torch.float32, device=self.device)   # NHWC order
        self.V1f, self.V1d = z(c3, kk, c2), z(c2, kk, c3)   # deconv0: c3 -> c2
        self.V2f, self.V2d = z(c2, kk, c1), z(c1, kk, c2)   # deconv1: c2 -> c1
        self.V3p = z(self.NY, c1)                      # [(t,co)][c1]: per-tap products of the last deconv
        self.V3f = z(c1, self.K3)                      # [c1][(t,co) padded]
        nl, Ld = self.v.lstm_layers, self.latent
        self.wT_enc = torch.zeros(nl, 2, Ld, 4 * Ld, dtype=torch.float32, device=self.device)   # [k][gate row]
        self.wT_dec = torch.zeros(nl, 2, Ld, 4 * Ld, dtype=torch.float32, device=self.device)
        # the layer records: geometry and operands written once, read by every launch of the layer (_down, _up, _wgrad_s2)
        i0, i1, i2 = self.layout.conv_idx
        nm = lambda stem, i: Names(f"{stem}.{i}.weight", f"{stem}.{i}.bias")
        self.conv1, self.deconv2 = nm("encoder_cnn.conv", i0), nm("decoder_cnn.deconv", i2)
        self.conv2 = Stride2(*nm("encoder_cnn.conv", i1), self.W2f, self.W2d, c2, c1, self.g1, self.g2)
        self.conv3 = Stride2(*nm("encoder_cnn.conv", i2), self.W3f, self.W3d, c3, c2, self.g2, self.g3)
        self.deconv0 = Stride2(*nm("decoder_cnn.deconv", i0), self.V1f, self.V1d, c3, c2, self.g2, self.g3)
        self.deconv1 = Stride2(*nm("decoder_cnn.deconv", i1), self.V2f, self.V2d, c2, c1, self.g1, self.g2)
        self.stride2 = (self.conv2, self.conv3, self.deconv0, self.deconv1)

    def _upload(self, jl: JobList) -> JobTable:
        t = JobTable(jl, self.device, self._job_blocks)
        self._tables[t.rows.data_ptr()] = t
        return t

    def table_of(self, tab: torch.Tensor) -> Optional[JobTable]:
        """The uploaded table whose device rows are `tab` (what pack, update_jobs and the backward pass hand out)."""
        return self._tables.get(tab.data_ptr())

    def run_table(self, tab: torch.Tensor, n: int, kind: int = 2):
        """One batched job launch of `tab` (n rows): sized (exactly the workgroups it can use, and through
        rbvae_run_jobs_table the LDS its rows need and the heaviest jobs first) when it is one of the engine's uploaded
        tables; jobs_heavy_first is asked per kind (1 = the optimiser update table, 2 = the pack / reduce tables)."""
        t = self._tables.get(tab.data_ptr())
        if t is None:
            L.call("rbvae_run_jobs", tab, n, self._job_blocks)
        elif self.table_launch:
            t.run(self.jobs_heavy_first >= kind)
        else:
            L.call("rbvae_run_jobs_sized", tab, *t.block_map)

    def pack(self, flat: torch.Tensor):
        """f32 parameters (reference layouts) -> the packed T copies the GEMMs read (one launch)."""
        key = flat.data_ptr()
        t = self._pack_tab.get(key)
        if t is None:
            t = self._pack_tab[key] = self._upload(self._pack_jobs(flat))
        self.run_table(t.rows, t.n)

    def update_jobs(self, flat, gflat, m, v, hyper, betas, eps, gscale, extra_rows=None, part=None):
        """Optimiser step + weight repack of a training step as ONE batched job launch: every parameter tensor is a job
        that applies torch.optim.Adam to its slice of the flat buffers (the arithmetic of rbvae_adam_step) and writes
        the tensor's packed copies from the new values while it holds them -- kind 3 (conv weights: the block updates
        the rows it packs), kind 6 (generic scatter to one or two copies), kind 7 (no packed copy: biases).
        part: None = every parameter; "tail" / "head" = the data-parallel trainer's gradient buckets (decoder CNN + both
        LSTM stacks / encoder CNN, cut at decoder_cnn.fc.weight): the tail is updated while the head is still being
        all-reduced.  Returns (device table, n_jobs); cached per buffer set."""
        key = ("update", flat.data_ptr(), gflat.data_ptr(), m.data_ptr(), v.data_ptr(), hyper.data_ptr(), tuple(betas),
               float(eps), float(gscale), tuple(map(tuple, extra_rows)) if extra_rows else None, part)
        tab = self._pack_tab.get(key)
        if tab is not None:
            return tab.rows, tab.n
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("update job table missing during graph capture: run one eager update with the same buffers, "
                               f"hyper-parameters and part ({part!r}) first (FusedTrainer's warm-up steps do)")
        ctx = adam_context(flat, gflat, m, v, hyper, betas, eps, gscale)
        packs_jl = self._pack_jobs(flat)
        by_src: Dict[int, List[List[int]]] = {}
        for row in packs_jl.rows:
            by_src.setdefault(row[Col.SRC], []).append(row)
        lay = self.layout
        jl = JobList()
        jl.rows = [list(r) for r in extra_rows] if extra_rows else []
        jl.keep = [packs_jl.keep]
        o_cut = lay.offsets["decoder_cnn.fc.weight"]
        for name in lay.names:
            src = lay.view(flat, name)
            packs = by_src.pop(src.data_ptr(), [])
            if part is not None and (lay.offsets[name] >= o_cut) != (part == "tail"):
                continue
            kinds = [p_[Col.KIND] for p_ in packs]
            if kinds == [JOB_CONV_PACK]:
                jl.add_conv_pack_adam(packs[0], ctx)
            elif kinds in ([JOB_PACK], [JOB_PACK, JOB_PACK]):
                jl.add_adam_pack(ctx, *packs, what=name)
            elif not packs:
                jl.add_adam(src, ctx)
            else:
                raise RuntimeError(f"{name}: unsupported pack job combination for the fused update")
        if by_src:
            raise RuntimeError("pack jobs whose source is not a parameter tensor")
        tab = self._pack_tab[key] = self._upload(jl)
        return tab.rows, tab.n

    def _pack_jobs(self, flat: torch.Tensor) -> JobList:
        lay, dt = self.layout, self.dt
        c1, c2, c3 = self.v.channels
        kk = self.kk
        g3 = self.g3[0] * self.g3[1]
        P = lambda name: lay.view(flat, name)
        jl = JobList()
        pk = lambda src, dst, dims, strides, d=None: jl.add(JOB_PACK, src, dst, dims, strides, dtype=dt if d is None else d)
        # conv1 [c1][cin][kk] -> [c1][t*cin + ci]
        pk(P(self.conv1.weight), self.W1p, (c1, self.in_ch, kk), (self.K1, 1, self.in_ch))
        for ly in self.stride2:                                       # [cs][cb][kk] -> [cs][t][cb] and [cb][t][cs]
            jl.add_conv_pack(P(ly.weight), ly.f, ly.d, ly.cs, ly.cb, kk, dt)
        v3 = P(self.deconv2.weight)                                   # [c1][out][kk]
        pk(v3, self.V3p, (c1, self.out_ch, kk), (1, c1, self.out_ch * c1))       # [(t*out+co)][c1]
        pk(v3, self.V3f, (c1, self.out_ch, kk), (self.K3, 1, self.out_ch))       # [c1][t*out+co]
        wfc = P("encoder_cnn.fc.weight")                              # [L][c3][g3]
        pk(wfc, self.Wfc, (self.latent, c3, g3), (self.F3, 1, c3))
        pk(wfc, self.WfcT, (self.latent, c3, g3), (1, self.Lp, c3 * self.Lp))
        wd = P("decoder_cnn.fc.weight")                               # [c3][g3][L]
        pk(wd, self.Wdfc, (c3, g3, self.latent), (self.Lp, c3 * self.Lp, 1))
        pk(wd, self.WdfcT, (c3, g3, self.latent), (1, c3, self.F3))
        pk(P("decoder_cnn.fc.bias"), self.bdfc, (c3, g3, 1), (1, c3, 0), F32)
        Ld = self.latent
        for stack, wT in (("encoder_rnn", self.wT_enc), ("decoder_rnn", self.wT_dec)):
            for l in range(self.v.lstm_layers):
                for m, nm in enumerate(("weight_ih", "weight_hh")):
                    pk(P(f"{stack}.lstm.{nm}_l{l}"), wT[l, m], (4 * Ld, Ld, 1), (1, 4 * Ld, 0), F32)
        return jl

    # ---- helpers ---------------------------------------------------------------
    def _buf(self, tag, numel, dtype=torch.float32):
        """Persistent temporary (same address every step, so uploaded job tables stay valid)."""
        key = (tag, numel, dtype)
        t = self._bufs.get(key)
        if t is None:
            t = torch.empty(numel, dtype=dtype, device=self.device)
            self._bufs[key] = t
        return t

    def _gemm(self, A, W, out, bias, gate, mask, nimg, ih, iw, th, tw, sa, oh, ow, so, kc, nout, lda, ldo, taps,
              cls_key, relu=0, drop_mode=0, drop_p=0.0, scale=1.0, seed=0, bias_grad=None, colsum_ws=None,
              tag=None):
        """bias_grad: f32 [nout] tensor that receives the column sums of the stored output (a reduce job
        over the kernel's per-tile partial sums, run with the other jobs at the end of backward)."""
        seed_dev = self.seed_dev

        def colsum_rows(name, rows, nout):
            """The kernel's partial-sum workspace [rows][nout] and the job that reduces it into bias_grad (None without one)."""
            if bias_grad is None:
                return None
            ws = self._buf((name, tag), rows * nout)
            self._jobs.add(JOB_ROWS, ws, bias_grad, (1, 1, nout), (0, 0, 1), nslab=rows, slab=nout)
            return ws

        if (self.fc_gemm and cls_key == "one" and gate is None and mask is None and drop_mode == 0 and not relu
                and scale == 1.0 and bias_grad is None and nimg <= 4096 and nout >= 1024
                and ih * iw * th * tw * oh * ow == 1 and L.query("rbvae_fc_gemm_ok", self.dt, nimg, kc, nout, lda, ldo)):
            # the two fc products at the latent bottleneck: 0.13 GFLOP each, latency-bound (csrc/fc_gemm.hip)
            L.call("rbvae_fc_gemm", self.dt, A, W, out, bias, colsum_ws, nimg, kc, nout, lda, ldo)
            return
        if (cls_key == "dgrad" and self.k == 3 and self.deconv_halo and sa == 1 and so == 2 and taps == 9
                and (oh, ow) == (2 * th, 2 * tw) and (ih, iw) == (th, tw) and colsum_ws is None
                and L.query("rbvae_deconv3x3s2_halo_tile_rows", self.dt, nimg, th, tw, kc, nout) == 128):
            # transposed 3x3 / stride 2 (decoder forward, encoder input gradients): the four parity classes in one
            # workgroup over an LDS-resident input patch (csrc/deconv_halo.hip).  Launches of several rounds of
            # workgroups only: a one-round launch (the 256-frame step's 8x8 grids: 512 workgroups) runs as long as the
            # four class launches of the gather GEMM (35 vs 34 us), measured 7-25 % faster from 1 000 workgroups up; the
            # 128-row form only (two workgroups per CU): the 256-row form measured slower than the class launches
            rows4 = L.query("rbvae_deconv3x3s2_halo_colsum_rows", self.dt, nimg, th, tw, kc, nout)
            wgs = (rows4 // 4) * (nout // 64)
            if wgs >= self._dh_min_wgs:
                ws = colsum_rows("colsum_dh", rows4, nout)
                L.call("rbvae_deconv3x3s2_halo", self.dt, A, W, out, bias, gate, mask, self.zero, nimg, th, tw, kc, nout, lda,
                       ldo, relu, drop_mode, float(drop_p), float(scale), int(seed), seed_dev, ws)
                return
        if (cls_key == "conv" and self.k == 3 and self.conv_s2_halo and self.dt == BF16 and sa == 2 and so == 1 and taps == 9
                and (oh, ow) == (th, tw) and (ih, iw) == (2 * th, 2 * tw) and colsum_ws is None):
            # 3x3 stride-2 convolution (encoder forward, decoder input gradients) with the input patch resident in LDS
            # (csrc/conv_s2.hip): 8 x 16-pixel tiles, so small images (the bench shape's 8 x 8 / 4 x 4 maps) stay on the
            # row-gather GEMM, as do launches of less than a few rounds of workgroups
            bn = L.query("rbvae_conv3x3s2_halo_ok", self.dt, nimg, ih, iw, kc, nout)
            if bn:
                mt = L.query("rbvae_conv3x3s2_halo_colsum_rows", nimg, ih, iw)
                if mt * (nout // bn) >= self._cs_min_wgs and mt * 128 <= self._cs_max_waste * nimg * oh * ow:
                    ws = colsum_rows("colsum_cs", mt, nout)
                    L.call("rbvae_conv3x3s2_halo", self.dt, A, W, out, bias, gate, mask, nimg, ih, iw, kc, nout, lda, ldo, relu,
                           drop_mode, float(drop_p), float(scale), int(seed), seed_dev, ws)
                    return
        desc, ncls = self._descs[cls_key]
        ws = colsum_rows("colsum", ncls * (-(-(nimg * th * tw) // 128)), nout) if bias_grad is not None else colsum_ws
        L.call("rbvae_gather_gemm", self.dt, A, W, out, bias, gate, mask, None, self.zero, nimg, ih, iw, th, tw, sa, oh, ow,
               so, kc, nout, lda, ldo, taps, ncls, ctypes.addressof(desc), relu, drop_mode, float(drop_p),
               float(scale), int(seed), seed_dev, ws)

    def _conv_idx(self, nimg, ih, iw, oh, ow):
        """Gather-index table of a stride-2 convolution (cached per shape, read by weight-gradient GEMMs on ANY
        stream).  A table is complete in device memory before it enters the cache: its kernel is followed by a
        host-side stream synchronisation (first use of a shape only), so no consumer on another stream can ever
        read a table whose kernel it has not waited for.  During graph capture nothing may be built: the trainer's
        eager warm-up steps (or prepare()) have filled the cache by then."""
        key = (nimg, ih, iw, oh, ow)
        t = self._idx_cache.get(key)
        if t is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("gather-index table missing during graph capture: run Engine.prepare(N) or one "
                                   "eager step of this shape first")
            t = torch.empty(self.k * self.k * nimg * oh * ow, dtype=torch.int32, device=self.device)
            L.call("rbvae_conv_gather_index", t, nimg, ih, iw, oh, ow, self.k, self.k, 2, 1)
            torch.cuda.current_stream().synchronize()
            self._idx_cache[key] = t
        return t

    def prepare(self, N: int):
        """Build every device table a pass over N frames reads from more than one stream (the gather-index tables
        of the weight-gradient GEMMs), on the current stream, before any side stream is forked."""
        for ly in (self.conv2, self.conv3):
            self._conv_idx(N, *ly.big, *ly.small)

    def _wf_ksplit(self, N, Cin, IH, IW, Nout):
        """K-slices of rbvae_wgrad_first for this layer, or 0 when the im2col-row path stays (f32, a shape outside the
        kernel, or too few pixel blocks per workgroup: the bench shape keeps its rows -- 8 MB, 4 blocks per workgroup)."""
        if not (self.wgrad_first and self.dt == BF16 and self.k == 3):
            return 0
        nblk = L.query("rbvae_wgrad_first_blocks", self.dt, Cin, IH, IW, Nout, N)
        if nblk == 0:
            return 0
        if Nout % 256 == 0:
            ks = max(1, min(256 // (Nout // 256), nblk))       # all 256 channels of a block in one workgroup, one workgroup per CU
        else:
            ks = max(1, min(512 // (Nout // 64), nblk))        # two workgroups per CU
        return ks if nblk // ks >= self._wf_min_steps else 0

    def _wgrad_first(self, mode, x, fm, Dy, N, Cin, IH, IW, Nout, ldy, ks, out, dims, strides, tag=None):
        slabs = self._buf(("slabs", tag), ks * Nout * 64)
        L.call("rbvae_wgrad_first", self.dt, mode, x, *fm, Dy, slabs, self.zero, N, Cin, IH, IW, Nout, ldy, ks)
        self._wgrad_reduce(slabs, out, Nout, 64, 1, ks, dims, strides)

    def _wgrad(self, Dy, In, idx, P, Co, Ci, ldy, ldi, taps, out, dims, strides, tag=None, geom=None, cus=256):
        """wgrad GEMM into K-slice slabs; their fixed-order reduction into the torch layout is a job.
        geom = (Nimg, OH, OW, IH, IW) of a 3x3 stride-2 layer (Dy rows at OH x OW, In rows at IH x IW): with the nine taps
        in one workgroup (csrc/wgrad_halo.hip) when the launch gives every workgroup enough pixel blocks."""
        # a 3x3 stride-2 layer in bf16 with its gather table, In rows at twice the Dy extent: what both one-launch kernels need
        s2 = (geom is not None and self.dt == BF16 and self.k == 3 and taps == 9 and idx is not None
              and geom[3] == 2 * geom[1] and geom[4] == 2 * geom[2])

        def run(kernel, ks, fn, *args):
            slabs = self._buf(("slabs", tag), ks * Co * taps * Ci)
            self.last_wgrad_kernel = kernel
            L.call(fn, self.dt, Dy, In, slabs, *args, ks)
            self._wgrad_reduce(slabs, out, Co, Ci, taps, ks, dims, strides)

        if (s2 and self.wgrad_halo and Co % 64 == 0 and Ci % 64 == 0
                and L.query("rbvae_wgrad3x3s2_halo_ok", self.dt, geom[0], geom[1], geom[2], Co, Ci)):
            nimg, oh, ow = geom[:3]
            nblk = L.query("rbvae_wgrad3x3s2_halo_blocks", nimg, oh, ow)
            ntile = (Co // 64) * (Ci // 64)
            # K-slices: one round of workgroups on the CUs this launch can count on; at most ~40 MB of f32 slabs
            ks = max(1, min(cus // ntile, nblk, (40 << 20) // (Co * taps * Ci * 4)))
            # measured (tools/time_wgrad_halo.py): 64 x 64 channels 178 -> 71 us (cfg 3 conv2: the HBM time of its operands)
            # and 52 -> 27 us (conv3).  With 16 channel tiles per pixel block (256 x 256) a block's 32 KB stage is re-fetched
            # by every tile: the LDS-DMA alone takes 173 us (11 TB/s through the L2s), the MFMAs + fragment reads alone 137,
            # together 245 against rbvae_wgrad_gemm's 172 -- narrow layers only
            if nblk // ks >= self._wh_min_steps and ntile <= self._wh_max_tiles:
                return run("wgrad_halo_k", ks, "rbvae_wgrad3x3s2_halo", self.zero, nimg, oh, ow, Co, Ci, ldy, ldi)
        if (s2 and self.wgrad_row
                and L.query("rbvae_wgrad3x3s2_row_ok", self.dt, geom[0], geom[1], geom[2], Co, Ci)
                and L.query("rbvae_wgrad3x3s2_row_blocks", geom[0], geom[1], geom[2]) >= self._wr_min_blocks):
            # wide layers: the three taps of one kernel row per workgroup (csrc/wgrad_row.hip) -- 50 KB of operands per
            # 6.3 MFLOP instead of rbvae_wgrad_gemm's 96, LDS-DMA issued by waves of their own
            nimg, oh, ow = geom[:3]
            nblk = L.query("rbvae_wgrad3x3s2_row_blocks", nimg, oh, ow)
            ntile = (Co // 128) * (Ci // 128) * 3
            # K-slices: one round of workgroups on the CUs this launch can count on, every workgroup >= _wr_min_steps
            # blocks, at most ~_wr_slab_mb of f32 slabs
            ks = max(1, min(cus // ntile, nblk // self._wr_min_steps, (self._wr_slab_mb << 20) // (Co * taps * Ci * 4),
                            int(round(math.sqrt(self._wr_ks_coef * nblk)))))
            return run("wgrad_row_k", ks, "rbvae_wgrad3x3s2_row", self.zero, nimg, oh, ow, Co, Ci, ldy, ldi)
        blocks = -(-Co // 128) * -(-Ci // (128 if Ci > 64 else 64)) * taps
        # K-slices: one round of workgroups on the 256 CUs, each with >= 256 pixels, and at most ~16 MB of f32
        # slabs to reduce afterwards
        # (cus: the CUs this launch can count on -- beside the LSTM backward kernels, which hold one CU per
        # sequence and whose registers leave no room for a second workgroup there, a 252-workgroup grid ran in two
        # rounds: 31 -> 43 us)
        ks = max(1, min(cus // max(blocks, 1), P // 256 if P >= 256 else 1,
                        max(1, (4 << 20) // (Co * taps * Ci))))
        if blocks >= 8 and P <= 4096:
            # the 4096-pixel layers (conv3 / first deconv at the bench shape): 3 K-slices of 22 steps instead of 7 of 9
            # -- 7 MB of slabs per weight instead of 16.5 MB; same GPU, 2 runs each: 0.4738 (7) / 0.4665 (4) /
            # 0.4659 (3) / 0.472 (2) ms per step
            ks = min(ks, 3)
        ks = max(ks, -(-P // 4096))   # the kernel keeps a K-slice's gather indices in LDS
        run("wgrad_gemm_k<%d>" % (2 if Ci > 64 else 1), ks, "rbvae_wgrad_gemm", idx, self.zero, P, In.numel() // ldi, Co, Ci, ldy, ldi, taps)

    def _wgrad_reduce(self, slabs, out, Co, Ci, taps, ks, dims, strides):
        if (taps > 1 and taps <= 16 and tuple(dims) == (Co, Ci, taps) and tuple(strides) == (taps * Ci, 1, Ci)
                and Ci % 4 == 0):
            # conv / conv-transpose weight: the coalesced row kernel (16-byte loads of the slabs' [t][ci] rows, LDS
            # transpose, 16-byte stores of the torch-layout row)
            self._jobs.add_conv_reduce(slabs, out, Co, Ci, taps, ks)
        else:
            self._jobs.add(JOB_PERMUTE, slabs, out, dims, strides, nslab=ks, slab=Co * taps * Ci)

    def _colsum(self, dt, X, P, C, ld, out, tag=None):
        """Column sums of a tensor no GEMM epilogue produced: partial kernel now, final reduction as a job."""
        nf = L.query("rbvae_colsum_ws_floats", P, C)
        ws = self._buf(("cs", tag), nf)
        L.call("rbvae_colsum_partial", dt, X, P, C, ld, ws)
        self._jobs.add(JOB_ROWS, ws, out, (1, 1, C), (0, 0, 1), nslab=nf // C, slab=C)

    # ---- side stream ------------------------------------------------------------------
    # The LSTM chains occupy 2B workgroups for ~25 us per stack; weight-gradient GEMMs that do not feed them are
    # issued on a side stream over exactly those windows (graph capture turns the fork/join into graph edges).
    def _fork(self):
        """The side stream picks up after everything queued so far on the current stream."""
        if not self.overlap:
            return False
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.device)
        self._side.wait_stream(torch.cuda.current_stream())
        return True

    def _on_side(self):
        return torch.cuda.stream(self._side) if self.overlap else contextlib.nullcontext()

    def _join(self):
        if self.overlap and self._side is not None:
            torch.cuda.current_stream().wait_stream(self._side)

    def _run_jobs(self):
        jl, self._jobs = self._jobs, None
        sig = jl.signature()
        t = self._bwd_tab.get(sig)
        if t is None:
            t = self._bwd_tab[sig] = self._upload(jl)
        self.run_table(t.rows, t.n)

    def _E(self, *shape, dtype=None):
        return torch.empty(*shape, dtype=dtype or self.tdt, device=self.device)

    # ---- a layer's launches: every argument of _gemm / _wgrad that belongs to the layer comes from its record ----------
    # (reached as self._gemm / self._wgrad at call time: bench.py's roofline leg replaces both on the instance)
    def _one(self, A, W, out, bias, gate, mask, rows, kc, nout, **kw):
        """One-tap product out[rows][nout] = A[rows][kc] . W[nout][kc]^T, dense rows."""
        self._gemm(A, W, out, bias, gate, mask, rows, 1, 1, 1, 1, 1, 1, 1, 1, kc, nout, kc, nout, 1, "one", **kw)

    def _down(self, ly: Stride2, N, A, out, bias, gate, mask, **kw):
        """big -> small grid (the encoder's forward, the decoder's input gradients)."""
        (bh, bw), (sh, sw) = ly.big, ly.small
        self._gemm(A, ly.f, out, bias, gate, mask, N, bh, bw, sh, sw, 2, sh, sw, 1, ly.cb, ly.cs, ly.cb, ly.cs, self.kk,
                   "conv", **kw)

    def _up(self, ly: Stride2, N, A, out, bias, gate, mask, **kw):
        """small -> big grid (the decoder's forward, the encoder's input gradients)."""
        (bh, bw), (sh, sw) = ly.big, ly.small
        self._gemm(A, ly.d, out, bias, gate, mask, N, sh, sw, sh, sw, 1, bh, bw, 2, ly.cs, ly.cb, ly.cs, ly.cb, self.kk,
                   "dgrad", **kw)

    def _wgrad_s2(self, ly: Stride2, p: _Pass, small, big, tag, cus=256):
        """The layer's weight gradient from its small-grid and its big-grid tensor."""
        (bh, bw), (sh, sw) = ly.big, ly.small
        kk, cs, cb = self.kk, ly.cs, ly.cb
        self._wgrad(small, big, self._conv_idx(p.N, bh, bw, sh, sw), p.N * sh * sw, cs, cb, cs, cb, kk, p.G(ly.weight),
                    (cs, cb, kk), (kk * cb, 1, cb), tag=(p.N, tag), geom=(p.N, sh, sw, bh, bw), cus=cus)

    def _site(self, p: _Pass, j):
        """(keep-mask, epilogue keywords) of dropout site j = 1 .. 4: drop_mode 0 none, 1 hash keyed seed * 8 + j, 2 the mask."""
        m, mk = (0, None) if p.drop == 0 else (2, p.masks[j - 1]) if p.masks is not None else (1, None)
        return mk, dict(drop_mode=m, drop_p=p.drop, scale=p.sv.gate_scale, seed=p.seed * 8 + j)

    def _lstm_fwd(self, p: _Pass, stack, parts=None, cast=None):
        """One stack forward; stack = (weights, packed weights, hs, hp, acts, cs).  parts: its input as the fc's K-slabs,
        summed while staging; cast: the padded storage-dtype copy of its output -- both are the wavefront kernel's."""
        dims = (p.S, p.T, self.latent, self.v.lstm_layers)
        if parts is None and cast is None:
            L.call("rbvae_lstm_fwd", *stack, *dims)
        else:
            L.call("rbvae_lstm_fwd_ex", *stack, *dims,
                   *((None, 1, 0) if parts is None else (parts, self.fc_split, p.N * self.latent)),
                   *((None, 0, 0) if cast is None else (cast, self.dt, self.Lp)))

    def _lstm_bwd(self, p: _Pass, w, wT, acts, cs, dh, dG, d_in, nparts=1):
        """One stack's BPTT; nparts > 1: dh as that many K-slabs (the wavefront kernel sums them)."""
        dims = (p.S, p.T, self.latent, self.v.lstm_layers)
        if nparts > 1:
            L.call("rbvae_lstm_bwd_ex", w, acts, cs, dh, nparts, p.N * self.latent, dG, d_in, None, 0, 0, None, *dims)
        else:
            L.call("rbvae_lstm_bwd", w, wT, acts, cs, dh, dG, d_in, *dims)

    # ---- forward ---------------------------------------------------------------
    def forward(self, flat: torch.Tensor, x: torch.Tensor, U: torch.Tensor, tau: float, hard: bool, noise_ratio: float,
                train: bool, masks: Optional[Sequence[torch.Tensor]] = None, seed: int = 0, need_grad: bool = True,
                encode_only: bool = False, target: Optional[torch.Tensor] = None, recon_gscale: float = 0.0,
                kl_p: Optional[float] = None, after_hs=None, defer_losses: bool = False,
                frame_map: Optional[Tuple[int, int, int, int, int]] = None, tau_dev: Optional[torch.Tensor] = None,
                bwd_from_dpre: bool = False):
        """x: [S,T,C,H,W] f32 NCHW frames; U: [S*T, L] uniform noise.
        bwd_from_dpre: the caller will run backward(g_xr=None) on this call's Saved: the last deconv's input gradient may
        be computed here, in the launch that forms dpre3 (deconv_last_bwd_fused).
        tau_dev: optional device float the kernels read the temperature from instead of `tau` (graph-replayed
        steps under an annealing schedule; backward() reads the same tensor).
        masks: explicit dropout keep-masks (u8, NHWC rows) for the 4 dropout sites, else a counter hash.
        target/recon_gscale: fuse recon_loss and its gradient into the last kernel (trainer path).
        defer_losses: leave recon_loss and the KL mean as per-block partial sums ("sse": (ws, nparts, 1/n),
        "kl": (parts, nparts, 1/rows)) for rbvae_combine_losses to finish.
        frame_map: (d1, d2, s0, s1, s2) -- frame n of x (and of target) starts at element
        (n // d1) * s0 + ((n % d1) // d2) * s1 + (n % d2) * s2 of the buffer x points at (rbvae_im2col_frames).
        after_hs: optional callable(h_seq) issued on the side stream as soon as the encoder LSTM is done (the
        trainer's pairwise term runs there, beside the decoder); backward() joins it.
        Returns dict(xr, hs, z, e, kl, mse, saved)."""
        v = self.v
        S, T, C, H, W = x.shape
        if (H, W) != self.hw or C != self.in_ch:
            raise RuntimeError(f"input frames {tuple(x.shape[2:])} do not match the model's "
                               f"({self.in_ch}, {self.hw[0]}, {self.hw[1]})")
        drop = v.dropout if train else 0.0
        sv = Saved()
        sv.N, sv.S, sv.T, sv.hw, sv.train, sv.tau, sv.tau_dev, sv.hard = S * T, S, T, (H, W), train, tau, tau_dev, hard
        sv.gate_scale = 1.0 / (1.0 - drop) if drop > 0 else 1.0
        sv.dd2_fused = None
        p = _Pass(self, sv, flat)
        p.drop, p.masks, p.seed, p.frame_map = drop, masks, seed, frame_map
        p.U, p.r, p.kl_p, p.defer_losses = U, (noise_ratio if v.noise_ratio_arg else 1.0), kl_p, defer_losses
        # the encoder stack's launch is followed by this: the side stream picks up there; after_hs itself is issued behind
        # the main stream's continuation (end of forward())
        fork = self._fork if after_hs is not None else (lambda: None)
        self._fwd_encoder(p, x.contiguous())
        decode = v.simple_order or not encode_only
        hs, kl = self._fwd_latent(p, need_grad, decode, fork)
        if not decode:
            return {"z": sv.z.view(S, T, self.latent), "hs": hs, "saved": sv}
        self._fwd_decoder(p)
        mse, sse = self._fwd_last(p, target, recon_gscale, need_grad, bwd_from_dpre)
        if after_hs is not None and not v.simple_order:
            with self._on_side():
                after_hs(hs)
        return {"xr": sv.xr, "hs": hs, "z": sv.z.view(S, T, self.latent), "e": sv.e, "kl": kl, "mse": mse, "sse": sse,
                "saved": sv}

    def _fwd_encoder(self, p: _Pass, x):
        """frames -> a1 -> a2 -> a3."""
        sv, N, H, W, C, k = p.sv, p.N, p.H, p.W, self.in_ch, self.k
        c1, c2, c3 = self.v.channels
        sv.a1 = self._E(p.P1, c1)
        mk, kw = self._site(p, 1)
        sv.x_in, sv.fm_in = x, p.fm(C)
        fused1 = bool(k == 3 and self.K1 == 64 and kw["drop_mode"] != 2
                      and L.query("rbvae_conv_first_fused_ok", self.dt, C, H, W, c1, N))
        # the im2col rows are written for the weight gradient unless it rebuilds them from the frames (rbvae_wgrad_first)
        keep_col = not (fused1 and sv.train and self._wf_ksplit(N, C, H, W, c1))
        sv.col1 = self._E(p.P1, self.K1) if keep_col else None
        if fused1:
            # im2col + GEMM + bias/ReLU/dropout of the first conv in one kernel (csrc/conv_first.hip)
            L.call("rbvae_conv_first_fused", self.dt, x, *sv.fm_in, self.W1p, p.P(self.conv1.bias), self.zero, sv.col1, sv.a1,
                   N, C, H, W, c1, c1, 1, kw["drop_mode"], float(p.drop), float(sv.gate_scale), int(kw["seed"]), self.seed_dev)
        else:
            L.call("rbvae_im2col_frames", self.dt, x, *sv.fm_in, H * W, W, 1, N, C, H, W, *self.g1, k, k, 2, 1, self.K1, sv.col1)
            self._one(sv.col1, self.W1p, sv.a1, p.P(self.conv1.bias), None, mk, p.P1, self.K1, c1, relu=1, **kw)
        sv.a2 = self._E(p.P2, c2)
        mk, kw = self._site(p, 2)
        self._down(self.conv2, N, sv.a1, sv.a2, p.P(self.conv2.bias), None, mk, relu=1, **kw)
        sv.a3 = self._E(p.P3, c3)
        self._down(self.conv3, N, sv.a2, sv.a3, p.P(self.conv3.bias), None, None, relu=1 if self.v.simple_order else 0)

    def _fwd_latent(self, p: _Pass, need_grad, decode, fork):
        """a3 -> fc logits e -> LSTM stacks and binarisation in the variant's order -> ds_pad, the decoder fc's padded input
        (decode False: stops at the codes).  Returns (h_seq, kl)."""
        v, sv, N, S, T, Ld, f32 = self.v, p.sv, p.N, p.S, p.T, self.latent, torch.float32
        nl = v.lstm_layers
        sv.hs_enc = self._E(nl + 1, S, T, Ld, dtype=f32)
        sv.hs_dec = self._E(nl + 1, S, T, Ld, dtype=f32)
        sv.e = self._E(N, Ld, dtype=f32) if v.simple_order else sv.hs_enc[0].view(N, Ld)
        # the slab input / cast output exist in the wavefront kernel only, whose LDS need grows with T: asked per call of
        # the query the C dispatcher uses itself (long sequences take the plain kernels, the unsplit fc and rbvae_cast_pad)
        p.fwd_wave = self.wave_ok and bool(L.query("rbvae_lstm_fwd_wave_ok", T, Ld, nl))
        parts = (self.fc_split,) if self.fc_split > 1 and p.fwd_wave else ()       # the logits as K-slabs, or whole
        p.e_parts = self._buf((N, "e_parts"), self.fc_split * N * Ld) if parts else None
        L.call("rbvae_skinny_linear_parts" if parts else "rbvae_skinny_linear", self.dt, sv.a3, self.Wfc,
               p.P("encoder_cnn.fc.bias"), p.e_parts if parts else sv.e, N, Ld, self.F3, self.F3, self.F3, Ld, *parts)
        keep = (lambda w: self._E(nl, S, T, w, dtype=f32)) if need_grad else (lambda w: None)     # what only backward() reads
        sv.hp_enc, sv.cs_enc, sv.acts_enc, sv.hp_dec, sv.cs_dec, sv.acts_dec = (keep(w) for w in (Ld, Ld, 4 * Ld) * 2)
        sv.y = self._E(N, Ld, dtype=f32)
        sv.ds_pad = self._E(N, self.Lp) if decode else None
        p.enc = (p.P("encoder_rnn.lstm.weight_ih_l0"), self.wT_enc, sv.hs_enc, sv.hp_enc, sv.acts_enc, sv.cs_enc)
        p.dec = (p.P("decoder_rnn.lstm.weight_ih_l0"), self.wT_dec, sv.hs_dec, sv.hp_dec, sv.acts_dec, sv.cs_dec)
        # what the binarisation launches share: eps, hard, the KL term's p / eps / switch, the noise key (the closure must
        # not hold p: a cycle would keep a captured pass's tensors alive until the collector runs)
        tail = (int(p.seed) * 8 + 5, self.seed_dev)
        p.bin = lambda klp, kl_eps, on: (v.eps, int(sv.hard), float(klp), kl_eps, on, *tail)
        if v.simple_order:
            hs, kl, padded = self._fwd_latent_simple(p), (self._E(1, dtype=f32) if p.kl_p is not None else None), False
        elif decode and self.wave_ok and bool(L.query("rbvae_lstm_pair_fwd_ok", T, Ld, nl)):
            hs, kl, padded = *self._fwd_latent_pair(p, fork), True
        else:
            hs, kl, padded = *self._fwd_latent_stacks(p, decode, fork), p.fwd_wave
        if decode and not padded:       # no LSTM launch wrote ds_pad itself
            L.call("rbvae_cast_pad", self.dt, sv.hs_dec[nl], sv.ds_pad, N, Ld, self.Lp)
        return hs, kl

    def _fwd_latent_pair(self, p: _Pass, fork):
        """encoder stack -> binarise (+ KL sums) -> decoder stack as one wavefront launch."""
        sv, N, S, T, Ld, nl, kl_p = p.sv, p.N, p.S, p.T, self.latent, self.v.lstm_layers, p.kl_p
        hs, sv.z, kl = sv.hs_enc[nl], sv.hs_dec[0].view(N, Ld), None
        parts = self._E(S, dtype=torch.float32) if kl_p is not None else None
        (wenc, wTe, *enc), (wdec, wTd, *dec) = p.enc, p.dec
        L.call("rbvae_lstm_pair_fwd", wenc, wTe, wdec, wTd, *enc, *dec, p.e_parts, self.fc_split, N * Ld, p.U, sv.y,
               parts, float(sv.tau), sv.tau_dev, float(p.r), *p.bin(kl_p if kl_p is not None else 0.5, 1e-8, 1),
               sv.ds_pad, self.dt, self.Lp, S, T, Ld, nl)
        if kl_p is not None:
            kl = (parts, S, 1.0 / N) if p.defer_losses else (parts.sum() * (1.0 / N)).reshape(1)
        fork()
        return hs, kl

    def _fwd_latent_stacks(self, p: _Pass, decode, fork):
        """encoder stack, binarise (+ KL), decoder stack as launches of their own (sequences the pair kernel refuses)."""
        sv, N, Ld, nl, kl_p, U = p.sv, p.N, self.latent, self.v.lstm_layers, p.kl_p, p.U
        kl = self._E(1, dtype=torch.float32) if kl_p is not None else None
        self._lstm_fwd(p, p.enc, parts=p.e_parts)
        hs = sv.hs_enc[nl]
        fork()
        sv.z = sv.hs_dec[0].view(N, Ld)
        if p.defer_losses and kl_p is not None:
            nkl = L.query("rbvae_binarize_kl_nparts", N, Ld)
            parts = self._E(nkl, dtype=torch.float32)
            L.call("rbvae_binarize_kl_fwd_parts", hs, U, sv.y, sv.z, parts, N, Ld, float(sv.tau), sv.tau_dev, float(p.r),
                   *p.bin(kl_p, 1e-8, 1))
            kl = (parts, nkl, 1.0 / N)
        else:
            L.call("rbvae_binarize_kl_fwd", hs, U, sv.y, sv.z, kl, N, Ld, float(sv.tau), float(p.r),
                   *p.bin(kl_p if kl_p is not None else 0.5, 1e-8, 1))
        if decode:
            self._lstm_fwd(p, p.dec, cast=sv.ds_pad if p.fwd_wave else None)
        return hs, kl

    def _fwd_latent_simple(self, p: _Pass):
        """The simple variant's order: binarise the logits, then both stacks (plain kernels, no KL term)."""
        sv, N, Ld, nl = p.sv, p.N, self.latent, self.v.lstm_layers
        sv.z = sv.hs_enc[0].view(N, Ld)
        L.call("rbvae_binarize_kl_fwd", sv.e, p.U, sv.y, sv.z, None, N, Ld, float(sv.tau), float(p.r), *p.bin(0.5, 1e-10, 0))
        self._lstm_fwd(p, p.enc)
        hs = sv.hs_enc[nl]
        sv.hs_dec[0].copy_(hs)
        self._lstm_fwd(p, p.dec)
        return hs

    def _fwd_decoder(self, p: _Pass):
        """ds_pad -> fc -> f -> d1 -> d2."""
        sv, N = p.sv, p.N
        c1, c2, c3 = self.v.channels
        sv.f = self._E(p.P3, c3)
        self._one(sv.ds_pad, self.Wdfc, sv.f, self.bdfc, None, None, N, self.Lp, self.F3)
        sv.d1 = self._E(p.P2, c2)
        mk, kw = self._site(p, 3)
        self._up(self.deconv0, N, sv.f, sv.d1, p.P(self.deconv0.bias), None, mk, relu=1, **kw)
        sv.d2 = self._E(p.P1, c1)
        mk, kw = self._site(p, 4)
        self._up(self.deconv1, N, sv.d1, sv.d2, p.P(self.deconv1.bias), None, mk, relu=1, **kw)

    def _fwd_last(self, p: _Pass, target, recon_gscale, need_grad, bwd_from_dpre):
        """d2 -> x_recon, with a target the squared-error sums and (need_grad) dpre3 = d(loss)/d(pre-sigmoid); returns
        (mse, sse).  The fused kernel where it exists (3x3, eval or deferred losses), else product matrix + col2im."""
        sv, N, S, T, H, W, k, oc = p.sv, p.N, p.S, p.T, p.H, p.W, self.k, self.out_ch
        c1, (h1, w1) = self.v.channels[0], self.g1
        sv.xr = self._E(S, T, oc, H, W, dtype=torch.float32)
        mse = sse = ws = sv.dpre3 = sv.b3_parts = None
        b3 = p.P(self.deconv2.bias)
        fparts = L.query("rbvae_deconv_last_fused_parts", self.dt, N, h1, w1, c1, oc) if (
            k == 3 and (target is None or p.defer_losses)) else 0
        if target is not None:
            # persistent (one fused forward is in flight at a time): the backward pass's job table points into it
            ws = self._buf((N, "col2im_ws"), max(L.query("rbvae_col2im_ws_floats"), 5 * fparts))
            nparts = fparts or L.query("rbvae_col2im_nparts", sv.xr.numel())
            if p.defer_losses:    # per-block partial sums stay in ws; rbvae_combine_losses finishes the mean
                sse = (ws, nparts, 1.0 / sv.xr.numel())
            else:
                mse = self._E(1, dtype=torch.float32)
            if need_grad:
                sv.dpre3 = self._E(N, H, W, oc, dtype=torch.float32)
                if fparts or L.query("rbvae_col2im_has_dcol", N, h1, w1, self.NY, H, W, oc):
                    # the kernel leaves dpre3's per-block column sums (the last deconv's bias gradient) behind the
                    # squared-error sums in ws
                    sv.b3_parts = (ws, nparts)
        if fparts:
            # last deconv + sigmoid + recon loss as one kernel (products on the matrix cores from an LDS-resident pixel
            # block, kept in f32): no product matrix in HBM, no separate col2im pass
            nb2 = (L.query("rbvae_deconv_last_dgrad_blocks", self.dt, oc, H, W, c1, N)
                   if (self.deconv_last_bwd_fused and bwd_from_dpre and target is not None and need_grad
                       and p.defer_losses and self.K3 == 64
                       and L.query("rbvae_deconv_last_fwd_bwd_ok", self.dt, N, h1, w1, c1, oc)) else 0)
            fm = p.fm(oc)
            if nb2:
                # ... and the layer's input gradient from the same resident block: backward()'s buffers, filled here
                dd2 = p.tmp("dd2", p.P1, c1)
                col3 = None if self._wf_ksplit(N, oc, H, W, c1) else p.tmp("col3", p.P1, self.K3)
                ws2 = self._buf((N, "colsum_dd2f"), nb2 * c1)
                sv.dd2_fused = (dd2, col3, ws2, nb2)
                L.call("rbvae_deconv_last_fwd_bwd", self.dt, sv.d2, self.V3p, self.NY, self.V3f, b3, self.zero, N, h1, w1,
                       c1, oc, sv.xr, target.contiguous(), *fm, ws, sv.dpre3, float(recon_gscale), col3, dd2,
                       float(sv.gate_scale), ws2)
            else:
                L.call("rbvae_deconv_last_fused", self.dt, sv.d2, self.V3p, self.NY, b3, self.zero, N, h1, w1, c1, oc,
                       sv.xr, None if target is None else target.contiguous(), *fm, ws, sv.dpre3, float(recon_gscale))
            return mse, sse
        Y = self._E(p.P1, self.NY)
        self._one(sv.d2, self.V3p, Y, None, None, None, p.P1, c1, self.NY)
        framed = target is not None and p.frame_map is not None
        L.call("rbvae_col2im_sigmoid_frames" if framed else "rbvae_col2im_sigmoid", self.dt, Y, self.NY, b3, N, h1, w1, H, W,
               oc, k, k, 1, sv.xr, None if target is None else target.contiguous(), *(p.frame_map if framed else ()), mse, ws,
               sv.dpre3, float(recon_gscale) if target is not None else 0.0, None)
        return mse, sse

    # ---- backward --------------------------------------------------------------
    def backward(self, flat: torch.Tensor, gflat: torch.Tensor, sv: Saved, g_xr: Optional[torch.Tensor],
                 g_hs: Optional[torch.Tensor], g_z: Optional[torch.Tensor], g_e: Optional[torch.Tensor] = None,
                 kl_weight: float = 0.0, kl_p: float = 0.5, g_hs_inplace: bool = False, side_first=None, cut=None):
        """Writes every parameter gradient into gflat (same layout as flat).
        g_xr: [S,T,C,H,W] upstream gradient of x_recon (None: use the fused dpre3 of forward()).
        g_hs / g_z: [S,T,L] upstream gradients of h_seq / z_seq (None = 0).
        g_e: upstream gradient of the conv logits (simple variant's second output).
        kl_weight: d(loss)/d(kl_mean) when the KL term was fused into forward().
        g_hs_inplace: the caller gives g_hs away (the binarise backward accumulates into it).
        side_first: optional callable issued on the side stream before anything else of this pass (the trainer's
        loss bookkeeping: everything it reads exists once forward() is done).
        cut: optional callable invoked once, on the main stream with every side stream joined, at the point where the
        gradients of decoder_cnn.* and both LSTM stacks (the contiguous tail of gflat from
        layout.offsets["decoder_cnn.fc.weight"]) are final and only the encoder CNN's remain to be computed: the
        data-parallel trainer ends one graph and starts the next there and all-reduces that tail beside the rest."""
        # The schedule: which stage (_bwd_*: they know nothing of streams) is issued when, and on which stream
        self._join()                       # side-stream work of forward() (after_hs)
        # the loss bookkeeping rides the side stream's fork for the decoder's weight gradients (no edge of its own)
        book_with_decoder = side_first is not None and self.overlap
        if side_first is not None and not book_with_decoder:
            side_first()
        p = _Pass(self, sv, flat, gflat)
        self._jobs = JobList()
        # decoder CNN, data-gradient chain first (main stream) ...
        self._bwd_last_dgrad(p, g_xr)
        self._bwd_decoder_dgrads(p)
        # ... then its weight / bias gradients, beside the LSTM chain when overlap is on.  The gather-index tables both
        # streams' weight-gradient GEMMs read are complete before they enter the cache (_conv_idx), built here on the
        # main stream before the fork
        self.prepare(p.N)
        self._fork()
        # with a cut the reductions queued so far (decoder bias sums: their producers ran before the fork) go with the
        # decoder's early reduction, so that every decoder gradient is final at the cut
        fork_jobs = None
        if cut is not None:
            fork_jobs, self._jobs = self._jobs, JobList()
        side_tail = []                # (event, callable): issued on the side stream behind the decoder's weight gradients

        def issue_decoder_side():
            early = self.overlap or cut is not None
            main_jobs, self._jobs = self._jobs, (fork_jobs if cut is not None else JobList())
            with self._on_side():
                if book_with_decoder:
                    side_first()
                # (with overlap the LSTM backward kernels run beside these: S workgroups that hold one CU each)
                self._bwd_decoder_wgrads(p, g_xr, cus=max(64, 256 - min(p.S, 128)) if self.overlap else 256)
                if early:
                    # the decoder's slab / partial-sum reductions right behind them, not at the end of the pass
                    self._run_jobs()
                else:
                    main_jobs.rows += self._jobs.rows
                    main_jobs.keep += self._jobs.keep
                # late side work: launches of the main chain's own products that nothing on that chain waits for; their
                # reduction jobs join the final reduction
                self._jobs = main_jobs
                for ev, fn in side_tail:
                    self._side.wait_event(ev)
                    fn()

        # the main stream's continuation is issued BEFORE the side work (see __init__)
        defer_side = self.overlap
        if not defer_side:
            issue_decoder_side()
        self._bwd_latent(p, g_z, g_hs, g_e, kl_weight, kl_p, g_hs_inplace)
        # Side-stream tail (behind the decoder's weight gradients, each piece behind an event on its inputs): launches
        # of the main chain's products that nothing on the chain waits for
        tail_ok = defer_side and cut is None

        def tail(fn):
            if not tail_ok:
                return fn()
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream())
            side_tail.append((ev, fn))

        tail(lambda: self._bwd_lstm_wgrads(p))          # behind ev_bptt: dG_dec / dG_enc are written
        self._bwd_fc_bias(p, g_e)
        # The encoder fc's weight gradient is a 32-workgroup launch nothing on the data-gradient chain waits for: with
        # the deferred side work it rides the side stream (behind ev_de, an event on de_pad), so the main chain goes
        # straight on to the next data-gradient GEMM instead of queueing it behind a full chip (18 us in the step)
        tail(lambda: self._bwd_fc_wgrad(p))
        # (the encoder's full-chip weight gradients stay on the main stream: on the side stream's tail they only contend
        # with the data-gradient GEMMs, 0.458 -> 0.476 / 0.487 ms per step in round 2)
        self._bwd_fc_conv3(p)
        if cut is not None:
            # here, not right behind the LSTM kernels: the decoder's weight gradients on the side stream take about as
            # long as the main chain needs to get this far, so the join costs no idle time (at the LSTM kernels it cost
            # 76 us per step, one-rank RCCL rehearsal)
            if defer_side:
                issue_decoder_side()
                defer_side = False
            self._join()
            cut()
        self._bwd_conv2_conv1(p)
        if defer_side:
            issue_decoder_side()
        # every slab / partial-sum reduction of this pass in one launch, once the side stream has caught up
        self._join()
        self._run_jobs()

    def _bwd_last_dgrad(self, p: _Pass, g_xr):
        """dpre3 (from g_xr, or forward()'s) -> dd2, the last deconv's input gradient gated by d2, with deconv1's bias
        gradient; col3 = dpre3's im2col rows unless the weight gradient reads dpre3 itself (wf3 K-slices)."""
        sv, N, H, W, k, oc, gs = p.sv, p.N, p.H, p.W, self.k, self.out_ch, p.sv.gate_scale
        c1, (h1, w1) = self.v.channels[0], self.g1
        if g_xr is not None:
            p.dpre3 = p.tmp("dpre3", N, H, W, oc, dtype=torch.float32)
            L.call("rbvae_sigmoid_bwd_nhwc", g_xr.contiguous(), sv.xr, p.dpre3, N, oc, H, W)
        else:
            p.dpre3 = sv.dpre3
            if p.dpre3 is None:
                raise RuntimeError("backward without g_xr needs forward(target=..., need_grad=True)")
        p.dd2 = dd2 = p.tmp("dd2", p.P1, c1)
        nb = L.query("rbvae_deconv_last_dgrad_blocks", self.dt, oc, H, W, c1, N) if k == 3 and self.K3 == 64 else 0
        p.wf3 = self._wf_ksplit(N, oc, H, W, c1) if nb else 0      # the last deconv's weight gradient from dpre3 itself
        p.col3 = col3 = None if p.wf3 else p.tmp("col3", p.P1, self.K3)
        gb = p.G(self.deconv1.bias)
        if nb:
            # im2col + GEMM + gate + bias-gradient partial sums in one kernel (csrc/conv_first.hip, MODE 1)
            ws = self._buf((N, "colsum_dd2f"), nb * c1)
            if g_xr is None and sv.dd2_fused is not None:
                # forward() left dd2, col3 and the column sums in these very buffers (rbvae_deconv_last_fwd_bwd)
                assert sv.dd2_fused[0].data_ptr() == dd2.data_ptr() and sv.dd2_fused[2].data_ptr() == ws.data_ptr()
                assert (sv.dd2_fused[1] is None) == (col3 is None) and sv.dd2_fused[3] == nb
            else:
                L.call("rbvae_deconv_last_dgrad_fused", self.dt, p.dpre3, self.V3f, self.zero, col3, sv.d2, dd2, N, oc, H, W,
                       c1, c1, float(gs), ws)
            self._jobs.add(JOB_ROWS, ws, gb, (1, 1, c1), (0, 0, 1), nslab=nb, slab=c1)
        else:
            L.call("rbvae_im2col", self.dt, p.dpre3, H * W * oc, 1, W * oc, oc, N, oc, H, W, h1, w1, k, k, 2, 1, self.K3, col3)
            self._one(col3, self.V3f, dd2, None, sv.d2, None, p.P1, self.K3, c1, scale=gs, bias_grad=gb, tag=(N, "dd2"))

    def _bwd_decoder_dgrads(self, p: _Pass):
        """dd2 -> dd1 -> df: a deconv's input gradient = the conv forward of its output gradient with the same weights."""
        sv, N = p.sv, p.N
        p.dd1 = p.tmp("dd1", p.P2, self.deconv1.cs)
        self._down(self.deconv1, N, p.dd2, p.dd1, None, sv.d1, None, scale=sv.gate_scale,
                   bias_grad=p.G(self.deconv0.bias), tag=(N, "dd1"))
        p.df = p.tmp("df", p.P3, self.deconv0.cs)
        self._down(self.deconv0, N, p.dd1, p.df, None, None, None)

    def _bwd_decoder_wgrads(self, p: _Pass, g_xr, cus):
        """Weight / bias gradients of the three deconvs and the decoder fc, on the `cus` CUs their launches can count on."""
        sv, N, H, W, oc, kk, G = p.sv, p.N, p.H, p.W, self.out_ch, self.kk, p.G
        c1, c2, c3 = self.v.channels
        g3 = self.g3[0] * self.g3[1]
        if g_xr is None and sv.b3_parts is not None:
            ws_b3, nb3 = sv.b3_parts
            self._jobs.add(JOB_ROWS, ws_b3[nb3:], G(self.deconv2.bias), (1, 1, oc), (0, 0, 1), nslab=nb3, slab=4)
        else:
            self._colsum(F32, p.dpre3, N * H * W, oc, oc, G(self.deconv2.bias), tag=(N, "b3"))
        if p.wf3:
            self._wgrad_first(1, p.dpre3, (0, 0, 0, 0, 0), sv.d2, N, oc, H, W, c1, c1, p.wf3, G(self.deconv2.weight),
                              (c1, oc, kk), (self.K3, 1, oc), tag=(N, "V3"))
        else:
            self._wgrad(sv.d2, p.col3, None, p.P1, c1, self.K3, c1, self.K3, 1, G(self.deconv2.weight), (c1, oc, kk),
                        (self.K3, 1, oc), tag=(N, "V3"), cus=cus)
        self._wgrad_s2(self.deconv1, p, sv.d1, p.dd2, "V2", cus)
        self._wgrad_s2(self.deconv0, p, sv.f, p.dd1, "V1", cus)
        # decoder fc: bias = per (position, channel) sum over frames, permuted to the torch (c, hw) order
        nf = L.query("rbvae_colsum_ws_floats", N, self.F3)
        wsf = self._buf((N, "bdfc"), nf)
        L.call("rbvae_colsum_partial", self.dt, p.df, N, self.F3, self.F3, wsf)
        self._jobs.add(JOB_PERMUTE, wsf, G("decoder_cnn.fc.bias"), (c3, g3, 1), (1, c3, 0), nslab=nf // self.F3, slab=self.F3)
        self._wgrad(p.df, sv.ds_pad, None, N, self.F3, self.Lp, self.F3, self.Lp, 1, G("decoder_cnn.fc.weight"),
                    (c3, g3, self.latent), (self.Lp, c3 * self.Lp, 1), tag=(N, "Wdfc"), cus=cus)

    def _bwd_latent(self, p: _Pass, g_z, g_hs, g_e, kl_weight, kl_p, g_hs_inplace):
        """df -> decoder fc -> decoder stack -> binarise backward (+ fused KL) -> encoder stack (the simple variant: both
        stacks, then the binarisation) -> de, the logits' gradient.  Leaves dG / dGe for the LSTM weight gradients and,
        from the wavefront kernels, de's padded copy and its per-sequence column sums (the fc bias gradient)."""
        v, sv, N, S, T, Ld, nl, f32 = self.v, p.sv, p.N, p.S, p.T, self.latent, self.v.lstm_layers, torch.float32
        # as in forward(): slab sums, the cast copy, the column sums and the fused binarise backward are the wavefront
        # kernel's, which long sequences do not fit
        bwd_wave = self.wave_ok and bool(L.query("rbvae_lstm_bwd_wave_ok", T, Ld, nl))
        split = self.fc_split if bwd_wave else 1
        parts = (split,) if split > 1 else ()        # the decoder fc's input gradient: K-slabs the BPTT launch sums, or whole
        dds = p.tmp("dds", *parts, N, Ld, dtype=f32)
        L.call("rbvae_skinny_linear_parts" if parts else "rbvae_skinny_linear", self.dt, p.df, self.WdfcT, None, dds, N, Ld,
               self.F3, self.F3, self.F3, Ld, *parts)
        wenc, wdec = p.P("encoder_rnn.lstm.weight_ih_l0"), p.P("decoder_rnn.lstm.weight_ih_l0")
        p.dG = dG = p.tmp("dG_dec", nl, S, T, 4 * Ld, dtype=f32)
        p.dGe = dGe = p.tmp("dG_enc", nl, S, T, 4 * Ld, dtype=f32)
        d_in_dec = p.tmp("d_in_dec", N, Ld, dtype=f32)
        p.de = de = p.tmp("de", N, Ld, dtype=f32)
        p.de_pad = de_pad = p.tmp("de_pad", N, self.Lp) if bwd_wave else None
        p.de_sums = de_sums = self._buf((N, "de_sums"), S * Ld) if bwd_wave else None
        rows = lambda g: None if g is None else g.reshape(N, Ld).contiguous()
        bin_args = (float(sv.tau), sv.tau_dev, float(kl_weight), float(kl_p), 1e-8, 1)
        if bwd_wave and L.query("rbvae_lstm_pair_bwd_ok", T, Ld, nl):
            # decoder stack -> binarise backward (+ fused KL) -> encoder stack: one wavefront launch (the codes'
            # gradient is not stored: None)
            L.call("rbvae_lstm_pair_bwd", wenc, wdec, sv.acts_enc, sv.cs_enc, sv.acts_dec, sv.cs_dec, dds, split, N * Ld,
                   rows(g_z), sv.y, sv.z, rows(g_hs), *bin_args, dGe, dG, de, None, de_pad, self.dt, self.Lp, de_sums,
                   S, T, Ld, nl)
            return
        self._lstm_bwd(p, wdec, self.wT_dec, sv.acts_dec, sv.cs_dec, dds, dG, d_in_dec, nparts=split)
        if v.simple_order:
            # decoder stack input = encoder stack output
            dz = p.tmp("dz", N, Ld, dtype=f32)
            self._lstm_bwd(p, wenc, self.wT_enc, sv.acts_enc, sv.cs_enc, d_in_dec, dGe, dz)
            L.call("rbvae_binarize_kl_bwd", dz, sv.y, sv.z, de, 0, N, Ld, float(sv.tau), None, 0.0, None, 0.5, 1e-10, 0)
            if g_e is not None:
                p.de = de + g_e.reshape(N, Ld)
            return
        # z -> binarise backward (+ fused KL) -> gradient of h_seq
        gz = d_in_dec if g_z is None else d_in_dec + g_z.reshape(N, Ld)
        if bwd_wave:
            # ... in the prologue of the encoder stack's BPTT launch
            L.call("rbvae_lstm_bwd_bin", wenc, sv.acts_enc, sv.cs_enc, gz, sv.y, sv.z, rows(g_hs), *bin_args, dGe, de,
                   de_pad, self.dt, self.Lp, de_sums, S, T, Ld, nl)
            return
        inplace = g_hs is not None and g_hs_inplace and g_hs.is_contiguous()
        dh = g_hs.view(N, Ld) if inplace else p.tmp("dh", N, Ld, dtype=f32)
        L.call("rbvae_binarize_kl_bwd", gz, sv.y, sv.z, dh, int(inplace), N, Ld, float(sv.tau), sv.tau_dev,
               float(kl_weight), None, float(kl_p), 1e-8, 1)
        if g_hs is not None and not inplace:
            dh = dh + g_hs.reshape(N, Ld)
        self._lstm_bwd(p, wenc, self.wT_enc, sv.acts_enc, sv.cs_enc, dh, dGe, de)

    def _bwd_lstm_wgrads(self, p: _Pass):
        sv = p.sv
        L.call("rbvae_lstm_wgrad_pair", p.dG, sv.hs_dec, sv.hp_dec, p.G("decoder_rnn.lstm.weight_ih_l0"),
               p.dGe, sv.hs_enc, sv.hp_enc, p.G("encoder_rnn.lstm.weight_ih_l0"), p.S, p.T, self.latent, self.v.lstm_layers, 0)

    def _bwd_fc_bias(self, p: _Pass, g_e):
        """The encoder fc's bias gradient (column sums of de) and de's padded copy, where the LSTM launch left neither."""
        N, Ld = p.N, self.latent
        if p.de_sums is not None and g_e is None:
            self._jobs.add(JOB_ROWS, p.de_sums, p.G("encoder_cnn.fc.bias"), (1, 1, Ld), (0, 0, 1), nslab=p.S, slab=Ld)
        else:
            self._colsum(F32, p.de, N, Ld, Ld, p.G("encoder_cnn.fc.bias"), tag=(N, "bfc"))
        if p.de_pad is None:
            p.de_pad = p.tmp("de_pad", N, self.Lp)
            L.call("rbvae_cast_pad", self.dt, p.de, p.de_pad, N, Ld, self.Lp)

    def _bwd_fc_wgrad(self, p: _Pass):
        c3, g3 = self.v.channels[2], self.g3[0] * self.g3[1]
        self._wgrad(p.de_pad, p.sv.a3, None, p.N, self.Lp, self.F3, self.Lp, self.F3, 1, p.G("encoder_cnn.fc.weight"),
                    (self.latent, c3, g3), (self.F3, 1, c3), tag=(p.N, "Wfc"))

    def _bwd_fc_conv3(self, p: _Pass):
        """de_pad -> da3 (gated by a3 in the simple variant) -> da2, with conv3's / conv2's bias and conv3's weight gradient."""
        N, c3, g3 = p.N, self.v.channels[2], self.g3[0] * self.g3[1]
        p.da3 = p.tmp("da3", p.P3, c3)
        # the GEMM sees da3 as [N][F3]; its fused column sums [m-tiles][F3] are [m-tiles*g3][c3] rows,
        # so the conv3 bias gradient is one row-reduce job over them
        mt = -(-N // 128)
        ws3 = self._buf((N, "ws3"), mt * self.F3)
        self._one(p.de_pad, self.WfcT, p.da3, None, p.sv.a3 if self.v.simple_order else None, None, N, self.Lp, self.F3,
                  colsum_ws=ws3)
        self._jobs.add(JOB_ROWS, ws3, p.G(self.conv3.bias), (1, 1, c3), (0, 0, 1), nslab=mt * g3, slab=c3)
        self._wgrad_s2(self.conv3, p, p.da3, p.sv.a2, "W3")
        p.da2 = p.tmp("da2", p.P2, self.conv3.cb)
        self._up(self.conv3, N, p.da3, p.da2, None, p.sv.a2, None, scale=p.sv.gate_scale, bias_grad=p.G(self.conv2.bias),
                 tag=(N, "da2"))

    def _bwd_conv2_conv1(self, p: _Pass):
        """conv2's weight gradient; da2 -> da1 with conv1's bias gradient; conv1's weight gradient (frames or im2col rows)."""
        sv, N, H, W, C, kk = p.sv, p.N, p.H, p.W, self.in_ch, self.kk
        c1 = self.v.channels[0]
        self._wgrad_s2(self.conv2, p, p.da2, sv.a1, "W2")
        da1 = p.tmp("da1", p.P1, c1)
        self._up(self.conv2, N, p.da2, da1, None, sv.a1, None, scale=sv.gate_scale, bias_grad=p.G(self.conv1.bias),
                 tag=(N, "da1"))
        out, dims, strides = p.G(self.conv1.weight), (c1, C, kk), (self.K1, 1, C)
        if sv.col1 is None:
            wf1 = self._wf_ksplit(N, C, H, W, c1)
            self._wgrad_first(0, sv.x_in, sv.fm_in, da1, N, C, H, W, c1, c1, wf1, out, dims, strides, tag=(N, "W1"))
        else:
            self._wgrad(da1, sv.col1, None, p.P1, c1, self.K1, c1, self.K1, 1, out, dims, strides, tag=(N, "W1"))
