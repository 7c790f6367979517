"""Cases and host helpers of the step tests that take the engine's large-frame kernel arms (test_step_arms_cpu.py,
test_step_arms_gpu.py): one fused bf16 training step per case, B = 1, T = 2 (four frames), explicit U, against the f64
oracle.  Host code only: nothing here touches the device.

The arms are the entry points engine._gemm / engine._wgrad / engine.forward / engine.backward switch to by shape and
launch size.  A case lowers the launch-size thresholds only (lower_thresholds); the shape predicates stay as shipped, so
which arm takes which layer below is what the library's own queries answer for four frames of that size.

  case        frame                maps                     mode    reaches
  1 native    percep 4 x 88 x 160  44x80, 22x40, 11x20      eval    the non-power-of-two bottleneck; deconv_halo on the 22x40
                                                                    map (11x20 fits the 256-row form only: gather GEMM),
                                                                    wgrad_row at 256 channels with 55 and 15 (ragged) blocks,
                                                                    wgrad_first and deconv_last_fwd_bwd with col = NULL,
                                                                    fc_gemm with fc_split = 16
  2 halo64    percep 4 x 64 x 64   32x32, 16x16, 8x8        train   conv3x3s2_halo where its 8 x 16 tiles fit (32x32 -> 16x16,
                                                                    forward and, with its column sums, backward), deconv_halo on
                                                                    both maps forward and backward, the keyed drop path of
                                                                    conv_first_fused, wgrad_first for both ends
  3 narrow    contrastive 3x48x80  24x40, 12x20, 6x10       eval    64-channel layers: wgrad_halo, conv_first_fused and
                                                                    wgrad_first with Cin = 3
  4 triplet   triplet 3 x 64 x 64  32x32, 16x16, 8x8        train   the 64-channel arms beside the triplet term

No frame size had to be moved: every predicate the table of the issue expected to accept a shape accepts it."""
import torch

from _ends_cases import keyed_keep_mask

B, T, LATENT = 1, 2, 32
TAU, NOISE_RATIO, BERNOULLI_P, ALPHA, BETA, MARGIN, LR = 0.7, 0.1, 0.1, 1.0, 1.0, 1.0, 1e-3
SEED = 17                                           # the trainer's noise seed (keyed dropout)

# the bf16 gates of test_bench_shape_step_against_oracle
LOSS_TOL = 1e-2                                     # * max(1, |ref|), against the plain f32 oracle
GRAD_MATCHED = 1.5e-2                               # relative L2 against the f64 oracle under the device's ReLU decisions
GRAD_UNCONDITIONED = 0.15                           # ... against the plain f64 oracle
TIE_BOUND, TIE_FRACTION = 0.1, 1e-3                 # differing decisions: |pre-activation| below, share of the live ones
REORDER = 2e-5                                      # same bf16 products, f32 sums in another order

CONV_S2, DECONV_HALO, WGRAD_HALO, WGRAD_ROW, WGRAD_FIRST, CONV_FIRST, DECONV_LAST, FC_GEMM = ARMS = (
    "rbvae_conv3x3s2_halo", "rbvae_deconv3x3s2_halo", "rbvae_wgrad3x3s2_halo", "rbvae_wgrad3x3s2_row", "rbvae_wgrad_first",
    "rbvae_conv_first_fused", "rbvae_deconv_last_fwd_bwd", "rbvae_fc_gemm")

# engine attributes: the five arms a flag turns off, and the weight-gradient three among them
SWITCHES = {"deconv_halo": DECONV_HALO, "conv_s2_halo": CONV_S2, "wgrad_halo": WGRAD_HALO, "wgrad_row": WGRAD_ROW,
            "wgrad_first": WGRAD_FIRST}
WGRAD_SWITCHES = ("wgrad_halo", "wgrad_row", "wgrad_first")
MODES = {"on": (), "off": tuple(SWITCHES), "wgrad_off": WGRAD_SWITCHES}

# The arm launches of one step in issue order (forward; backward's main chain; the decoder's weight gradients, issued last
# for the side stream), each with the predicate that admits it at N = 4 frames.
CASES = [
    dict(id="native_88x160", variant="percep", in_ch=4, hw=(88, 160), train=False, model_seed=71, data_seed=72, launches=[
        (CONV_FIRST, "conv1: rbvae_conv_first_fused_ok(bf16, 4, 88, 160, 256, N), K1 = 64"),
        (FC_GEMM, "decoder fc: one tap, no epilogue, nout = F3 = 56 320 >= 1024, rbvae_fc_gemm_ok"),
        (DECONV_HALO, "deconv1 22x40 -> 44x80: rbvae_deconv3x3s2_halo_tile_rows == 128 (112 workgroups >= _dh_min_wgs = 1)"),
        (DECONV_LAST, "last deconv + loss + dd2: rbvae_deconv_last_fwd_bwd_ok, K3 = 64; col = NULL (wgrad_first takes V3)"),
        (FC_GEMM, "da3 = de . Wfc^T with its column sums (ws3)"),
        (WGRAD_ROW, "conv3 weight, 11x20 map: rbvae_wgrad3x3s2_row_ok, 15 blocks >= _wr_min_blocks = 1 (16 tiles: not wgrad_halo)"),
        (WGRAD_ROW, "conv2 weight, 22x40 map: 55 blocks"),
        (DECONV_HALO, "da1 22x40 -> 44x80 with conv1's bias gradient through ('colsum_dh', tag): 112 rows"),
        (WGRAD_FIRST, "last deconv's weight from dpre3 (mode 1): rbvae_wgrad_first_blocks = 120 >= ks * _wf_min_steps"),
        (WGRAD_ROW, "deconv1 weight, 22x40 map"),
        (WGRAD_ROW, "deconv0 weight, 11x20 map"),
    ]),     # eval: conv1's weight gradient keeps its im2col rows (engine.forward: keep_col unless train), deconv0 / da2 on the
            # 11x20 map fit the 256-row form only, conv2 / conv3 / dd1 / df waste 1.31 / 2.33 of their 8 x 16 tiles
    dict(id="halo_64x64", variant="percep", in_ch=4, hw=(64, 64), train=True, model_seed=73, data_seed=74, launches=[
        (CONV_FIRST, "conv1 with the keyed dropout (drop_mode 1)"),
        (CONV_S2, "conv2 32x32 -> 16x16: rbvae_conv3x3s2_halo_ok = 256, 8 tiles cover the map 1.0 times <= _cs_max_waste"),
        (FC_GEMM, "decoder fc, nout = F3 = 16 384"),
        (DECONV_HALO, "deconv0 8x8 -> 16x16: tile_rows == 128, 8 workgroups"),
        (DECONV_HALO, "deconv1 16x16 -> 32x32: 32 workgroups"),
        (DECONV_LAST, "last deconv + loss + dd2, col = NULL"),
        (CONV_S2, "dd1 32x32 -> 16x16 with deconv0's bias gradient through ('colsum_cs', tag): 8 rows"),
        (FC_GEMM, "da3"),
        (WGRAD_ROW, "conv3 weight, 8x8 map: 4 blocks"),
        (DECONV_HALO, "da2 8x8 -> 16x16 with conv2's bias gradient through ('colsum_dh', tag)"),
        (WGRAD_ROW, "conv2 weight, 16x16 map: 16 blocks"),
        (DECONV_HALO, "da1 16x16 -> 32x32 with conv1's bias gradient"),
        (WGRAD_FIRST, "conv1 weight from the frames (mode 0; train: no im2col rows kept): 32 blocks"),
        (WGRAD_FIRST, "last deconv's weight from dpre3 (mode 1)"),
        (WGRAD_ROW, "deconv1 weight, 16x16 map"),
        (WGRAD_ROW, "deconv0 weight, 8x8 map"),
    ]),     # conv3 / df 16x16 -> 8x8: their tiles cover the 8x8 map twice, gather GEMM
    dict(id="narrow_48x80", variant="contrastive", in_ch=3, hw=(48, 80), train=False, model_seed=75, data_seed=76, launches=[
        (CONV_FIRST, "conv1, Cin = 3: rbvae_conv_first_fused_ok(bf16, 3, 48, 80, 64, N)"),
        (FC_GEMM, "decoder fc, nout = F3 = 3840"),
        (DECONV_LAST, "last deconv + loss + dd2, 3 output channels, col = NULL"),
        (FC_GEMM, "da3"),
        (WGRAD_HALO, "conv3 weight, 6x10 map: rbvae_wgrad3x3s2_halo_ok, one 64 x 64 tile <= _wh_max_tiles, 16 blocks"),
        (WGRAD_HALO, "conv2 weight, 12x20 map: 36 blocks"),
        (WGRAD_FIRST, "last deconv's weight from dpre3, Cin = 3: 36 blocks"),
        (WGRAD_HALO, "deconv1 weight, 12x20 map"),
        (WGRAD_HALO, "deconv0 weight, 6x10 map"),
    ]),     # 64 channels: conv3x3s2_halo refuses them, deconv_halo has the 256-row form only (12x20) or none (6x10)
    dict(id="triplet_64x64", variant="triplet", in_ch=3, hw=(64, 64), train=True, model_seed=77, data_seed=78, launches=[
        (CONV_FIRST, "conv1, Cin = 3, keyed dropout"),
        (FC_GEMM, "decoder fc, nout = F3 = 4096"),
        (DECONV_HALO, "deconv0 8x8 -> 16x16, 64 channels: tile_rows == 128, 2 workgroups"),
        (DECONV_HALO, "deconv1 16x16 -> 32x32: 8 workgroups"),
        (DECONV_LAST, "last deconv + loss + dd2, col = NULL"),
        (FC_GEMM, "da3"),
        (WGRAD_HALO, "conv3 weight, 8x8 map: 8 blocks"),
        (DECONV_HALO, "da2 with conv2's bias gradient"),
        (WGRAD_HALO, "conv2 weight, 16x16 map: 32 blocks"),
        (DECONV_HALO, "da1 with conv1's bias gradient"),
        (WGRAD_FIRST, "conv1 weight from the frames, Cin = 3"),
        (WGRAD_FIRST, "last deconv's weight from dpre3"),
        (WGRAD_HALO, "deconv1 weight"),
        (WGRAD_HALO, "deconv0 weight"),
    ]),
]
BY_ID = {c["id"]: c for c in CASES}
IDS = [c["id"] for c in CASES]
GRAPH_IDS = ["native_88x160", "halo_64x64"]


def expected_launches(case, mode="on"):
    """The pinned arm launches of `case` with the switches of `mode` off."""
    off = {SWITCHES[s] for s in MODES[mode]}
    return [name for name, _ in case["launches"] if name not in off]


def arm_launches(names):
    """The arm entry points among the logged library calls, in issue order."""
    return [n for n in names if n in ARMS]


def lower_thresholds(eng):
    """Launch-size thresholds only: a four-frame step then takes the arms its shapes fit.  The shape predicates (the
    library's *_ok queries, _cs_max_waste, _wh_max_tiles) stay as shipped."""
    eng._dh_min_wgs = eng._cs_min_wgs = 1
    eng._wr_min_blocks = 1
    eng._wh_min_steps = eng._wf_min_steps = 1


def switch_off(eng, mode):
    for s in MODES[mode]:
        assert getattr(eng, s) is True, s
        setattr(eng, s, False)


def inputs(case):
    """item [B, 2, T, C, H, W] in [0, 1) and U [2, B*T, L], from the case's own generator."""
    g = torch.Generator().manual_seed(case["data_seed"])
    item = torch.rand(B, 2, T, case["in_ch"], *case["hw"], generator=g)
    U = torch.rand(2, B * T, LATENT, generator=g)
    return item, U


def site_maps(case):
    """(channels, h, w) of the four dropout / ReLU sites: conv1, conv2, deconv0, deconv1 outputs."""
    from rbvae_oracle import VARIANTS
    c1, c2, _ = VARIANTS[case["variant"]].channels
    H, W = case["hw"]
    return [(c1, H // 2, W // 2), (c2, H // 4, W // 4), (c2, H // 4, W // 4), (c1, H // 2, W // 2)]


def rows_to_oracle(rows, n_seq, h, w):
    """NHWC rows [2 * n_seq * h * w, C] of the engine (frames ordered (view, item, state)) -> the oracle's two per-view
    tensors [n_seq, C, h, w]."""
    rows = torch.as_tensor(rows)
    t = rows.reshape(2, n_seq, h, w, rows.shape[-1]).permute(0, 1, 4, 2, 3)
    return t[0], t[1]


def keyed_masks(case, key, counter):
    """The keep-masks a keyed-dropout step draws: site k = 1 .. 4 hashes (key * 8 + k, counter, element index of the NHWC
    output).  Returns (rows [site] bool [N*h*w, C], oracle [view][site] float [B*T, C, h, w])."""
    from rbvae_oracle import VARIANTS
    p = VARIANTS[case["variant"]].dropout
    rows, orc = [], [[], []]
    for k, (c, h, w) in enumerate(site_maps(case), start=1):
        keep = keyed_keep_mask(2 * B * T * h * w, c, key * 8 + k, p, seed_dev=counter)
        rows.append(torch.from_numpy(keep))
        v0, v1 = rows_to_oracle(keep, B * T, h, w)
        orc[0].append(v0.float())
        orc[1].append(v1.float())
    return rows, orc


def rel_l2(got, ref):
    got, ref = got.double().reshape(-1), ref.double().reshape(-1)
    return float((got - ref).norm()) / max(float(ref.norm()), 1e-12)


def worst_rel_l2(got, ref):
    """(tensor name, relative L2) of the worst tensor of two dicts with the same keys."""
    return max(((k, rel_l2(got[k], ref[k])) for k in ref), key=lambda t: t[1])


def oracle_step(variant, w0, item, U, dtype, train, masks=None, gates=None, want_pre=False, grads=True):
    """One oracle step in `dtype` from the f32 weights w0: (losses as floats, gradients, pre-activations)."""
    import rbvae_oracle as O
    p = {k: v.to(dtype).requires_grad_(grads) for k, v in w0.items()}
    pre = [] if want_pre else None
    mk = None if masks is None else [[x.to(dtype) for x in mm] for mm in masks]
    with torch.set_grad_enabled(grads):
        res = O.step_losses(variant, p, item.to(dtype), [U[0].to(dtype), U[1].to(dtype)], TAU, NOISE_RATIO, BERNOULLI_P, ALPHA,
                            BETA, MARGIN, train=train, masks=mk, gates=gates, pre=pre)
        if grads:
            res["total"].backward()
    return ({k: float(v.detach()) for k, v in res.items()}, {k: v.grad for k, v in p.items()} if grads else None, pre)


# ---- the sensitivity table: what each gate of the GPU file can see ---------------------------------------------------------

class TraceF:
    """Stands in for rbvae_oracle.F during one oracle step: every convolution's input and, after backward(), the gradient
    of its output.  calls[6 * view + j]: conv1, conv2, conv3, deconv0, deconv1, deconv2 of that view."""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        return getattr(self._real, name)

    def _traced(self, fn, x, w, b, **kw):
        out = fn(x, w, b, **kw)
        rec = {"x": x.detach()}
        out.register_hook(lambda g, rec=rec: rec.__setitem__("dy", g.detach()))
        self.calls.append(rec)
        return out

    def conv2d(self, x, w, b, **kw):
        return self._traced(self._real.conv2d, x, w, b, **kw)

    def conv_transpose2d(self, x, w, b, **kw):
        return self._traced(self._real.conv_transpose2d, x, w, b, **kw)


def conv_wgrad(x, dy, skip=None):
    """Weight gradient [Co, Ci, 3, 3] of a 3x3 stride-2 pad-1 convolution, tap by tap.  skip(ky, kx) -> None, or a 0/1
    tensor broadcastable to [N, 1, OH, OW]: the output pixels whose contribution to that tap a defect leaves out."""
    N, Co, OH, OW = dy.shape
    xp = torch.nn.functional.pad(x, (1, 1, 1, 1))
    g = x.new_zeros(Co, x.shape[1], 3, 3)
    for ky in range(3):
        for kx in range(3):
            patch = xp[:, :, ky:ky + 2 * OH:2, kx:kx + 2 * OW:2]
            d = dy
            drop = skip(ky, kx) if skip is not None else None
            if drop is not None:
                d = dy * (1 - drop)
            g[:, :, ky, kx] = torch.einsum("nohw,nihw->oi", d, patch)
    return g


CONV1_W, CONV1_B, CONV2_W, DECONV1_W = ("encoder_cnn.conv.0.weight", "encoder_cnn.conv.0.bias", "encoder_cnn.conv.3.weight",
                                        "decoder_cnn.deconv.3.weight")

# defect -> (tensor it moves, is it a weight-gradient defect, the gate that must see it): "matched" = item 3's 1.5e-2
# against the oracle; "reorder" = item 4's 2e-5 between the arms-on run and the run with the weight-gradient arms off
# (weight gradients only).  Measured at the reduced case (percep, 4 x 16 x 24, f64), in this order: 2.0e-1, 1.8e-1, 9.7e-1,
# 9.5e-2 -- all four are above 1.5e-2, so the oracle gate alone catches each; none is left to the 2e-5 gate, none is invisible.
DEFECTS = {
    "conv2_border_tap_last_column": (CONV2_W, True, "matched"),
    "bias_last_tile_rows": (CONV1_B, False, "matched"),
    "deconv1_transposed_taps": (DECONV1_W, True, "matched"),
    "conv1_last_frame": (CONV1_W, True, "matched"),
}


def defective(name, clean, trace, n_seq):
    """The gradient tensor DEFECTS[name] moves, derived with that one defect from the traced oracle step."""
    if name == "conv2_border_tap_last_column":
        # the tap kx = 2 of the last output column reads the last input column (2 (OW - 1) + 1 = IW - 1): dropped, as a
        # kernel would that took it for padding
        def skip(ky, kx):
            if kx != 2:
                return None
            OW = trace.calls[1]["dy"].shape[-1]
            m = torch.zeros(1, 1, 1, OW, dtype=clean[CONV2_W].dtype)
            m[..., OW - 1] = 1
            return m
        return sum(conv_wgrad(trace.calls[6 * v + 1]["x"], trace.calls[6 * v + 1]["dy"], skip) for v in range(2))
    if name == "bias_last_tile_rows":
        # conv1's bias gradient = the column sums of da1's NHWC rows, 128 per tile: the last tile's partial sums not reduced
        rows = torch.cat([trace.calls[6 * v]["dy"].permute(0, 2, 3, 1).reshape(-1, clean[CONV1_B].shape[0]) for v in range(2)])
        assert rows.shape[0] % 128 == 0 and rows.shape[0] > 128
        return rows[:-128].sum(0)
    if name == "deconv1_transposed_taps":
        return clean[DECONV1_W].transpose(-1, -2).contiguous()
    if name == "conv1_last_frame":
        # the last of the 2 * n_seq frames (view 1, last item, last state) never reaches the sum
        return (conv_wgrad(trace.calls[0]["x"], trace.calls[0]["dy"])
                + conv_wgrad(trace.calls[6]["x"][:n_seq - 1], trace.calls[6]["dy"][:n_seq - 1]))
    raise KeyError(name)


def caught_by(err, weight_gradient):
    """Which gate of the GPU file sees a defect of relative L2 `err`, or None."""
    if err > GRAD_MATCHED:
        return "matched"
    if weight_gradient and err > REORDER:
        return "reorder"
    return None
