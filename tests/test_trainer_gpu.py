"""The fused training step against the oracle's step + Adam (dropout off so both see the same network)."""
import numpy as np
import pytest
import torch

import rbvae_oracle as O

pytestmark = pytest.mark.gpu


def _oracle_step(variant, params, item, U, tau, r, p, alpha, beta, margin, steps, lr=1e-3):
    state = {}
    hist = []
    for st in range(1, steps + 1):
        for v in params.values():
            v.grad = None
        res = O.step_losses(variant, params, item, U, tau, r, p, alpha, beta, margin)
        res["total"].backward()
        hist.append({k: float(v) for k, v in res.items()})
        grads = {k: v.grad.clone() for k, v in params.items()}
        with torch.no_grad():
            O.adam_step({k: v for k, v in params.items()}, grads, state, lr, st)
    return hist, grads


@pytest.mark.parametrize("variant,use_graph", [("percep", False), ("percep", True), ("triplet", False)])
def test_fused_step_matches_oracle(variant, use_graph):
    import sfv_amd as sfv
    from importlib import import_module
    FusedTrainer = import_module("symbols-from-video_amd.trainer").FusedTrainer
    in_ch = 4 if variant == "percep" else 3
    B, T, Ld, hw = 3, 4, 32, (16, 24)
    torch.manual_seed(5)
    m = sfv.Seq2SeqBinaryVAE(in_ch, in_ch, Ld, Ld, variant=variant, input_hw=hw, compute_dtype="f32")
    params = {k: v.clone().requires_grad_() for k, v in m.state_dict().items()}
    m = m.cuda().eval()                                   # eval: no dropout on either side
    g = torch.Generator().manual_seed(6)
    item = torch.rand(B, 2, T, in_ch, *hw, generator=g)
    U = torch.rand(2, B * T, Ld, generator=g)
    tau, r, p, alpha, beta, margin = 0.8, 0.1, 0.1, 1.0, 0.5, 0.2
    steps = 3
    hist, last_grads = _oracle_step(variant, params, item, [U[0], U[1]], tau, r, p, alpha, beta, margin, steps)
    tr = FusedTrainer(m, lr=1e-3, alpha=alpha, beta_kl=beta, bernoulli_p=p, noise_ratio=r, margin=margin,
                      device_noise=False, use_graph=use_graph)
    for st in range(steps):
        losses = tr.step(item.cuda(), tau, U=U.cuda()).cpu().tolist()
        ref = hist[st]
        for got, k in zip(losses, ("total", "recon", "kl", "pair")):
            assert abs(got - ref[k]) < 2e-4 * max(1.0, abs(ref[k])), (st, k, got, ref[k])
    # gradients of the last step and the parameters after `steps` Adam updates
    lay = tr.eng.layout
    for k in lay.names:
        gr = lay.view(tr.gflat, k).cpu().double().reshape(-1)
        rf = last_grads[k].double().reshape(-1)
        assert float((gr - rf).norm()) <= 2e-3 * max(float(rf.norm()), 1e-7), k
    sd = m.state_dict()
    worst = max(float((sd[k].cpu() - params[k].detach()).abs().max()) for k in lay.names)
    assert worst < 5e-4, worst                      # 3 Adam steps of lr 1e-3 move a weight by <= 3e-3


def test_step_rejects_bad_input():
    import sfv_amd as sfv
    from importlib import import_module
    FusedTrainer = import_module("symbols-from-video_amd.trainer").FusedTrainer
    m = sfv.Seq2SeqBinaryVAE(4, 4, 32, 32, variant="percep", input_hw=(16, 16)).cuda()
    tr = FusedTrainer(m)
    with pytest.raises(ValueError):
        tr.step(torch.zeros(2, 3, 4, 4, 16, 16, device="cuda"), 1.0)
    with pytest.raises(ZeroDivisionError):
        tr.step(torch.zeros(2, 2, 1, 4, 16, 16, device="cuda"), 1.0)
    with pytest.raises(ValueError):
        FusedTrainer(sfv.Seq2SeqBinaryVAE(3, 3, 16, 16, variant="simple").cuda())


def test_input_buffer_is_read_in_place():
    """A batch written into trainer.input_buffer() and passed back to step() gives the same losses and weights as
    the same batch passed as a separate tensor (which step() copies into that buffer)."""
    import sfv_amd as sfv
    from importlib import import_module
    FusedTrainer = import_module("symbols-from-video_amd.trainer").FusedTrainer
    B, T, Ld, hw = 2, 3, 32, (16, 16)
    g = torch.Generator().manual_seed(9)
    item = torch.rand(B, 2, T, 4, *hw, generator=g).cuda()
    U = torch.rand(2, B * T, Ld, generator=g).cuda()
    res = []
    for in_place in (False, True):
        torch.manual_seed(8)
        m = sfv.Seq2SeqBinaryVAE(4, 4, Ld, Ld, variant="percep", input_hw=hw, compute_dtype="f32").cuda().eval()
        tr = FusedTrainer(m, device_noise=False, use_graph=True)
        x = item
        if in_place:
            x = tr.input_buffer(B, T, 4, *hw)
            x.copy_(item)
        for _ in range(2):
            losses = tr.step(x, 0.9, U=U).clone()
        res.append((losses, m._flat.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


# The reference's own sweeps: latent_dim 25 / 50 / 75 / 100, T = 5 / 9 / 17 states, batches of
# odd size, native 88x160 frames whose 11x20 bottleneck is not a power of two.  One fused step (exact-f32 mode,
# eval: no dropout on either side) against the oracle's step: losses 2e-4, gradients 2e-3 relative L2.
@pytest.mark.parametrize("variant,in_ch,B,T,Ld,hw", [
    ("percep", 4, 3, 5, 25, (24, 40)),
    ("percep", 4, 1, 9, 50, (16, 16)),
    ("percep", 4, 2, 17, 100, (8, 16)),
    ("percep", 4, 1, 2, 75, (88, 160)),
    ("contrastive", 3, 2, 5, 50, (32, 24)),
    ("triplet", 3, 3, 9, 16, (16, 16)),
])
def test_fused_step_parameter_ranges(variant, in_ch, B, T, Ld, hw):
    import sfv_amd as sfv
    from importlib import import_module
    FusedTrainer = import_module("symbols-from-video_amd.trainer").FusedTrainer
    torch.manual_seed(21)
    m = sfv.Seq2SeqBinaryVAE(in_ch, in_ch, Ld, Ld, variant=variant, input_hw=hw, compute_dtype="f32")
    params = {k: v.clone().requires_grad_() for k, v in m.state_dict().items()}
    m = m.cuda().eval()
    g = torch.Generator().manual_seed(22)
    item = torch.rand(B, 2, T, in_ch, *hw, generator=g)
    U = torch.rand(2, B * T, Ld, generator=g)
    tau, r, p, alpha, beta, margin = 0.6, 0.3, 0.1, 0.7, 0.4, 0.2
    hist, grads = _oracle_step(variant, params, item, [U[0], U[1]], tau, r, p, alpha, beta, margin, 1)
    tr = FusedTrainer(m, lr=1e-3, alpha=alpha, beta_kl=beta, bernoulli_p=p, noise_ratio=r, margin=margin,
                      device_noise=False, use_graph=False)
    losses = tr.step(item.cuda(), tau, U=U.cuda()).cpu().tolist()
    for got, k in zip(losses, ("total", "recon", "kl", "pair")):
        assert abs(got - hist[0][k]) < 2e-4 * max(1.0, abs(hist[0][k])), (k, got, hist[0][k])
    lay = tr.eng.layout
    for k in lay.names:
        gr = lay.view(tr.gflat, k).cpu().double().reshape(-1)
        rf = grads[k].double().reshape(-1)
        assert float((gr - rf).norm()) <= 2e-3 * max(float(rf.norm()), 1e-7), k


def _long_sequence_cases():
    """Latent 32 with the percep variant's 4 LSTM layers: T = the first sequence length the backward wavefront kernel
    refuses (the encoder's fused binarise backward, the cast copy and the slab sums have to fall back), and a T where
    only the two-stack backward launch is refused -- both from the restated dispatch of tests/_lstm_cases.py.  16 x 16
    frames are the smallest the model takes; 16 x 32 is the smallest whose fc layers run K-split (F3 = 2048)."""
    import _lstm_cases as C
    T_wave, T_pair = C.T_BWD_32x4, C.T_PAIR_BWD_32x4
    assert C.bwd_dispatch(T_wave, 32, 4) == "lstm_bwd_k<32>" and C.bwd_dispatch(T_wave - 1, 32, 4).startswith("lstm_bwd_wave_k")
    assert not C.pair_bwd_ok(T_pair, 32, 4) and C.bwd_wave_ok(T_pair, 32, 4) and C.pair_bwd_ok(T_pair - 1, 32, 4)
    T_fwd = C.T_FWD_32x4                       # ... and the first T the forward wavefront kernel refuses
    assert C.fwd_dispatch(T_fwd, 32, 4) == "lstm_fwd_k<32>" and C.fwd_dispatch(T_fwd - 1, 32, 4).startswith("lstm_fwd_wave_k")
    return [(T_wave, (16, 16)), (T_pair, (16, 16)), (T_wave, (16, 32)), (T_fwd, (16, 32))]


@pytest.mark.parametrize("T,hw", _long_sequence_cases())
def test_fused_step_long_sequences(T, hw):
    """The engine chooses the LSTM launches per call from the queries the C dispatchers use themselves
    (rbvae_lstm_*_wave_ok, rbvae_lstm_pair_*_ok): a sequence too long for the wavefront kernels runs on the plain kernels
    + rbvae_binarize_kl_bwd + rbvae_cast_pad + the unsplit fc instead of raising.  Same tolerances as
    test_fused_step_parameter_ranges."""
    test_fused_step_parameter_ranges("percep", 4, 1, T, 32, hw)
    import sfv_amd as sfv
    assert not sfv._lib.query("rbvae_lstm_pair_bwd_ok", T, 32, 4)


@pytest.mark.parametrize("Ld,T,hw", [(50, 5, (32, 32)), (100, 8, (32, 32)), (25, 4, (16, 16))])
def test_bf16_step_tracks_f32_step_at_other_latents(Ld, T, hw):
    """bf16 storage at the reference's other latent sizes (layer-by-layer LSTM kernels above 32, the K = 64 / 128 fc
    products through rbvae_fc_gemm, padded codes): one step against the exact-f32 engine fed the same noise -- losses
    within 1e-2, every gradient tensor within 8e-2 relative L2: measured 4.6-4.7e-2 at every size, the well-trodden L = 25
    included (bf16 rounding of activations plus ReLU decisions that differ between the two runs near zero -- with the
    decisions matched it is 5e-3, test_bench_shape_step_against_oracle); wiring errors are O(1)."""
    import sfv_amd as sfv
    from importlib import import_module
    FusedTrainer = import_module("symbols-from-video_amd.trainer").FusedTrainer
    B = 4
    g = torch.Generator().manual_seed(61 + Ld)
    item = torch.rand(B, 2, T, 4, *hw, generator=g).cuda()
    U = torch.rand(2, B * T, Ld, generator=g).cuda()
    out = {}
    for dt in ("f32", "bf16"):
        torch.manual_seed(60)
        m = sfv.Seq2SeqBinaryVAE(4, 4, Ld, Ld, variant="percep", input_hw=hw, compute_dtype=dt).cuda().eval()
        tr = FusedTrainer(m, lr=1e-3, alpha=1.0, beta_kl=1.0, bernoulli_p=0.1, noise_ratio=0.1, device_noise=False,
                          use_graph=False)
        losses = tr.step(item, 0.7, U=U).cpu()
        lay = tr.eng.layout
        out[dt] = (losses, {k: lay.view(tr.gflat, k).detach().cpu().double().reshape(-1).clone() for k in lay.names})
    lf, lb = out["f32"][0], out["bf16"][0]
    assert torch.isfinite(lb).all() and float(((lf - lb).abs() / lf.abs().clamp_min(1.0)).max()) < 1e-2, (lf, lb)
    worst = max((float((out["bf16"][1][k] - v).norm() / max(float(v.norm()), 1e-12)), k) for k, v in out["f32"][1].items())
    assert worst[0] < 8e-2, worst


def test_bf16_graph_steps_track_f32_steps():
    """The bench configuration in small: bf16 storage, dropout on, device-side noise, HIP-graph replay.  Twenty
    steps must keep the loss finite, close to the exact-f32 trainer fed the same noise-free setting, and going down."""
    import sfv_amd as sfv
    from importlib import import_module
    FusedTrainer = import_module("symbols-from-video_amd.trainer").FusedTrainer
    B, T, Ld, hw = 4, 8, 32, (32, 32)
    g = torch.Generator().manual_seed(31)
    item = torch.randn(B, 2, T, 4, *hw, generator=g).cuda()
    U = torch.rand(2, B * T, Ld, generator=g).cuda()
    curves = {}
    for dt in ("f32", "bf16"):
        torch.manual_seed(30)
        m = sfv.Seq2SeqBinaryVAE(4, 4, Ld, Ld, variant="percep", input_hw=hw, compute_dtype=dt).cuda().eval()
        tr = FusedTrainer(m, lr=1e-3, alpha=1.0, beta_kl=1.0, bernoulli_p=0.1, noise_ratio=0.1, device_noise=False,
                          use_graph=True)
        curves[dt] = [tr.step(item, 0.7, U=U)[0].item() for _ in range(20)]
    f, b = curves["f32"], curves["bf16"]
    assert all(np.isfinite(b)) and b[-1] < b[0]
    assert max(abs(x - y) / abs(x) for x, y in zip(f, b)) < 2e-2, (f[-1], b[-1])


# ---- round 2: schedule through device scalars, checkpoint state, validation, per-rank noise, bench shape ----------
def _mk(variant="percep", in_ch=4, Ld=32, hw=(16, 16), dtype="f32", seed=40, train=False):
    import sfv_amd as sfv
    torch.manual_seed(seed)
    m = sfv.Seq2SeqBinaryVAE(in_ch, in_ch, Ld, Ld, variant=variant, input_hw=hw, compute_dtype=dtype)
    params = {k: v.clone().requires_grad_() for k, v in m.state_dict().items()}
    m = m.cuda()
    m.train(train)
    return m, params


def _FT():
    from importlib import import_module
    return import_module("symbols-from-video_amd.trainer").FusedTrainer


def test_annealed_run_uses_one_graph_and_matches_eager():
    """percep_RBVAE_train.py:424-437: the temperature changes during a run.  It reaches the kernels through a device
    scalar, so the captured graph is reused: one graph for the whole schedule, bit-identical to the eager path."""
    B, T, Ld, hw = 2, 4, 32, (16, 16)
    g = torch.Generator().manual_seed(41)
    item = torch.rand(B, 2, T, 4, *hw, generator=g).cuda()
    U = torch.rand(2, B * T, Ld, generator=g).cuda()
    taus = [1.0, 1.0, 0.83, 0.83, 0.61, 0.5, 0.5]
    res = {}
    for use_graph in (False, True):
        m, _ = _mk(hw=hw)
        tr = _FT()(m, lr=1e-3, alpha=1.0, beta_kl=0.5, bernoulli_p=0.1, device_noise=False, use_graph=use_graph)
        hist = []
        for i, tau in enumerate(taus):
            if i == 4:
                tr.lr = 5e-4                       # an lr schedule step travels the same way
            hist.append(tr.step(item, tau, U=U).clone())
        res[use_graph] = (torch.stack(hist), m._flat.clone())
        if use_graph:
            assert len(tr._graphs) == 1
    assert torch.equal(res[False][0], res[True][0]) and torch.equal(res[False][1], res[True][1])
    # and the schedule really acted: the same run at constant tau ends elsewhere
    m, _ = _mk(hw=hw)
    tr = _FT()(m, lr=1e-3, alpha=1.0, beta_kl=0.5, bernoulli_p=0.1, device_noise=False, use_graph=True)
    for _ in taus:
        tr.step(item, 1.0, U=U)
    assert not torch.equal(m._flat, res[True][1])


def test_anneal_matches_oracle_schedule():
    """Three optimiser steps at three temperatures against the oracle's steps (graph path)."""
    B, T, Ld, hw = 2, 3, 32, (16, 16)
    m, params = _mk(hw=hw, seed=42)
    g = torch.Generator().manual_seed(43)
    item = torch.rand(B, 2, T, 4, *hw, generator=g)
    U = torch.rand(2, B * T, Ld, generator=g)
    tr = _FT()(m, lr=1e-3, alpha=1.0, beta_kl=1.0, bernoulli_p=0.1, noise_ratio=0.1, device_noise=False, use_graph=True)
    state = {}
    for st, tau in enumerate((1.0, 0.7, 0.4), 1):
        for v in params.values():
            v.grad = None
        ref = O.step_losses("percep", params, item, [U[0], U[1]], tau, 0.1, 0.1, 1.0, 1.0)
        ref["total"].backward()
        with torch.no_grad():
            O.adam_step(dict(params), {k: v.grad for k, v in params.items()}, state, 1e-3, st)
        got = tr.step(item.cuda(), tau, U=U.cuda()).cpu().tolist()
        for x, k in zip(got, ("total", "recon", "kl", "pair")):
            assert abs(x - float(ref[k])) < 2e-4 * max(1.0, abs(float(ref[k]))), (st, k, x, float(ref[k]))
    assert len(tr._graphs) == 1


def test_trainer_state_dict_is_torch_adam_format_and_round_trips():
    """percep_RBVAE_train.py:691-702 stores optimizer.state_dict(): the fused trainer's state loads into a real
    torch.optim.Adam over the model's parameters (same next update), and back into a fresh trainer (same next step)."""
    B, T, Ld, hw = 2, 3, 32, (16, 16)
    g = torch.Generator().manual_seed(44)
    item = torch.rand(B, 2, T, 4, *hw, generator=g).cuda()
    U = torch.rand(2, B * T, Ld, generator=g).cuda()
    m, _ = _mk(hw=hw, seed=45)
    tr = _FT()(m, lr=2e-3, device_noise=False, use_graph=False, seed=77)
    assert tr.state_dict()["optimizer_state_dict"]["state"] == {}          # torch: no state before the first step
    for _ in range(3):
        tr.step(item, 0.8, U=U)
    sd = tr.state_dict()
    msd = {k: v.clone() for k, v in m.state_dict().items()}
    osd = sd["optimizer_state_dict"]
    assert set(osd) == {"state", "param_groups"} and len(osd["state"]) == len(list(m.parameters()))
    assert float(osd["state"][0]["step"]) == 3.0 and osd["param_groups"][0]["lr"] == 2e-3
    # (a) a real torch Adam continues from it exactly like the fused optimiser does
    tr.step(item, 0.8, U=U)
    after_fused = m._flat.clone()
    grads = tr.gflat.clone()
    m2, _ = _mk(hw=hw, seed=45)
    m2.load_state_dict(msd)
    opt = torch.optim.Adam(m2.parameters(), lr=1e-3)
    import copy
    opt.load_state_dict(copy.deepcopy(osd))         # torch keeps the given tensors and updates them in place
    assert opt.param_groups[0]["lr"] == 2e-3
    lay = m2._layout
    for n, p in zip(lay.names, m2.parameters()):
        p.grad = lay.view(grads, n).clone()
    opt.step()
    assert float((m2._flat - after_fused).abs().max()) < 1e-6
    # (b) a fresh trainer resumes bit-identically (weights + moments + step + noise seed)
    m3, _ = _mk(hw=hw, seed=46)
    m3.load_state_dict(msd)
    tr3 = _FT()(m3, lr=1e-3, device_noise=False, use_graph=False)
    tr3.load_state_dict(sd)
    assert tr3.seed == 77 and tr3.lr == 2e-3
    tr3.step(item, 0.8, U=U)
    assert torch.equal(m3._flat, after_fused)
    with pytest.raises(ValueError):
        bad = {"state": {}, "param_groups": [dict(osd["param_groups"][0], weight_decay=0.1)]}
        tr3.load_state_dict(bad)


@pytest.mark.parametrize("variant,pair_loss", [("percep", None), ("triplet", None), ("percep", "triplet")])
def test_validate_matches_oracle(variant, pair_loss):
    """percep_RBVAE_train.py:590-635: eval mode, hard codes at the final temperature, weights / (1 + alpha + beta)."""
    in_ch = 4 if variant == "percep" else 3
    B, T, Ld, hw = 3, 4, 32, (16, 24)
    m, params = _mk(variant, in_ch, Ld, hw, seed=47, train=True)          # validate() must ignore train mode
    g = torch.Generator().manual_seed(48)
    item = torch.rand(B, 2, T, in_ch, *hw, generator=g)
    U = torch.rand(2, B * T, Ld, generator=g)
    alpha, beta, p, r, margin, tau = 0.7, 0.4, 0.1, 0.3, 0.2, 0.3
    with torch.no_grad():
        ref = O.step_losses(variant, {k: v.detach() for k, v in params.items()}, item, [U[0], U[1]], tau, r, p, alpha,
                            beta, margin, hard=True, train=False, validation_norm=True, pair_loss=pair_loss)
    tr = _FT()(m, alpha=alpha, beta_kl=beta, bernoulli_p=p, noise_ratio=r, margin=margin, pair_loss=pair_loss)
    flat0 = m._flat.clone()
    got = tr.validate(item.cuda(), tau, U=U.cuda()).cpu().tolist()
    for x, k in zip(got, ("total", "recon", "kl", "pair")):
        assert abs(x - float(ref[k])) < 1e-4 * max(1.0, abs(float(ref[k]))), (k, x, float(ref[k]))
    assert torch.equal(flat0, m._flat) and int(tr.step_dev.item()) == 0


def test_pair_loss_is_independent_of_the_conv_widths():
    """BASELINE configs[4]: the percep-shaped network (256 channels, 4-layer LSTMs) trained with the triplet term
    (triplet_RBVAE_train.py:461-468): one fused step against the oracle's."""
    B, T, Ld, hw = 2, 4, 32, (16, 16)
    m, params = _mk("percep", 4, Ld, hw, seed=49)
    g = torch.Generator().manual_seed(50)
    item = torch.rand(B, 2, T, 4, *hw, generator=g)
    U = torch.rand(2, B * T, Ld, generator=g)
    ref = O.step_losses("percep", params, item, [U[0], U[1]], 0.7, 0.1, 0.1, 0.9, 0.6, 0.2, pair_loss="triplet")
    ref["total"].backward()
    tr = _FT()(m, alpha=0.9, beta_kl=0.6, bernoulli_p=0.1, noise_ratio=0.1, margin=0.2, device_noise=False,
               use_graph=False, pair_loss="triplet")
    got = tr.step(item.cuda(), 0.7, U=U.cuda()).cpu().tolist()
    for x, k in zip(got, ("total", "recon", "kl", "pair")):
        assert abs(x - float(ref[k])) < 1e-4 * max(1.0, abs(float(ref[k]))), (k, x, float(ref[k]))
    lay = tr.eng.layout
    for k in lay.names:
        gr = lay.view(tr.gflat, k).cpu().double().reshape(-1)
        rf = params[k].grad.double().reshape(-1)
        assert float((gr - rf).norm()) <= 1e-3 * max(float(rf.norm()), 1e-7), k
    with pytest.raises(ValueError):
        _FT()(m, pair_loss="cosine")


def test_ranks_and_seeds_draw_different_noise():
    """every data-parallel rank draws its own dropout masks and Binary-Concrete noise; a seed reproduces."""
    from importlib import import_module
    T_ = import_module("symbols-from-video_amd.trainer")
    B, T, Ld, hw = 2, 4, 32, (16, 16)
    g = torch.Generator().manual_seed(51)
    item = torch.rand(B, 2, T, 4, *hw, generator=g).cuda()

    def run(seed, rank):
        m, _ = _mk(hw=hw, seed=52, train=True)
        tr = T_.FusedTrainer(m, device_noise=True, use_graph=False, seed=seed)
        tr.rank = rank
        tr._noise_key = T_.noise_key(tr.seed, rank)
        return tr.step(item, 0.7).clone()

    a, a2, b, c = run(5, 0), run(5, 0), run(5, 1), run(6, 0)
    assert torch.equal(a, a2)
    assert not torch.equal(a, b) and not torch.equal(a, c) and not torch.equal(b, c)
    torch.manual_seed(9)
    m, _ = _mk(hw=hw, seed=52)
    torch.manual_seed(1234)
    assert T_.FusedTrainer(m).seed == 1234                      # default: torch.initial_seed()


def _bench_case(seed):
    B, T, Ld, hw = 16, 8, 32, (32, 32)
    g = torch.Generator().manual_seed(seed)
    item = torch.randn(B, 2, T, 4, *hw, generator=g)
    U = torch.rand(2, B * T, Ld, generator=g)
    v = O.VARIANTS["percep"]
    shapes = [(256, 16, 16), (256, 8, 8), (256, 8, 8), (256, 16, 16)]
    masks = [[(torch.rand(B * T, *s, generator=g) >= v.dropout).float() for s in shapes] for _ in range(2)]
    return B, T, Ld, hw, item, U, masks


from importlib import import_module as _imp  # noqa: E402
_gmod = _imp("symbols-from-video_amd._gates")
_device_gates, _count_ties = _gmod.device_gates, _gmod.count_ties


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_bench_shape_step_against_oracle(dtype):
    """The exact bench workload (BASELINE configs[1]: item [16,2,8,4,32,32], latent 32, tau 0.7, r 0.1, p 0.1,
    alpha = beta = 1, dropout ON through explicit masks, explicit U): one fused step against the oracle's step (run in
    f64) + Adam.  Losses are compared with the plain oracle.  For the gradients the oracle is given the device's own
    ReLU decisions: 33.6 M pre-activations pass through a ReLU per step, a handful of them lie within f32 rounding of
    zero, and ONE such tie resolved the other way moves the first conv's weight gradient (norm 2e-4, the sum of 16.7 M
    cancelling terms) by 2.4e-4 relative -- measured: 3.6e-4 / 5.5e-4 with 1-3 ties.  The test asserts that the
    device's decisions differ from sign(oracle pre-activation) only within rounding of zero, and then gates every
    gradient tensor: f32 5e-5 relative L2 (north_star asks 1e-4), bf16 (the benched mode) 1.5e-2 -- direction, not just norm."""
    B, T, Ld, hw, item, U, masks = _bench_case(60)
    m, params = _mk("percep", 4, Ld, hw, dtype=dtype, seed=61, train=True)
    tr = _FT()(m, lr=1e-3, alpha=1.0, beta_kl=1.0, bernoulli_p=0.1, noise_ratio=0.1, device_noise=False, use_graph=False)
    w0 = {k: v.detach().clone() for k, v in params.items()}
    got = tr.step(item.cuda(), 0.7, U=U.cuda(), dropout_masks=masks).cpu().tolist()
    gates = _device_gates(tr, B, T)
    # losses: plain oracle, f32, no knowledge of the device
    with torch.no_grad():
        ref = O.step_losses("percep", w0, item, [U[0], U[1]], 0.7, 0.1, 0.1, 1.0, 1.0, train=True, masks=masks)
    ltol = 1e-4 if dtype == "f32" else 1e-2
    for x, k in zip(got, ("total", "recon", "kl", "pair")):
        assert abs(x - float(ref[k])) < ltol * max(1.0, abs(float(ref[k]))), (k, x, float(ref[k]))
    # gradients: f64 oracle with the device's ReLU decisions
    p64 = {k: v.double().requires_grad_() for k, v in w0.items()}
    pre = []
    r64 = O.step_losses("percep", p64, item.double(), [U[0].double(), U[1].double()], 0.7, 0.1, 0.1, 1.0, 1.0, train=True,
                        masks=[[x.double() for x in mm] for mm in masks], gates=gates, pre=pre)
    r64["total"].backward()
    ties = _count_ties(pre, gates, masks, 2e-5 if dtype == "f32" else 0.1)
    n_act = sum(int((mm[j] > 0).sum()) for mm in masks for j in range(4))
    # how many decisions differ: a handful in f32; in bf16 (pre-activations rounded to 8 bits) at most 0.1 % of the live ones
    assert ties <= (20 if dtype == "f32" else 1e-3 * n_act), (ties, n_act)
    # the UNCONDITIONED figure beside it: the same f64 oracle WITHOUT the device's decisions (loose by construction: every
    # tie moves a small-norm tensor by ~1/sqrt(#terms)); a gating bug cannot hide behind the gates
    pu = {k: v.double().requires_grad_() for k, v in w0.items()}
    O.step_losses("percep", pu, item.double(), [U[0].double(), U[1].double()], 0.7, 0.1, 0.1, 1.0, 1.0, train=True,
                  masks=[[x.double() for x in mm] for mm in masks])["total"].backward()
    lay = tr.eng.layout
    worst = ("", 0.0)
    for k in lay.names:
        gr = lay.view(tr.gflat, k).cpu().double().reshape(-1)
        rf = p64[k].grad.reshape(-1)
        e = float((gr - rf).norm()) / max(float(rf.norm()), 1e-12)
        worst = max(worst, (k, e), key=lambda t: t[1])
    worst_u = ("", 0.0)
    for k in lay.names:
        gr = lay.view(tr.gflat, k).cpu().double().reshape(-1)
        rf = pu[k].grad.reshape(-1)
        worst_u = max(worst_u, (k, float((gr - rf).norm()) / max(float(rf.norm()), 1e-12)), key=lambda t: t[1])
    print(f"bench shape {dtype}: {ties} ReLU ties of {n_act} live activations ({100.0 * ties / n_act:.4f} %); worst gradient "
          f"rel-L2 {worst[1]:.2e} ({worst[0]}) under the device's decisions, {worst_u[1]:.2e} ({worst_u[0]}) unconditioned")
    assert worst[1] < (5e-5 if dtype == "f32" else 1.5e-2), worst        # measured: 5.2e-6 / 4.9e-3
    assert worst_u[1] < (2e-3 if dtype == "f32" else 0.15), worst_u      # measured round 2: 5.5e-4 / 4.7e-2
    # the optimiser step: the oracle's Adam on the device's gradients lands on the device's weights (the first Adam
    # step is lr * g / (|g| + eps): on the oracle's own gradients every element smaller than the gradient error could
    # legitimately move the other way, so that comparison says nothing)
    with torch.no_grad():
        O.adam_step(w0, {k: lay.view(tr.gflat, k).cpu() for k in lay.names}, {}, 1e-3, 1)
    sd = m.state_dict()
    dw = max(float((sd[k].cpu() - w0[k]).abs().max()) for k in lay.names)
    assert dw < 1e-6, dw


def test_bench_shape_graph_replay_equals_eager_bf16():
    """The benched configuration itself -- bf16, dropout by counter hash, device-side noise, graph replay -- against the
    same trainer run eagerly: bit-identical losses and weights over 3 steps (so the graph runs the arithmetic the
    oracle-checked eager path runs)."""
    B, T, Ld, hw, item, _, _ = _bench_case(62)
    res = []
    for use_graph in (False, True):
        m, _ = _mk("percep", 4, Ld, hw, dtype="bf16", seed=63, train=True)
        tr = _FT()(m, lr=1e-3, alpha=1.0, beta_kl=1.0, bernoulli_p=0.1, noise_ratio=0.1, device_noise=True,
                   use_graph=use_graph, seed=3)
        ls = [tr.step(item.cuda(), 0.7).clone() for _ in range(3)]
        res.append((torch.stack(ls), m._flat.clone()))
    assert torch.isfinite(res[0][0]).all()
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_load_state_dict_drops_captured_graphs_and_reprimes():
    """betas / eps are by-value arguments of the captured launches -- a trainer that has already stepped from
    its graph and then loads an optimiser state with OTHER betas must step with them (equal to a fresh trainer given the
    same state), not replay the old graph."""
    B, T, Ld, hw = 2, 3, 32, (16, 16)
    g = torch.Generator().manual_seed(91)
    item = torch.rand(B, 2, T, 4, *hw, generator=g).cuda()
    U = torch.rand(2, B * T, Ld, generator=g).cuda()
    m, _ = _mk(hw=hw, seed=92)
    tr = _FT()(m, lr=1e-3, device_noise=False, use_graph=True, seed=5)
    for _ in range(3):
        tr.step(item, 0.8, U=U)
    assert tr._graphs
    sd = tr.state_dict()
    sd["optimizer_state_dict"]["param_groups"][0]["betas"] = (0.5, 0.9)
    sd["optimizer_state_dict"]["param_groups"][0]["eps"] = 1e-6
    msd = {k: v.clone() for k, v in m.state_dict().items()}
    tr.load_state_dict(sd["optimizer_state_dict"])            # a bare torch-format dict: no "seed" key
    assert not tr._graphs and tr.betas == (0.5, 0.9) and tr.eps == 1e-6
    tr.step(item, 0.8, U=U)
    m2, _ = _mk(hw=hw, seed=93)
    m2.load_state_dict(msd)
    tr2 = _FT()(m2, lr=1e-3, device_noise=False, use_graph=False, seed=5)
    tr2.load_state_dict(sd["optimizer_state_dict"])
    tr2.step(item, 0.8, U=U)
    assert torch.equal(m._flat, m2._flat)


@pytest.mark.parametrize("variant,in_ch,hw,item_shape", [("contrastive", 3, (64, 64), (2, 2, 4)), ("percep", 4, (32, 48), (2, 2, 4))])
def test_large_frame_weight_gradient_kernels_equal_the_gemm_path(variant, in_ch, hw, item_shape):
    """The engine switches three weight-gradient kernels in by size (rbvae_wgrad3x3s2_halo for the 3x3 layers of <= 2 channel
    tiles, rbvae_wgrad_first for the two 3/4-channel ends with the forward kernels' col = NULL): forced on at a small shape
    (thresholds lowered to one pixel block per workgroup) they must leave the gradients of the rbvae_wgrad_gemm path --
    the same bf16 products, f32 sums in another order -- and the same losses, from the same weights, batch, noise and
    dropout keys."""
    import sfv_amd as sfv
    from importlib import import_module
    FusedTrainer = import_module("symbols-from-video_amd.trainer").FusedTrainer
    B, V, T = item_shape
    g = torch.Generator().manual_seed(41)
    item = torch.rand(B, V, T, in_ch, *hw, generator=g).cuda()
    res = []
    for forced in (True, False):
        torch.manual_seed(40)
        m = sfv.Seq2SeqBinaryVAE(in_ch, in_ch, 32, 32, variant=variant, input_hw=hw, compute_dtype="bf16").cuda().train()
        tr = FusedTrainer(m, lr=1e-3, alpha=1.0, beta_kl=1.0, bernoulli_p=0.1, noise_ratio=0.1, device_noise=True, use_graph=False,
                          seed=77)
        eng = tr.eng = m._engine_for(item)            # the trainer adopts the model's engine at its first step
        eng.seed_dev = tr.step_dev
        if forced:
            eng._wf_min_steps = 1
            eng._wh_min_steps = 1
        else:
            eng.wgrad_first = False
            eng.wgrad_halo = False
        L = sfv._lib
        names, orig = [], L.call
        L.call = lambda name, *a: (names.append(name), orig(name, *a))[1]
        try:
            losses = tr.step(item, 0.7).cpu()
        finally:
            L.call = orig
        res.append((losses, tr.gflat.clone(), eng, names))
    (la, ga, ea, na), (lb, gb, eb, nb) = res
    assert na.count("rbvae_wgrad_first") == 2 and "rbvae_wgrad_first" not in nb
    assert ("rbvae_wgrad3x3s2_halo" in na) == (variant == "contrastive") and "rbvae_wgrad3x3s2_halo" not in nb
    assert torch.allclose(la, lb, rtol=1e-6, atol=1e-6), (la, lb)
    lay = ea.layout
    for k in lay.names:
        a, b = lay.view(ga, k).double().reshape(-1), lay.view(gb, k).double().reshape(-1)
        assert float((a - b).norm()) <= 2e-5 * max(float(b.norm()), 1e-9), k


def test_sixteen_fc_groups_equal_four():
    """The fc products on either side of the LSTM stacks run K-split over 4 workgroup groups, over 16 from 16 384 fc inputs up
    (native 4x88x160: 56 320, cfg 3: 65 536); the LSTM kernels sum the groups' slabs in order.  Sixteen groups forced at the
    bench shape (4096 inputs) leave the losses of four and its gradients up to the f32 summation order of the fc products and
    the bf16 roundings of the activations behind them that an f32 ulp flips (the first conv's weight gradient, a sum of
    millions of cancelling terms, moves by 1.6e-4 relative; gate 2e-3)."""
    import sfv_amd as sfv
    from importlib import import_module
    FusedTrainer = import_module("symbols-from-video_amd.trainer").FusedTrainer
    g = torch.Generator().manual_seed(43)
    item = torch.randn(4, 2, 8, 4, 32, 32, generator=g).cuda()
    res = []
    for groups in (16, 4):
        torch.manual_seed(42)
        m = sfv.Seq2SeqBinaryVAE(4, 4, 32, 32, variant="percep", input_hw=(32, 32), compute_dtype="bf16").cuda().train()
        tr = FusedTrainer(m, lr=1e-3, alpha=1.0, beta_kl=1.0, bernoulli_p=0.1, noise_ratio=0.1, device_noise=True, use_graph=False,
                          seed=78)
        eng = tr.eng = m._engine_for(item)
        eng.seed_dev = tr.step_dev
        assert eng.fc_split == 4 and eng.F3 == 4096
        eng.fc_split = groups
        res.append((tr.step(item, 0.7).cpu(), tr.gflat.clone(), eng.layout))
    (la, ga, lay), (lb, gb, _) = res
    assert torch.allclose(la, lb, rtol=2e-6, atol=2e-6), (la, lb)
    for k in lay.names:
        a, b = lay.view(ga, k).double().reshape(-1), lay.view(gb, k).double().reshape(-1)
        assert float((a - b).norm()) <= 2e-3 * max(float(b.norm()), 1e-9), k


def test_fc_groups_fall_back_to_eight_or_four_when_sixteen_does_not_divide():
    """F3 = 256 * (72 / 8) * (120 / 8) = 34 560 fc inputs (a 4 x 72 x 120 frame): a multiple of 128 (four K units of 32 per
    group fit) but not of 512, so sixteen groups do not divide it -- the engine takes the largest of 16 / 8 / 4 that does
    instead of dropping to ONE group on 32 CUs, and the step still matches the one-group step."""
    import sfv_amd as sfv
    from importlib import import_module
    FusedTrainer = import_module("symbols-from-video_amd.trainer").FusedTrainer
    g = torch.Generator().manual_seed(44)
    item = torch.randn(1, 2, 3, 4, 72, 120, generator=g).cuda()
    res = []
    for force_one in (False, True):
        torch.manual_seed(45)
        m = sfv.Seq2SeqBinaryVAE(4, 4, 32, 32, variant="percep", input_hw=(72, 120), compute_dtype="bf16").cuda().train()
        tr = FusedTrainer(m, lr=1e-3, device_noise=True, use_graph=False, seed=79)
        eng = tr.eng = m._engine_for(item)
        eng.seed_dev = tr.step_dev
        assert eng.F3 == 34560 and eng.fc_split in (8, 4) and eng.F3 % (eng.fc_split * 32) == 0
        if force_one:
            eng.fc_split = 1
        res.append((tr.step(item, 0.7).cpu(), tr.gflat.clone(), eng.layout))
    (la, ga, lay), (lb, gb, _) = res
    assert torch.allclose(la, lb, rtol=2e-5, atol=2e-5), (la, lb)
    for k in lay.names:
        a, b = lay.view(ga, k).double().reshape(-1), lay.view(gb, k).double().reshape(-1)
        assert float((a - b).norm()) <= 3e-3 * max(float(b.norm()), 1e-9), k


def test_step_is_bit_identical_with_either_lstm_wavefront_kernel():
    """The two LSTM launches of a step with one wave per layer (lstm_pair_fwd_unit_k / lstm_pair_bwd_unit_k, the default at
    latent_dim 32) and with one thread per gate row (rbvae_dbg_lstm_unit_threads(0)): three captured-graph steps from the same
    weights, batch, noise and dropout keys leave bit-identical losses, gradients and parameters."""
    import sfv_amd as sfv
    from importlib import import_module
    FusedTrainer = import_module("symbols-from-video_amd.trainer").FusedTrainer
    g = torch.Generator().manual_seed(43)
    item = torch.randn(4, 2, 8, 4, 32, 32, generator=g).cuda()
    dbg = sfv._lib.dbg_lib()
    res = []
    for unit in (1, 0):
        old = dbg.rbvae_dbg_lstm_unit_threads(unit)
        try:
            torch.manual_seed(44)
            m = sfv.Seq2SeqBinaryVAE(4, 4, 32, 32, variant="percep", input_hw=(32, 32), compute_dtype="bf16").cuda().train()
            tr = FusedTrainer(m, lr=1e-3, alpha=1.0, beta_kl=1.0, bernoulli_p=0.1, noise_ratio=0.1, device_noise=True,
                              use_graph=True, seed=78)
            hist = [tr.step(item, 0.7).clone() for _ in range(3)]
            torch.cuda.synchronize()
            res.append((torch.stack(hist).cpu(), tr.gflat.clone(), m._flat.clone()))
        finally:
            dbg.rbvae_dbg_lstm_unit_threads(old)
    (la, ga, wa), (lb, gb, wb) = res
    assert torch.isfinite(la).all()
    assert torch.equal(la, lb) and torch.equal(ga, gb) and torch.equal(wa, wb)
