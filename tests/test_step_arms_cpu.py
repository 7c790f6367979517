"""Host side of the large-frame arm step tests (tests/_arms_cases.py): the mask-layout helper against a plain loop, the
gated f64 oracle against the plain one, and the sensitivity table -- four named wiring defects, each derived at a reduced
case and held to the gates test_step_arms_gpu.py applies."""
import numpy as np
import pytest
import torch

import rbvae_oracle as O

import _arms_cases as A


@pytest.mark.parametrize("n_seq,h,w,c", [(2, 2, 3, 8), (3, 1, 5, 16)])
def test_rows_to_oracle_against_a_plain_loop(n_seq, h, w, c):
    rows = np.random.default_rng(5).integers(0, 2, size=(2 * n_seq * h * w, c)).astype(bool)
    v = A.rows_to_oracle(rows, n_seq, h, w)
    assert v[0].shape == v[1].shape == (n_seq, c, h, w)
    r = 0
    for view in range(2):
        for n in range(n_seq):
            for y in range(h):
                for x in range(w):
                    for ch in range(c):
                        assert bool(v[view][n, ch, y, x]) == bool(rows[r, ch]), (view, n, y, x, ch)
                    r += 1


def test_keyed_masks_have_the_sites_shapes_and_differ_between_sites():
    case = A.BY_ID["triplet_64x64"]
    rows, orc = A.keyed_masks(case, 12345, 0)
    for k, (c, h, w) in enumerate(A.site_maps(case)):
        assert rows[k].shape == (2 * A.B * A.T * h * w, c)
        assert orc[0][k].shape == orc[1][k].shape == (A.B * A.T, c, h, w)
        kept = float(rows[k].float().mean())
        assert abs(kept - 0.8) < 0.01, kept
    assert not torch.equal(rows[0], rows[3]) and not torch.equal(rows[1], rows[2])
    again, _ = A.keyed_masks(case, 12345, 1)
    assert not torch.equal(rows[0], again[0])                      # the step counter enters the key


def test_pinned_launches_name_every_arm():
    seen = {n for c in A.CASES for n, _ in c["launches"]}
    assert seen == set(A.ARMS)
    for c in A.CASES:
        assert not set(A.expected_launches(c, "off")) & set(A.SWITCHES.values())
        assert set(A.expected_launches(c, "off")) == {A.CONV_FIRST, A.DECONV_LAST, A.FC_GEMM}
        kept = A.expected_launches(c, "wgrad_off")
        assert not set(kept) & {A.WGRAD_HALO, A.WGRAD_ROW, A.WGRAD_FIRST} and len(kept) < len(c["launches"])


def _small(hw, seed):
    case = dict(variant="percep", in_ch=4, hw=hw, data_seed=seed)
    item, U = A.inputs(case)
    torch.manual_seed(seed + 1)
    w0 = O.init_params("percep", 4, 4, A.LATENT, hw)
    return item, U, {k: v.detach().float() for k, v in w0.items()}


def test_gated_oracle_equals_the_plain_oracle_bit_for_bit():
    """Given gates = (pre-activation > 0) the f64 oracle is the plain f64 oracle: losses and every gradient bit-equal."""
    item, U, w0 = _small((16, 16), 81)
    plain, g_plain, pre = A.oracle_step("percep", w0, item, U, torch.float64, False, want_pre=True)
    gates = [[x > 0 for x in pv] for pv in pre]
    gated, g_gated, pre2 = A.oracle_step("percep", w0, item, U, torch.float64, False, gates=gates, want_pre=True)
    assert plain == gated
    for k in g_plain:
        assert torch.equal(g_plain[k], g_gated[k]), k
    from importlib import import_module
    assert import_module("symbols-from-video_amd._gates").count_ties(pre2, gates, None, A.TIE_BOUND) == 0


def test_sensitivity_of_the_gates_to_four_wiring_defects(monkeypatch):
    """percep widths, 4 x 16 x 24 frames (maps 8x12, 4x6, 2x3; 384 rows = three 128-row tiles at the first map), f64.  The
    tap-by-tap weight gradient without a defect is autograd's; with one defect each, the relative L2 against the clean
    oracle says which gate of the GPU file sees it."""
    item, U, w0 = _small((16, 24), 83)
    trace = A.TraceF(O.F)
    monkeypatch.setattr(O, "F", trace)
    _, clean, _ = A.oracle_step("percep", w0, item, U, torch.float64, False)
    monkeypatch.undo()
    assert len(trace.calls) == 12 and all("dy" in c for c in trace.calls)
    n_seq = A.B * A.T
    for j, name in ((0, A.CONV1_W), (1, A.CONV2_W)):
        whole = sum(A.conv_wgrad(trace.calls[6 * v + j]["x"], trace.calls[6 * v + j]["dy"]) for v in range(2))
        assert A.rel_l2(whole, clean[name]) < 1e-12, name
    rows = torch.cat([trace.calls[6 * v]["dy"].permute(0, 2, 3, 1).reshape(-1, 256) for v in range(2)])
    assert A.rel_l2(rows.sum(0), clean[A.CONV1_B]) < 1e-12
    for name, (tensor, is_wgrad, want) in A.DEFECTS.items():
        bad = A.defective(name, clean, trace, n_seq)
        assert bad.shape == clean[tensor].shape
        err = A.rel_l2(bad, clean[tensor])
        got = A.caught_by(err, is_wgrad)
        print(f"\nARMS sensitivity {name}: {tensor} moves by {err:.3e} relative L2 -> seen by {got}")
        assert got is not None, f"{name}: {err:.3e} is below both gates"
        assert got == want, (name, err, got, want)
