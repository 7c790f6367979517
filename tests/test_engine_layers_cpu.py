"""The engine's layer records (engine.Stride2: conv2, conv3, deconv0, deconv1) against the parameter layout, for the four
variants at the frame sizes of tests/_arms_cases.py and of bench.py, in both storage dtypes.  Every stride-2 launch of the
step takes its channels, grids, packed operands and parameter names from these records, so a transposed pair in one of
them is a wrong launch in forward, input gradient and weight gradient alike.  Host only: the engine is constructed on the
CPU device, nothing is launched and the library is not loaded."""
from importlib import import_module

import pytest
import torch

E = import_module("symbols-from-video_amd.engine")

# (variant, channels in, frame): the step-arms cases, the bench shape and the simple variant's native frame
SHAPES = [("percep", 4, (88, 160)), ("percep", 4, (64, 64)), ("percep", 4, (32, 32)), ("contrastive", 3, (48, 80)),
          ("triplet", 3, (64, 64)), ("simple", 3, (64, 64))]


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("variant,cin,hw", SHAPES)
def test_layer_records_match_the_layout(variant, cin, hw, dtype):
    eng = E.Engine(variant, cin, cin, 32, hw, dtype=dtype, device=torch.device("cpu"))
    lay, k, kk = eng.layout, eng.k, eng.k * eng.k
    assert eng.stride2 == (eng.conv2, eng.conv3, eng.deconv0, eng.deconv1)
    for ly in eng.stride2:
        assert ly.weight in lay.shapes and ly.bias in lay.shapes
        assert lay.shapes[ly.weight] == (ly.cs, ly.cb, k, k)
        assert tuple(ly.f.shape) == (ly.cs, kk, ly.cb) and tuple(ly.d.shape) == (ly.cb, kk, ly.cs)
        assert ly.f.dtype == ly.d.dtype == eng.tdt
        assert ly.big == (2 * ly.small[0], 2 * ly.small[1])
    # a conv's bias has its small-grid channels, a deconv's its big-grid channels
    assert [lay.shapes[ly.bias] for ly in eng.stride2] == [(eng.conv2.cs,), (eng.conv3.cs,), (eng.deconv0.cb,), (eng.deconv1.cb,)]
    for ly in (eng.conv1, eng.deconv2):
        assert ly.weight in lay.shapes and ly.bias in lay.shapes
    # no packed copy is shared, and the four records are the four stride-2 parameters of the layout
    assert len({t.data_ptr() for ly in eng.stride2 for t in (ly.f, ly.d)}) == 8
    names = {n for n in lay.names if n.endswith(".weight") and ("conv." in n or "deconv." in n)}
    assert {ly.weight for ly in eng.stride2} | {eng.conv1.weight, eng.deconv2.weight} == names
    # the grids halve from the frame down to the bottleneck, encoder and decoder over the same three
    H, W = hw
    assert eng.conv2.big == (H // 2, W // 2) == eng.deconv1.big
    assert eng.conv2.small == eng.conv3.big == eng.deconv0.big == eng.deconv1.small == (H // 4, W // 4)
    assert eng.conv3.small == eng.deconv0.small == lay.bott == (H // 8, W // 8)
    # channels chain: conv2's output is conv3's input, deconv0's output is deconv1's input
    assert (eng.conv2.cb, eng.conv2.cs, eng.conv3.cs) == eng.v.channels == (eng.deconv1.cb, eng.deconv0.cb, eng.deconv0.cs)
    assert eng.conv3.cb == eng.conv2.cs and eng.deconv1.cs == eng.deconv0.cb
