"""GPU: rbvae_run_jobs_table (the LDS of a job launch worked out by the library from the table's rows) against
rbvae_run_jobs_sized (every workgroup with the fixed 36 992-byte tile) on separate copies of the buffers: every
destination bit for bit -- weights, moments, both packed copies, reduced gradients, gathered rows.

  all       every kind in one table (tests/_jobs_lds_cases.py); its largest job is the whole-row conv pack: 36 976 bytes
  small     fused conv packs in 64-channel pieces, flat Adam jobs, a wave row reduction and a gather: 10 224 bytes, the
            case where the tile shrinks most (a step's update table)
  tiled     the smallest tiled Adam job (2^20 elements) sets the size: 34 816 bytes
Each also with rbvae_job_launch_order's permutation.  Then one Engine.update_jobs table through Engine.run_table against
rbvae_adam_step + Engine.pack, as test_kernels_gpu.test_fused_update_jobs_equal_adam_plus_pack does for the other launches."""
from importlib import import_module

import pytest
import torch

import _jobs_lds_cases as K

pytestmark = pytest.mark.gpu
J = import_module("symbols-from-video_amd.jobs")


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


@pytest.fixture(scope="module")
def sfv():
    import sfv_amd
    return sfv_amd


def run(sfv, names, how):
    dev = torch.device("cuda", 0)
    t = K.Table(names, dev)
    tab = J.JobTable(t.jl, dev, 256)
    if how == "sized":
        sfv._lib.call("rbvae_run_jobs_sized", tab.rows, *tab.block_map)
    else:
        tab.run(heavy_first=how == "ordered")
    torch.cuda.synchronize()
    return t, tab


@pytest.mark.parametrize("names,lds", [(K.ALL, 36976), (K.SMALL, 10224), (K.TILED, 34816)], ids=["all", "small", "tiled"])
def test_table_launch_equals_the_sized_launch(sfv, names, lds):
    ref, tab = run(sfv, names, "sized")
    assert J.job_lds_bytes(ref.jl.rows) == lds
    before = K.Table(names, torch.device("cuda", 0)).outputs
    assert any(not torch.equal(bits(before[k]), bits(v)) for k, v in ref.outputs.items()), "the sized launch wrote nothing"
    for how in ("table", "ordered"):
        got, _ = run(sfv, names, how)
        assert set(got.outputs) == set(ref.outputs)
        for k, v in ref.outputs.items():
            assert torch.equal(bits(got.outputs[k]), bits(v)), f"{how}: {k} differs from rbvae_run_jobs_sized"
    # every output of the table was written by the reference launch (so that the comparison above compares results)
    for k, v in ref.outputs.items():
        assert not torch.equal(bits(before[k]), bits(v)), f"{k} was not written"


def test_refusals(sfv):
    dev = torch.device("cuda", 0)
    t = K.Table(("gather",), dev)
    tab = J.JobTable(t.jl, dev, 256)
    host = tab.host_rows.ctypes.data
    for args in ((None, 1, 256, tab.rows, tab.block_map[0], None), (host, 0, 256, tab.rows, tab.block_map[0], None),
                 (host, 1, 0, tab.rows, tab.block_map[0], None), (host, 1, 256, None, tab.block_map[0], None),
                 (host, 1, 256, tab.rows, None, None), (host, 1, 256, tab.rows, tab.block_map[0].data_ptr() + 4, None)):
        with pytest.raises(ValueError):
            sfv._lib.call("rbvae_run_jobs_table", *args)
    torch.cuda.synchronize()


def test_engine_update_table_equals_adam_plus_pack(sfv):
    """Engine.update_jobs through Engine.run_table (rbvae_run_jobs_table, in map order and heaviest first) against
    rbvae_adam_step + Engine.pack and against the launch through rbvae_run_jobs_sized: parameters, moments and every
    packed copy bit for bit.  percep, 16 input channels, 8 x 8 frames."""
    E = import_module("symbols-from-video_amd.engine")
    packed = ("W1p", "W2f", "W2d", "W3f", "W3d", "Wfc", "WfcT", "Wdfc", "WdfcT", "bdfc", "V1f", "V1d", "V2f", "V2d", "V3p",
              "V3f", "wT_enc", "wT_dec")
    res = []
    for how in ("adam+pack", "table", "ordered", "sized"):
        eng = E.Engine("percep", 16, 16, 32, (8, 8), "bf16", torch.device("cuda", 0))
        n = eng.layout.total
        gen = torch.Generator().manual_seed(96)
        flat = (torch.randn(n, generator=gen) * 0.1).cuda()
        grad = (torch.randn(n, generator=gen) * 0.01).cuda()
        m = (torch.randn(n, generator=gen) * 0.01).cuda()
        v = (torch.rand(n, generator=gen) * 1e-4).cuda()
        step = torch.tensor([6], dtype=torch.int64, device="cuda")
        hyper, one, out4 = torch.zeros(2, device="cuda"), torch.ones(1, device="cuda"), torch.empty(4, device="cuda")
        sfv._lib.call("rbvae_combine_losses", None, 0, 0.0, one, one, 0, 0.0, one, 0, 0.0, 0.0, 1.0, 1.0, out4, step, 2e-3, None,
                      0.9, 0.999, hyper)
        if how == "adam+pack":
            sfv._lib.call("rbvae_adam_step", flat, grad, m, v, n, 2e-3, 0.9, 0.999, 1e-8, 0, 0.5, None, hyper)
            eng.pack(flat)
        else:
            eng.table_launch, eng.jobs_heavy_first = how != "sized", int(how == "ordered")
            tab, nj = eng.update_jobs(flat, grad, m, v, hyper, (0.9, 0.999), 1e-8, 0.5)
            t = eng.table_of(tab)
            assert J.job_lds_bytes(t.jl.rows) == 10224 and t.block_map[1] < nj * 256
            eng.run_table(tab, nj, 1)
        torch.cuda.synchronize()
        lay = eng.layout
        pv = {f"{t}/{nm}": lay.view(buf, nm).clone() for t, buf in (("w", flat), ("m", m), ("v", v)) for nm in lay.names}
        res.append({**pv, **{k: getattr(eng, k).clone() for k in packed}})
    for k in res[0]:
        for other, how in zip(res[1:], ("table", "ordered", "sized")):
            assert torch.equal(bits(res[0][k]), bits(other[k])), f"{how}: {k}"
