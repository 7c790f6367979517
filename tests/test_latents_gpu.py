"""GPU: _latents.encode_frames, the one path from the script's frames to soft latents and hard codes, against a stub model
that records what encode() is given: which uniforms the helper draws and when, what it skips when the latents are given,
and the mode it leaves the model in.  6 frames of [3, 8, 8] and latent_dim 5: nothing here launches a kernel of the
library."""
from importlib import import_module

import pytest
import torch

import sfv_amd as sfv

pytestmark = pytest.mark.gpu

H = import_module("symbols-from-video_amd._latents")
F_, LD = 6, 5


class Stub:
    """encode() returns a function of u: the soft latents are u itself, the hard codes u > 0.5"""

    def __init__(self, training=True, fail=False):
        self.training, self.latent_dim, self.fail, self.calls, self.modes = training, LD, fail, [], []

    def eval(self):
        self.training = False

    def train(self, mode=True):
        self.training = mode

    def encode(self, x, temperature=0.5, hard=False, noise_ratio=0.1, u=None):
        self.calls.append(dict(x=x, temperature=temperature, hard=hard, noise_ratio=noise_ratio, u=u))
        self.modes.append(self.training)
        if self.fail:
            raise RuntimeError("encode failed")
        return ((u > 0.5) if hard else u).double()[:, None]


@pytest.fixture(scope="module")
def x():
    return torch.rand(F_, 3, 8, 8, generator=torch.Generator().manual_seed(1)).cuda()


@pytest.mark.parametrize("hard", (False, True))
def test_draws_once_on_the_host(x, hard):
    m = Stub()
    torch.manual_seed(5)
    z, codes = H.encode_frames(m, x, hard=hard, temperature=0.3, noise_ratio=0.2)
    after = torch.get_rng_state()
    torch.manual_seed(5)
    u = torch.rand((F_, LD))
    assert torch.equal(after, torch.get_rng_state())        # one draw of [F, L], nothing else
    assert [c["hard"] for c in m.calls] == ([False, True] if hard else [False]) and m.modes == [False] * len(m.calls)
    for c in m.calls:
        assert c["u"].is_cuda and torch.equal(c["u"].cpu(), u) and c["u"] is m.calls[0]["u"]
        assert c["x"].shape == (F_, 1, 3, 8, 8) and torch.equal(c["x"][:, 0], x)
        assert c["temperature"] == 0.3 and c["noise_ratio"] == 0.2
    assert z.dtype == torch.float32 and z.is_contiguous() and torch.equal(z.cpu(), u) and m.training
    if hard:
        assert codes.dtype == torch.float32 and codes.is_contiguous() and torch.equal(codes.cpu(), (u > 0.5).float())
    else:
        assert codes is None


def test_given_uniforms_are_used(x):
    m = Stub(training=False)
    u = torch.rand(F_, LD, generator=torch.Generator().manual_seed(2))
    before = torch.get_rng_state()
    z, codes = H.encode_frames(m, x, hard=True, u=u)
    assert torch.equal(before, torch.get_rng_state()) and torch.equal(z.cpu(), u) and torch.equal(codes.cpu(), (u > 0.5).float())
    assert len(m.calls) == 2 and not m.training and m.calls[0]["temperature"] == 0.2 and m.calls[0]["noise_ratio"] == 0.3


def test_given_latents(x):
    lat = torch.rand(F_, LD, generator=torch.Generator().manual_seed(3)).cuda().double()
    m = Stub()
    before = torch.get_rng_state()
    z, codes = H.encode_frames(m, x, hard=False, latents=lat)
    assert m.calls == [] and torch.equal(before, torch.get_rng_state()) and m.training       # nothing ran, nothing was drawn
    assert codes is None and z.dtype == torch.float32 and torch.equal(z, lat.float())
    torch.manual_seed(5)
    z, codes = H.encode_frames(m, x, hard=True, latents=lat)
    torch.manual_seed(5)
    u = torch.rand((F_, LD))                                 # the hard pass needs the uniforms: drawn as without latents
    assert [c["hard"] for c in m.calls] == [True] and torch.equal(m.calls[0]["u"].cpu(), u) and m.training
    assert torch.equal(z, lat.float()) and torch.equal(codes.cpu(), (u > 0.5).float())


@pytest.mark.parametrize("training", (False, True))
def test_mode_is_restored_when_encode_raises(x, training):
    m = Stub(training=training, fail=True)
    with pytest.raises(RuntimeError, match="encode failed"):
        H.encode_frames(m, x, hard=True)
    assert m.training is training and m.modes == [False]


CALLS = {"latent_scores": sfv.latent_scores, "latent_symbols": sfv.latent_symbols, "latent_segments": sfv.latent_segments,
         "latent_mixture": sfv.latent_mixture, "latent_hmm": sfv.latent_hmm,
         "latent_projections": lambda m, x, fi, fl: sfv.latent_projections(m, x, frame_indices=fi, flags=fl),
         "latent_spectral": sfv.latent_spectral}


@pytest.mark.parametrize("name", sorted(CALLS))
def test_refusals_in_order(x, name):
    """a CPU x ahead of a 3-D x ahead of a wrong frame count, each in the words the seven functions have always used"""
    m, wrong = Stub(), list(range(F_ - 1))
    with pytest.raises(ValueError, match=r"^x must be on the GPU \(there is no CPU path\)$"):
        CALLS[name](m, x.cpu()[0], wrong, [2])
    with pytest.raises(ValueError, match=r"^x must be \[F, C, H, W\], got \(3, 8, 8\)$"):
        CALLS[name](m, x[0], wrong, [2])
    assert m.calls == []
    if name not in ("latent_projections", "latent_spectral"):       # those two encode and project first
        with pytest.raises(ValueError, match="^5 frame indices for 6 frames$"):
            CALLS[name](m, x, wrong, [2])
        assert m.calls == [] and m.training
    assert H.frame_count(x) == F_
