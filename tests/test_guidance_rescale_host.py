"""Guidance rescale, host side (no GPU): the two C exports and their refusals before any HIP call, the ValueErrors of
y['guidance_rescale'], the parser's flag and its refusals, and self-checks of the CPU restatement on random data."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import guidance_rescale_restatement as RR
from test_dpm_host import diffusion


# ------------------------------------------------------------------------------------------------------------------- C ABI
def _lib_or_skip():
    from gesturediffusion_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgdx.so not built (run python __graft_entry__.py)")
    return _lib


def test_set_guidance_rescale_refusals():
    _lib = _lib_or_skip()
    lib = _lib.load()
    assert lib.gdx_set_guidance_rescale(None, 0.5) == -1
    assert b"gdx_set_guidance_rescale: null handle" in lib.gdx_last_error()
    h = C.c_void_p()
    cfg = _lib.Config(arch=1, njoints=16, latent_dim=128, ff_size=256, num_layers=2, num_heads=4, seed_poses=10, mfcc_dim=26,
                      cl_head=8, window=10)
    if lib.gdx_create(C.byref(cfg), C.byref(h)) == 0:          # where a handle can be made without a device
        for bad in (-0.1, 1.5, math.nan, math.inf):
            assert lib.gdx_set_guidance_rescale(h, bad) == -1, bad
            assert b"gdx_set_guidance_rescale: phi must lie in [0, 1]" in lib.gdx_last_error()
        for ok in (0.0, 0.7, 1.0):
            assert lib.gdx_set_guidance_rescale(h, ok) == 0, ok
        lib.gdx_destroy(h)


def test_cfg_rescale_refusals_precede_any_hip_call():
    """Every pointer is a made-up non-null address: a refusal that came after a launch could not return cleanly here."""
    _lib = _lib_or_skip()
    lib = _lib.load()
    assert lib.gdx_cfg_rescale(None, None) == -1
    assert b"gdx_cfg_rescale: null argument" in lib.gdx_last_error()
    good = dict(batch=2, njoints=16, frames=20, x0_cond=0x1000, x0_uncond=0x2000, scale=0x3000, phi=0.7, t=None, lo=0, hi=0,
                workspace=0x4000, factor=0x5000, out=0x6000)
    for name in ("x0_cond", "x0_uncond", "scale", "workspace", "factor", "out"):
        a = _lib.CfgRescaleArgs(**dict(good, **{name: None}))
        assert lib.gdx_cfg_rescale(C.byref(a), None) == -1, name
        assert b"gdx_cfg_rescale: null argument" in lib.gdx_last_error(), name
    for field, value in (("batch", 0), ("batch", 65536), ("batch", -1), ("njoints", 0), ("frames", 0)):
        a = _lib.CfgRescaleArgs(**dict(good, **{field: value}))
        assert lib.gdx_cfg_rescale(C.byref(a), None) == -1, (field, value)
        assert b"gdx_cfg_rescale: bad shape" in lib.gdx_last_error(), (field, value)
    for bad in (-0.1, 1.5, math.nan):
        a = _lib.CfgRescaleArgs(**dict(good, phi=bad))
        assert lib.gdx_cfg_rescale(C.byref(a), None) == -1, bad
        assert b"gdx_cfg_rescale: phi must lie in [0, 1]" in lib.gdx_last_error(), bad


# ----------------------------------------------------------------------------------------------------------- the ValueErrors
def test_key_validation():
    from gesturediffusion_amd.engine import guidance_rescale_of
    assert guidance_rescale_of({}, True) == 0.0 and guidance_rescale_of({}, False) == 0.0       # absent: off
    for ok in (0, 0.0, 0.7, 1, 1.0):
        got = guidance_rescale_of({"guidance_rescale": ok}, True)
        assert isinstance(got, float) and got == ok
    with pytest.raises(ValueError, match="ClassifierFreeSampleModel"):
        guidance_rescale_of({"guidance_rescale": 0.7}, False)
    with pytest.raises(ValueError, match="ClassifierFreeSampleModel"):
        guidance_rescale_of({"guidance_rescale": 0}, False)
    for bad in (True, False, -0.1, 1.5, 2, -1, math.nan, math.inf, -math.inf, "0.7", None, (0.7,), [0.7]):
        with pytest.raises(ValueError, match="guidance_rescale"):
            guidance_rescale_of({"guidance_rescale": bad}, True)
    for bad in (torch.tensor(0.7), torch.tensor([0.7])):
        with pytest.raises(ValueError, match="synchronise"):
            guidance_rescale_of({"guidance_rescale": bad}, True)


# --------------------------------------------------------------------------------------------------------------- the parser
def test_parser_takes_the_flag():
    from gesturediffusion_amd.utils.parser_util import generate_args
    assert generate_args(["--synthetic"]).guidance_rescale == 0.0
    assert generate_args(["--synthetic", "--guidance_param", "1"]).guidance_rescale == 0.0
    for sampler in ("p", "ddim", "plms", "dpmpp", "dpmpp_sde"):
        assert generate_args(["--synthetic", "--sampler", sampler, "--guidance_rescale", "0.7"]).guidance_rescale == 0.7
    assert generate_args(["--synthetic", "--guidance_rescale", "1"]).guidance_rescale == 1.0
    assert generate_args(["--synthetic", "--guidance_rescale", "0", "--guidance_param", "1"]).guidance_rescale == 0.0


def test_parser_refusals(capsys):
    from gesturediffusion_amd.utils.parser_util import generate_args
    with pytest.raises(SystemExit):
        generate_args(["--synthetic", "--guidance_rescale", "0.7", "--guidance_param", "1"])
    assert "--guidance_rescale needs guidance" in capsys.readouterr().err
    with pytest.raises(SystemExit):                        # a model trained without condition dropout: the scale becomes 1
        generate_args(["--synthetic", "--cond_mask_prob", "0", "--guidance_rescale", "0.7"])
    for bad in ("1.5", "-0.1", "nan"):
        with pytest.raises(SystemExit):
            generate_args(["--synthetic", "--guidance_rescale", bad])
        assert "--guidance_rescale must lie in [0, 1]" in capsys.readouterr().err


def test_sample_chunks_refuses_a_rescale_without_guidance():
    from gesturediffusion_amd.sample.generate import sample_chunks
    with pytest.raises(ValueError, match="guidance_rescale needs guidance_param"):
        sample_chunks(None, diffusion("cosine", "ddim10"), torch.zeros(2, 16, 1, 10), None, 1, 20, 10, guidance_param=1.0,
                      guidance_rescale=0.7)


# ------------------------------------------------------------------------------------------- self-checks of the restatement
def _data(B=3, J=16, T=33, offset=0.0, seed=5):
    g = torch.Generator().manual_seed(seed)
    c = torch.randn(B, J, 1, T, generator=g) + offset
    u = torch.randn(B, J, 1, T, generator=g) + offset
    return c, u, torch.tensor([2.5, -1.0, 0.3])[:B]


def _std64(v):
    return v.reshape(v.shape[0], -1).double().std(dim=1)


def test_restatement_phi_zero_is_the_blend():
    for offset in (0.0, 50.0):
        c, u, s = _data(offset=offset)
        out, f = RR.rescale(c, u, s, 0.0)
        assert torch.equal(f, torch.ones(3)) and torch.equal(out, u + s.view(-1, 1, 1, 1) * (c - u))


def test_restatement_phi_one_matches_the_standard_deviation():
    """std(out) / std(c) within 1e-6 of 1 for |mean| <= std: f is one rounding (2^-24 relative) off the fp64 ratio and every
    product g * f one more, of which the standard deviation of N elements sees at most the worst, so about 3 * 2^-24 = 1.8e-7
    with the input means' own contribution; 1e-6 leaves a margin of five."""
    for offset in (0.0, 0.5, -0.9):
        c, u, s = _data(offset=offset)
        assert bool((c.reshape(3, -1).mean(1).abs() <= c.reshape(3, -1).std(1)).all())
        out, f = RR.rescale(c, u, s, 1.0)
        ratio = _std64(out) / _std64(c)
        assert float((ratio - 1).abs().max()) < 1e-6, ratio
        assert float((f - 1).abs().max()) > 1e-2             # and the factor did something at these scales


def test_restatement_mixes_linearly_in_phi():
    c, u, s = _data()
    _, f1 = RR.rescale(c, u, s, 1.0)
    _, f7 = RR.rescale(c, u, s, 0.7)
    phi = np.float64(np.float32(0.7))
    want = phi * f1.double().numpy() + (1 - phi)
    assert np.abs(f7.double().numpy() - want).max() < 2 ** -22


def test_restatement_constant_guided_output_and_unguided_samples():
    c = torch.full((2, 16, 1, 20), 3.25)
    out, f = RR.rescale(c, c.clone(), torch.tensor([2.5, -1.0]), 0.7)
    assert torch.equal(f, torch.ones(2)) and torch.equal(out, c)
    c, u, s = _data()
    guided = torch.tensor([False, True, False])
    out, f = RR.rescale(c, u, s, 0.7, guided)
    every, fe = RR.rescale(c, u, s, 0.7)
    assert torch.equal(out[0], c[0]) and torch.equal(out[2], c[2]) and torch.equal(out[1], every[1])
    assert f[0] == 1 and f[2] == 1 and f[1] == fe[1]


def test_restatement_nan_stays_in_its_sample():
    c, u, s = _data()
    clean, fc = RR.rescale(c, u, s, 0.7)
    c2 = c.clone()
    c2[1, 3, 0, 4] = math.nan
    out, f = RR.rescale(c2, u, s, 0.7)
    assert math.isnan(float(f[1])) and bool(torch.isnan(out[1]).all())
    assert torch.equal(out[0], clean[0]) and torch.equal(out[2], clean[2]) and f[0] == fc[0] and f[2] == fc[2]
