"""Guidance interval, host side (no GPU): the per-step flag function against hand-written lists, the parser's flag and its
refusal, the ValueErrors of y['guidance_interval'], and the two C exports on a null handle."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from test_dpm_host import diffusion

T, F = True, False


def _full():
    from gesturediffusion_amd.diffusion import gaussian_diffusion as gd
    return gd.GaussianDiffusion(betas=gd.get_named_beta_schedule("cosine", 1000), model_mean_type=gd.ModelMeanType.START_X,
                                model_var_type=gd.ModelVarType.FIXED_SMALL, loss_type=gd.LossType.MSE)


# --------------------------------------------------------------------------------------------------------- the flag function
def test_flags_full_schedule():
    """1000 steps, the identity map: index i is model timestep i."""
    df = _full()
    flags = df.guided_steps((300, 700))
    assert flags == [F] * 300 + [T] * 401 + [F] * 299
    assert df.guided_steps(None) == [T] * 1000
    assert df.guided_steps((999, 999)) == [F] * 999 + [T]
    assert df.guided_steps((0, 0)) == [T] + [F] * 999


def test_flags_ddim10():
    df = diffusion("cosine", "ddim10")
    assert df.timestep_map == [0, 100, 200, 300, 400, 500, 600, 700, 800, 900]
    assert df.guided_steps((300, 700)) == [F, F, F, T, T, T, T, T, F, F]         # both bounds are kept timesteps: inclusive
    assert df.guided_steps((301, 699)) == [F, F, F, F, T, T, T, F, F, F]         # one inside either bound
    assert df.guided_steps((300, 600)) == [F, F, F, T, T, T, T, F, F, F]
    assert df.guided_steps((250, 260)) == [F] * 10                               # between two kept timesteps
    assert df.guided_steps(None) == [T] * 10


def test_flags_logsnr10():
    df = diffusion("linear", "logsnr10")
    assert df.timestep_map == [0, 5, 22, 73, 202, 410, 603, 757, 886, 999]
    assert df.guided_steps((300, 700)) == [F, F, F, F, F, T, T, F, F, F]
    assert df.guided_steps((73, 603)) == [F, F, F, T, T, T, T, F, F, F]
    assert df.guided_steps((5, 5)) == [F, T, F, F, F, F, F, F, F, F]


def test_flags_section_respacing():
    df = diffusion("cosine", [20])
    assert df.timestep_map == [0, 53, 105, 158, 210, 263, 315, 368, 421, 473, 526, 578, 631, 684, 736, 789, 841, 894, 946, 999]
    assert df.guided_steps((300, 700)) == [F] * 6 + [T] * 8 + [F] * 6            # 315 .. 684
    assert df.guided_steps((315, 684)) == [F] * 6 + [T] * 8 + [F] * 6
    assert df.guided_steps((316, 683)) == [F] * 7 + [T] * 6 + [F] * 7


def test_flags_empty_and_outside():
    for df, n in ((diffusion("cosine", "ddim10"), 10), (diffusion("linear", "logsnr10"), 10), (_full(), 1000)):
        assert df.guided_steps((1, 0)) == [F] * n                                # lo > hi: the legal empty interval
        assert df.guided_steps((700, 300)) == [F] * n
        assert df.guided_steps((-5, 2000)) == [T] * n                            # bounds outside 0..999
        assert df.guided_steps((1000, 5000)) == [F] * n
        assert df.guided_steps((-10, -1)) == [F] * n
        assert df.guided_steps((-2**63, 2**63 - 1)) == [T] * n                   # the library's default
    assert diffusion("cosine", "ddim10").guided_steps((-7, 100)) == [T, T] + [F] * 8


# --------------------------------------------------------------------------------------------------------------- the parser
def test_parser_takes_the_flag():
    from gesturediffusion_amd.utils.parser_util import generate_args
    a = generate_args(["--synthetic", "--guidance_interval", "300", "700"])
    assert a.guidance_interval == [300, 700] and a.guidance_param == 2.5
    assert generate_args(["--synthetic"]).guidance_interval is None
    assert generate_args(["--synthetic", "--guidance_interval", "700", "300"]).guidance_interval == [700, 300]   # empty, legal
    for sampler in ("p", "ddim", "plms", "dpmpp", "dpmpp_sde"):
        assert generate_args(["--synthetic", "--sampler", sampler, "--guidance_interval", "0", "999"]).guidance_interval == [0, 999]


def test_parser_refuses_the_flag_without_guidance(capsys):
    from gesturediffusion_amd.utils.parser_util import generate_args
    with pytest.raises(SystemExit):
        generate_args(["--synthetic", "--guidance_param", "1", "--guidance_interval", "300", "700"])
    assert "--guidance_interval needs guidance" in capsys.readouterr().err
    with pytest.raises(SystemExit):                        # a model trained without condition dropout: the scale becomes 1
        generate_args(["--synthetic", "--cond_mask_prob", "0", "--guidance_interval", "300", "700"])
    with pytest.raises(SystemExit):
        generate_args(["--synthetic", "--guidance_interval", "300"])
    with pytest.raises(SystemExit):
        generate_args(["--synthetic", "--guidance_interval", "300.5", "700"])
    assert generate_args(["--synthetic", "--guidance_param", "1"]).guidance_interval is None


def test_sample_chunks_refuses_an_interval_without_guidance():
    from gesturediffusion_amd.sample.generate import sample_chunks
    with pytest.raises(ValueError, match="guidance_interval needs guidance_param"):
        sample_chunks(None, diffusion("cosine", "ddim10"), torch.zeros(2, 16, 1, 10), None, 1, 20, 10, guidance_param=1.0,
                      guidance_interval=(300, 700))


# ----------------------------------------------------------------------------------------------------------- the ValueErrors
def test_key_validation():
    from gesturediffusion_amd.engine import guidance_interval_of
    assert guidance_interval_of({}, True) is None and guidance_interval_of({}, False) is None      # absent: today's behaviour
    assert guidance_interval_of({"guidance_interval": (300, 700)}, True) == (300, 700)
    assert guidance_interval_of({"guidance_interval": [700, 300]}, True) == (700, 300)
    assert guidance_interval_of({"guidance_interval": (np.int64(3), -4)}, True) == (3, -4)
    with pytest.raises(ValueError, match="ClassifierFreeSampleModel"):
        guidance_interval_of({"guidance_interval": (300, 700)}, False)
    for bad in ((300,), (1, 2, 3), (300.0, 700), ("300", "700"), 300, None, (True, 5), {300, 700}, (2**63, 0), (0, -2**63 - 1)):
        with pytest.raises(ValueError, match="guidance_interval"):
            guidance_interval_of({"guidance_interval": bad}, True)
    for bad in (torch.tensor([300, 700]), (torch.tensor(300), torch.tensor(700))):
        with pytest.raises(ValueError, match="guidance_interval"):
            guidance_interval_of({"guidance_interval": bad}, True)
    with pytest.raises(ValueError, match="synchronise"):
        guidance_interval_of({"guidance_interval": torch.tensor([300, 700])}, True)


# ------------------------------------------------------------------------------------------------------------------- C ABI
def _lib_or_skip():
    from gesturediffusion_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgdx.so not built (run python __graft_entry__.py)")
    return _lib


def test_null_handle_is_refused_without_a_hip_call():
    _lib = _lib_or_skip()
    lib = _lib.load()
    assert lib.gdx_set_guidance_interval(None, 300, 700) == -1
    assert b"gdx_set_guidance_interval: null handle" in lib.gdx_last_error()
    n = C.c_int64(-7)
    assert lib.gdx_forward_samples(None, C.byref(n)) == -1
    assert b"gdx_forward_samples: null argument" in lib.gdx_last_error() and n.value == -7
    h = C.c_void_p()
    cfg = _lib.Config(arch=1, njoints=16, latent_dim=128, ff_size=256, num_layers=2, num_heads=4, seed_poses=10, mfcc_dim=26,
                      cl_head=8, window=10)
    if lib.gdx_create(C.byref(cfg), C.byref(h)) == 0:          # where a handle can be made without a device
        assert lib.gdx_forward_samples(h, None) == -1
        assert lib.gdx_set_guidance_interval(h, 700, 300) == 0 and lib.gdx_set_guidance_interval(h, -2**63, 2**63 - 1) == 0
        assert lib.gdx_forward_samples(h, C.byref(n)) == 0 and n.value == 0
        lib.gdx_destroy(h)
