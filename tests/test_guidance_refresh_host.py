"""Guidance refresh, host side (no GPU): the ValueErrors of y['guidance_refresh'], the refusal of everything that cannot
remember across calls, GaussianDiffusion.guidance_plan against hand-written lists and against the restatement's counter, the
parser's flag, and the two C exports' refusals before any HIP call."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import guidance_refresh_restatement as FR
from test_dpm_host import diffusion

O, R, U = "off", "refresh", "reuse"


# ----------------------------------------------------------------------------------------------------------- the ValueErrors
def test_key_validation():
    from gesturediffusion_amd.engine import guidance_refresh_of
    assert guidance_refresh_of({}, True) == 1 and guidance_refresh_of({}, False) == 1           # absent: off
    for ok in (1, 2, 3, 4, 1000, np.int64(2)):
        got = guidance_refresh_of({"guidance_refresh": ok}, True)
        assert type(got) is int and got == ok
    with pytest.raises(ValueError, match="ClassifierFreeSampleModel"):
        guidance_refresh_of({"guidance_refresh": 2}, False)
    with pytest.raises(ValueError, match="ClassifierFreeSampleModel"):
        guidance_refresh_of({"guidance_refresh": 1}, False)
    for bad in (True, False, 2.0, 1.5, 0, -1, -2**40, 2**31, "2", None, (2,), [2], float("nan")):
        with pytest.raises(ValueError, match="guidance_refresh"):
            guidance_refresh_of({"guidance_refresh": bad}, True)
    for bad in (torch.tensor(2), torch.tensor([2])):
        with pytest.raises(ValueError, match="synchronise"):
            guidance_refresh_of({"guidance_refresh": bad}, True)


def test_paths_without_memory_refuse_the_key():
    """every > 1 outside the in-library loops is a ValueError that names the in-library loop; every = 1 and no key pass."""
    from gesturediffusion_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    from gesturediffusion_amd.model.cfg_sampler import ClassifierFreeSampleModel
    from gesturediffusion_amd.sampling_options import MEMORY, read

    def refuse(y, guided_model, who):
        read(y, guided=guided_model, num_layers=8, use_text=False, options=MEMORY).refuse_memory(who)
    for k in (2, 3, 100):
        with pytest.raises(ValueError, match="in-library loop") as e:
            refuse({"guidance_refresh": k}, True, "the step-wise forward")
        assert "the step-wise forward" in str(e.value) and f"= {k}" in str(e.value)
    refuse({"guidance_refresh": 1}, True, "x")
    refuse({}, True, "x")
    refuse({}, False, "x")
    with pytest.raises(ValueError, match="ClassifierFreeSampleModel"):
        refuse({"guidance_refresh": 2}, False, "x")
    with pytest.raises(ValueError, match="guidance_refresh"):
        refuse({"guidance_refresh": 0}, True, "x")
    guided = object.__new__(ClassifierFreeSampleModel)       # only its type is looked at
    with pytest.raises(ValueError, match="in-library loop"):
        GaussianDiffusion._refuse_refresh(guided, {"y": {"guidance_refresh": 2}}, "calc_bpd_loop")
    GaussianDiffusion._refuse_refresh(guided, {"y": {"guidance_refresh": 1}}, "calc_bpd_loop")
    GaussianDiffusion._refuse_refresh(guided, {"y": {}}, "calc_bpd_loop")
    GaussianDiffusion._refuse_refresh(guided, None, "calc_bpd_loop")
    with pytest.raises(ValueError, match="ClassifierFreeSampleModel"):       # a non-native / unguided model with the key
        GaussianDiffusion._refuse_refresh(lambda x, t, **kw: x, {"y": {"guidance_refresh": 2}}, "a step-wise loop")


def test_stepwise_routes_refuse_before_the_first_model_call():
    """calc_bpd_loop, a progressive generator, fused=False and a non-native model with k = 2: ValueError, the model never called."""
    from gesturediffusion_amd.model.cfg_sampler import ClassifierFreeSampleModel
    df = diffusion("cosine", "ddim10")

    class Never(ClassifierFreeSampleModel):
        def __init__(self):                                  # no inner model: nothing here may reach it
            torch.nn.Module.__init__(self)

        def forward(self, *a, **k):
            raise AssertionError("the model was called")

    m = Never()
    y = {"guidance_refresh": 2, "scale": torch.ones(2)}
    x = torch.zeros(2, 16, 1, 20)
    kw = dict(model_kwargs={"y": y}, device=torch.device("cpu"))
    with pytest.raises(ValueError, match="in-library loop"):
        df.calc_bpd_loop(m, x, model_kwargs={"y": y})
    with pytest.raises(ValueError, match="in-library loop"):
        df.calc_bpd_loop(m, x, model_kwargs={"y": y}, fused=False)
    for gen in (df.p_sample_loop_progressive, df.ddim_sample_loop_progressive, df.plms_sample_loop_progressive,
                df.dpm_solver_sample_loop_progressive, df.dpm_solver_sde_sample_loop_progressive):
        with pytest.raises(ValueError, match="in-library loop"):
            next(gen(m, x.shape, noise=x, **kw))
    for loop in (df.p_sample_loop, df.ddim_sample_loop, df.plms_sample_loop, df.dpm_solver_sample_loop,
                 df.dpm_solver_sde_sample_loop):
        with pytest.raises(ValueError, match="in-library loop"):
            loop(m, x.shape, noise=x, fused=False, **kw)
        with pytest.raises(ValueError, match="in-library loop"):      # routed step-wise by a denoised_fn
            loop(m, x.shape, noise=x, denoised_fn=lambda v: v, **kw)
        with pytest.raises(ValueError, match="ClassifierFreeSampleModel"):      # a non-native callable with the key
            loop(lambda xx, t, **k: xx, x.shape, noise=x, **kw)


# ------------------------------------------------------------------------------------------------------------------ the plan
def test_plan_ddim10():
    df = diffusion("cosine", "ddim10")
    assert df.guidance_plan() == [R] * 10
    assert df.guidance_plan(guidance_refresh=1) == [R] * 10
    assert df.guidance_plan(guidance_refresh=2) == [R, U] * 5
    assert df.guidance_plan(guidance_refresh=3) == [R, U, U, R, U, U, R, U, U, R]
    assert df.guidance_plan(guidance_refresh=4) == [R, U, U, U, R, U, U, U, R, U]
    assert df.guidance_plan(guidance_refresh=100) == [R] + [U] * 9


def test_plan_with_an_interval():
    """ddim10 under (300, 700): indices 9, 8 unguided, 7 .. 3 guided, 2 .. 0 unguided; only guided calls are counted."""
    df = diffusion("cosine", "ddim10")
    iv = (300, 700)
    assert df.guidance_plan(iv, 1) == [O, O, R, R, R, R, R, O, O, O]
    assert df.guidance_plan(iv, 2) == [O, O, R, U, R, U, R, O, O, O]
    assert df.guidance_plan(iv, 3) == [O, O, R, U, U, R, U, O, O, O]
    for every in (1, 2, 3):
        assert df.guidance_plan((1, 0), every) == [O] * 10                       # the empty interval: nothing to refresh
    # one guided call late in the loop (logsnr10's timestep 5, index 1): it is call n = 0, a refresh
    dl = diffusion("linear", "logsnr10")
    assert dl.guided_steps((5, 5)) == [False, True] + [False] * 8
    assert dl.guidance_plan((5, 5), 2) == [O] * 8 + [R, O]


def test_plan_plms_has_two_calls_in_step_zero():
    df = diffusion("cosine", "ddim10")
    assert df.guidance_plan(plms=True) == [R] * 11
    assert df.guidance_plan(None, 2, plms=True) == [R, U, R, U, R, U, R, U, R, U, R]
    assert df.guidance_plan(None, 3, plms=True) == [R, U, U, R, U, U, R, U, U, R, U]
    # calls at indices 9, 8, 8, 7, ...: under (300, 800) index 8 is guided, 9 is not -- the second call of step 0 is call n = 0
    assert df.guidance_plan((300, 800), 2, plms=True) == [O, R, U, R, U, R, U, R, O, O, O]
    # a loop of one step (skip 9): calls at index 0 and at (0 - 1) mod 10 = 9
    assert df.guidance_plan(None, 2, plms=True, skip_timesteps=9) == [R, U]
    assert df.guidance_plan((900, 999), 2, plms=True, skip_timesteps=9) == [O, R]


def test_plan_with_skip_timesteps():
    df = diffusion("cosine", "ddim10")
    assert df.guidance_plan(None, 2, skip_timesteps=3) == [R, U, R, U, R, U, R]
    assert df.guidance_plan((300, 700), 2, skip_timesteps=3) == [R, U, R, U, O, O, O]       # starts at index 6: guided at once
    assert df.guidance_plan((300, 700), 3, skip_timesteps=4) == [R, U, U, O, O, O]
    assert df.guidance_plan(None, 2, plms=True, skip_timesteps=3) == [R, U, R, U, R, U, R, U]


def test_plan_counts_and_the_restatements_counter():
    """Refreshes = ceil(G / every), on three schedules; and the plan is what the restatement's own counter gives."""
    from test_guidance_interval_host import _full
    for df in (diffusion("cosine", "ddim10"), diffusion("linear", "logsnr10"), diffusion("cosine", [20]), _full()):
        for iv in (None, (300, 700), (1, 0), (0, 0)):
            flags = df.guided_steps(iv)
            for plms in (False, True):
                for skip in (0, 3):
                    for every in (1, 2, 3, 4, 7):
                        plan = df.guidance_plan(iv, every, plms=plms, skip_timesteps=skip)
                        G = len(plan) - plan.count(O)
                        assert len(plan) == len(flags) - skip + (1 if plms else 0)
                        assert plan.count(R) == -(-G // every), (iv, plms, skip, every)
                        assert plan == FR.plan(flags, every, plms, skip)
    for bad in (0, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="guidance_refresh"):
            diffusion("cosine", "ddim10").guidance_plan(None, bad)


# --------------------------------------------------------------------------------------------------------------- the parser
def test_parser_takes_the_flag():
    from gesturediffusion_amd.utils.parser_util import generate_args
    assert generate_args(["--synthetic"]).guidance_refresh == 1
    assert generate_args(["--synthetic", "--guidance_param", "1"]).guidance_refresh == 1
    for sampler in ("p", "ddim", "plms", "dpmpp", "dpmpp_sde"):
        assert generate_args(["--synthetic", "--sampler", sampler, "--guidance_refresh", "2"]).guidance_refresh == 2
    assert generate_args(["--synthetic", "--guidance_refresh", "1"]).guidance_refresh == 1


def test_parser_refusals(capsys):
    from gesturediffusion_amd.utils.parser_util import generate_args
    with pytest.raises(SystemExit):
        generate_args(["--synthetic", "--guidance_refresh", "2", "--guidance_param", "1"])
    assert "--guidance_refresh needs guidance" in capsys.readouterr().err
    with pytest.raises(SystemExit):                        # a model trained without condition dropout: the scale becomes 1
        generate_args(["--synthetic", "--cond_mask_prob", "0", "--guidance_refresh", "2"])
    capsys.readouterr()
    for bad in ("0", "-3"):
        with pytest.raises(SystemExit):
            generate_args(["--synthetic", "--guidance_refresh", bad])
        assert "--guidance_refresh must be at least 1" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        generate_args(["--synthetic", "--guidance_refresh", "2.5"])


def test_sample_chunks_refusals():
    from gesturediffusion_amd.sample.generate import sample_chunks
    args = (None, diffusion("cosine", "ddim10"), torch.zeros(2, 16, 1, 10), None, 1, 20, 10)
    with pytest.raises(ValueError, match="guidance_refresh needs guidance_param"):
        sample_chunks(*args, guidance_param=1.0, guidance_refresh=2)
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="guidance_refresh must be an int"):
            sample_chunks(*args, guidance_param=2.5, guidance_refresh=bad)


# ------------------------------------------------------------------------------------------------------------------- C ABI
def _lib_or_skip():
    from gesturediffusion_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgdx.so not built (run python __graft_entry__.py)")
    return _lib


def test_set_guidance_refresh_refusals():
    _lib = _lib_or_skip()
    lib = _lib.load()
    assert lib.gdx_set_guidance_refresh(None, 2) == -1
    assert b"gdx_set_guidance_refresh: null handle" in lib.gdx_last_error()
    h = C.c_void_p()
    cfg = _lib.Config(arch=1, njoints=16, latent_dim=128, ff_size=256, num_layers=2, num_heads=4, seed_poses=10, mfcc_dim=26,
                      cl_head=8, window=10)
    if lib.gdx_create(C.byref(cfg), C.byref(h)) == 0:          # where a handle can be made without a device
        for bad in (0, -1, -2**31):
            assert lib.gdx_set_guidance_refresh(h, bad) == -1, bad
            assert b"gdx_set_guidance_refresh: every must be at least 1" in lib.gdx_last_error()
        for ok in (1, 2, 4, 2**31 - 1):
            assert lib.gdx_set_guidance_refresh(h, ok) == 0, ok
        lib.gdx_destroy(h)


def test_cfg_delta_refusals_precede_any_hip_call():
    """Every pointer is a made-up non-null address: a refusal that came after a launch could not return cleanly here."""
    _lib = _lib_or_skip()
    lib = _lib.load()
    assert lib.gdx_cfg_delta(None, None) == -1
    assert b"gdx_cfg_delta: null argument" in lib.gdx_last_error()
    good = dict(count=640, a=0x1000, b=0x2000, out=0x3000)
    for name in ("a", "b", "out"):
        args = _lib.CfgDeltaArgs(**dict(good, **{name: None}))
        assert lib.gdx_cfg_delta(C.byref(args), None) == -1, name
        assert b"gdx_cfg_delta: null argument" in lib.gdx_last_error(), name
    for count in (0, -1, -2**40):
        args = _lib.CfgDeltaArgs(**dict(good, count=count))
        assert lib.gdx_cfg_delta(C.byref(args), None) == -1, count
        assert b"gdx_cfg_delta: count must be positive" in lib.gdx_last_error(), count
