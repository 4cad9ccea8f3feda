"""Layer cache, host side (no GPU): the ValueErrors of y['layer_cache'], the refusal of everything that cannot remember across
calls, GaussianDiffusion.layer_cache_plan against hand-written lists and against the restatement's counter, the parser's flag,
the header's rule and the C exports' refusals before any HIP call."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import layer_cache_restatement as LR
from conftest import REPO
from test_dpm_host import diffusion

F, P = "full", "partial"
MID = (300, 700)         # ddim10: indices 9, 8 unguided, 7 .. 3 guided, 2 .. 0 unguided


# ----------------------------------------------------------------------------------------------------------- the ValueErrors
def test_key_validation():
    from gesturediffusion_amd.engine import layer_cache_of
    assert layer_cache_of({}, 8) == (1, 0)                                             # absent: off
    for ok in ((2, 1), (2, 7), [3, 4], (np.int64(2), np.int32(3)), (1000, 2)):
        got = layer_cache_of({"layer_cache": ok}, 8)
        assert got == (int(ok[0]), int(ok[1])) and all(type(v) is int for v in got)
    for keep in (0, -5, 99, 8):                                                        # every = 1: keep is not looked at
        assert layer_cache_of({"layer_cache": (1, keep)}, 8) == (1, 0)
    for bad in (2, (2,), (2, 1, 1), (True, 1), (2, True), (2.0, 1), (2, 1.0), "21", None, (None, 1), ("2", "1"), {2: 1}):
        with pytest.raises(ValueError, match="two Python ints"):
            layer_cache_of({"layer_cache": bad}, 8)
    for bad in ((0, 1), (-1, 1), (2**31, 1)):
        with pytest.raises(ValueError, match="every"):
            layer_cache_of({"layer_cache": bad}, 8)
    for bad in ((2, 0), (2, 8), (2, -1), (3, 100)):
        with pytest.raises(ValueError, match=r"keep <= num_layers - 1 = 7"):
            layer_cache_of({"layer_cache": bad}, 8)
    with pytest.raises(ValueError, match="num_layers - 1 = 1"):                        # L = 2: keep = 1 only
        layer_cache_of({"layer_cache": (2, 2)}, 2)
    with pytest.raises(ValueError, match="keep"):                                      # L = 1: nothing to cache
        layer_cache_of({"layer_cache": (2, 1)}, 1)
    for bad in (torch.tensor([2, 1]), (torch.tensor(2), 1), [2, torch.tensor(1)]):
        with pytest.raises(ValueError, match="synchronise"):
            layer_cache_of({"layer_cache": bad}, 8)


def test_paths_without_memory_refuse_the_key():
    """every > 1 outside the in-library loops is a ValueError that names the in-library loop; every = 1 and no key pass; the
    key needs no guided model."""
    from gesturediffusion_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    from gesturediffusion_amd.model.cfg_sampler import ClassifierFreeSampleModel
    from gesturediffusion_amd.sampling_options import MEMORY, read

    def refuse(y, num_layers, who):
        read(y, guided=False, num_layers=num_layers, use_text=False, options=MEMORY).refuse_memory(who)
    for lc in ((2, 1), (3, 2), (100, 7)):
        with pytest.raises(ValueError, match="in-library loop") as e:
            refuse({"layer_cache": lc}, 8, "the step-wise forward")
        assert "the step-wise forward" in str(e.value) and f"= ({lc[0]}, {lc[1]})" in str(e.value)
    refuse({"layer_cache": (1, 0)}, 8, "x")
    refuse({}, 8, "x")
    with pytest.raises(ValueError, match="two Python ints"):
        refuse({"layer_cache": 2}, 8, "x")
    guided = object.__new__(ClassifierFreeSampleModel)       # only its type is looked at
    for model in (guided, lambda x, t, **kw: x):
        with pytest.raises(ValueError, match="in-library loop"):
            GaussianDiffusion._refuse_refresh(model, {"y": {"layer_cache": (2, 1)}}, "calc_bpd_loop")
        GaussianDiffusion._refuse_refresh(model, {"y": {"layer_cache": (1, 1)}}, "calc_bpd_loop")
        GaussianDiffusion._refuse_refresh(model, {"y": {}}, "calc_bpd_loop")
        GaussianDiffusion._refuse_refresh(model, None, "calc_bpd_loop")


def test_stepwise_routes_refuse_before_the_first_model_call():
    """calc_bpd_loop, the inversion, a progressive generator, fused=False, denoised_fn and a non-native model with (2, 1):
    ValueError, the model never called."""
    from gesturediffusion_amd.model.cfg_sampler import ClassifierFreeSampleModel
    df = diffusion("cosine", "ddim10")

    class Never(ClassifierFreeSampleModel):
        def __init__(self):                                  # no inner model: nothing here may reach it
            torch.nn.Module.__init__(self)

        def forward(self, *a, **k):
            raise AssertionError("the model was called")

    def plain(xx, t, **k):
        raise AssertionError("the model was called")

    x = torch.zeros(2, 16, 1, 20)
    for m, y in ((Never(), {"layer_cache": (2, 1), "scale": torch.ones(2)}), (plain, {"layer_cache": (2, 1)})):
        kw = dict(model_kwargs={"y": y}, device=torch.device("cpu"))
        for fused in (True, False):
            with pytest.raises(ValueError, match="in-library loop"):
                df.calc_bpd_loop(m, x, model_kwargs={"y": y}, fused=fused)
            with pytest.raises(ValueError, match="in-library loop"):
                df.ddim_reverse_sample_loop(m, x, model_kwargs={"y": y}, fused=fused)
        with pytest.raises(ValueError, match="in-library loop"):
            next(df.ddim_reverse_sample_loop_progressive(m, x, model_kwargs={"y": y}))
        for gen in (df.p_sample_loop_progressive, df.ddim_sample_loop_progressive, df.plms_sample_loop_progressive,
                    df.dpm_solver_sample_loop_progressive, df.dpm_solver_sde_sample_loop_progressive):
            with pytest.raises(ValueError, match="in-library loop"):
                next(gen(m, x.shape, noise=x, **kw))
        for loop in (df.p_sample_loop, df.ddim_sample_loop, df.plms_sample_loop, df.dpm_solver_sample_loop,
                     df.dpm_solver_sde_sample_loop, df.unipc_sample_loop):
            with pytest.raises(ValueError, match="in-library loop"):
                loop(m, x.shape, noise=x, fused=False, **kw)
            with pytest.raises(ValueError, match="in-library loop"):      # routed step-wise by a denoised_fn
                loop(m, x.shape, noise=x, denoised_fn=lambda v: v, **kw)
            with pytest.raises(ValueError, match="in-library loop"):      # ... by a cond_fn
                loop(m, x.shape, noise=x, cond_fn=lambda *a, **k: None, **kw)
    with pytest.raises(ValueError, match="in-library loop"):              # a non-native callable runs step-wise whatever `fused`
        df.p_sample_loop(plain, x.shape, noise=x, model_kwargs={"y": {"layer_cache": (2, 1)}}, device=torch.device("cpu"))


# ------------------------------------------------------------------------------------------------------------------ the plan
def test_plan_ddim10_by_hand():
    df = diffusion("cosine", "ddim10")
    for guided in (True, False):
        assert df.layer_cache_plan((1, 0), guided=guided) == [F] * 10
        assert df.layer_cache_plan((2, 1), guided=guided) == [F, P] * 5
        assert df.layer_cache_plan((3, 5), guided=guided) == [F, P, P, F, P, P, F, P, P, F]
        assert df.layer_cache_plan((100, 1), guided=guided) == [F] + [P] * 9
        assert df.layer_cache_plan((2, 1), guided=guided, plms=True) == [F, P] * 5 + [F]
        assert df.layer_cache_plan((2, 1), guided=guided, skip_timesteps=3) == [F, P, F, P, F, P, F]
        assert df.layer_cache_plan((2, 1), guided=guided, plms=True, skip_timesteps=9) == [F, P]
    # the plan does not depend on keep
    assert df.layer_cache_plan((3, 1)) == df.layer_cache_plan((3, 7))


def test_plan_promotion_and_cfg_serving_cond():
    """The width changes mid-loop under an interval.  ddim10 under (300, 700), modes by call: C C G G G G G C C C.
    every = 3: m = 0 full (K = COND), 1 partial, 2 is GDX_CFG under K = COND: not covered, full -- the promotion, a narrow full
    call followed by a wide call -- 3 full by the count, 4, 5 partial, 6 full, 7 is GDX_COND under K = GDX_CFG: covered, partial
    (the conditional rows of the stored change serve it), 8 partial, 9 full."""
    df = diffusion("cosine", "ddim10")
    assert df.guidance_plan(MID, 1) == ["off"] * 2 + ["refresh"] * 5 + ["off"] * 3
    assert df.layer_cache_plan((3, 1), MID) == [F, P, F, F, P, P, F, P, P, F]
    assert df.layer_cache_plan((2, 1), MID) == [F, P] * 5            # the promotion at m = 2 coincides with the count
    assert df.layer_cache_plan((4, 1), MID) == [F, P, F, P, F, P, P, P, F, P]
    # with the guidance refresh the guided calls alternate GDX_CFG / GDX_COND: modes C C G c G c G C C C
    assert df.guidance_plan(MID, 2) == ["off", "off", "refresh", "reuse", "refresh", "reuse", "refresh", "off", "off", "off"]
    # every = 3: m = 3 is full by the count in GDX_COND (K = COND), so the GDX_CFG call m = 4 is a second promotion
    assert df.layer_cache_plan((3, 1), MID, 2) == [F, P, F, F, F, P, F, P, P, F]
    assert df.layer_cache_plan((4, 1), MID, 2) == [F, P, F, P, F, P, P, P, F, P]
    # no interval, refresh 2: G c G c ...; every = 3: calls 3 and 9 are full GDX_COND calls, so the GDX_CFG calls after them (4)
    # are promotions
    assert df.layer_cache_plan((3, 1), None, 2) == [F, P, P, F, F, P, F, P, P, F]
    # PLMS's second call sits at the index below the first: under (300, 800) index 9 is unguided, 8 guided: C G G G ...
    assert df.layer_cache_plan((4, 1), (300, 800), plms=True) == [F, F, P, P, F, P, P, P, F, P, P]
    # an unguided model ignores the guidance arguments
    assert df.layer_cache_plan((3, 1), MID, 2, guided=False) == [F, P, P, F, P, P, F, P, P, F]


def test_plan_against_the_restatements_counter():
    """every in {1, 2, 3}, intervals that change the width mid-loop, guidance_refresh in {1, 2}, PLMS's second call and
    skip_timesteps, on three schedules: the package's plan is the restatement's."""
    from test_guidance_interval_host import _full
    seen = set()
    for df in (diffusion("cosine", "ddim10"), diffusion("linear", "logsnr10"), diffusion("cosine", [20]), _full()):
        for iv in (None, MID, (1, 0), (0, 0), (300, 800), (500, 999)):
            flags = df.guided_steps(iv)
            for plms in (False, True):
                for skip in (0, 3):
                    for refresh in (1, 2):
                        for guided in (True, False):
                            modes = LR.modes_of(flags, refresh, guided, plms, skip)
                            assert len(modes) == len(flags) - skip + (1 if plms else 0)
                            for every in (1, 2, 3):
                                got = df.layer_cache_plan((every, 1), iv, refresh, guided=guided, plms=plms, skip_timesteps=skip)
                                want = LR.plan(modes, every)
                                assert got == want, (iv, plms, skip, refresh, guided, every)
                                assert got[0] == F and (every > 1 or got == [F] * len(modes))
                                assert got.count(F) >= -(-len(modes) // every)
                                # what the cases must include
                                stored = None
                                for c, what in zip(modes, want):
                                    if what == F and stored == LR.COND and c == LR.CFG:
                                        seen.add("promotion")
                                    if what == P and stored == LR.CFG and c == LR.COND:
                                        seen.add("cfg serves cond")
                                    stored = c if what == F else stored
    assert seen == {"promotion", "cfg serves cond"}
    df = diffusion("cosine", "ddim10")
    assert df.layer_cache_plan((2, 1), guided=False, mode=1) == [F, P] * 5              # GDX_UNCOND throughout
    for bad in (2, (0, 1), (2.0, 1), (True, 1), None, torch.tensor([2, 1])):
        with pytest.raises(ValueError, match="layer_cache"):
            df.layer_cache_plan(bad)


# --------------------------------------------------------------------------------------------------------------- the parser
def test_parser_takes_the_flag():
    from gesturediffusion_amd.utils.parser_util import generate_args
    assert generate_args(["--synthetic"]).layer_cache is None
    for sampler in ("p", "ddim", "plms", "dpmpp", "dpmpp_sde", "unipc"):
        assert generate_args(["--synthetic", "--sampler", sampler, "--layer_cache", "2", "3"]).layer_cache == (2, 3)
    assert generate_args(["--synthetic", "--guidance_param", "1", "--layer_cache", "4", "7"]).layer_cache == (4, 7)   # no guidance needed
    assert generate_args(["--synthetic", "--layers", "2", "--layer_cache", "2", "1"]).layer_cache == (2, 1)
    assert generate_args(["--synthetic", "--layer_cache", "1", "99"]).layer_cache is None                             # off


def test_parser_refusals(capsys):
    from gesturediffusion_amd.utils.parser_util import generate_args
    for bad in ("0", "-3"):
        with pytest.raises(SystemExit):
            generate_args(["--synthetic", "--layer_cache", bad, "1"])
        assert "--layer_cache EVERY must be at least 1" in capsys.readouterr().err
    for keep in ("0", "8", "-1"):
        with pytest.raises(SystemExit):
            generate_args(["--synthetic", "--layer_cache", "2", keep])
        assert "--layer_cache KEEP must lie in 1 .. layers - 1 = 7" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        generate_args(["--synthetic", "--layers", "2", "--layer_cache", "2", "2"])
    assert "layers - 1 = 1" in capsys.readouterr().err
    for argv in (["--layer_cache", "2"], ["--layer_cache", "2.5", "1"], ["--layer_cache", "2", "1", "1"]):
        with pytest.raises(SystemExit):
            generate_args(["--synthetic", *argv])
    capsys.readouterr()
    with pytest.raises(SystemExit):
        generate_args(["--dataset", "genea2023", "--data_dir", "/nonexistent", "--sampler", "ddim", "--invert_gt",
                       "--layer_cache", "2", "1"])
    assert "--invert_gt runs no layer cache" in capsys.readouterr().err


def test_sample_chunks_refuses_the_cache_with_an_inversion():
    from gesturediffusion_amd.sample.generate import sample_chunks
    args = (None, diffusion("cosine", "ddim10"), torch.zeros(2, 16, 1, 10), None, 1, 20, 10)
    with pytest.raises(ValueError, match="invert_of_chunk runs no layer cache"):
        sample_chunks(*args, sampler="ddim", invert_of_chunk=lambda c: None, layer_cache=(2, 1))


# ------------------------------------------------------------------------------------------------------------- the header
def test_header_states_the_rule_at_the_setter():
    hdr = open(os.path.join(REPO, "include", "gdx.h")).read()
    rule = hdr[hdr.index("int gdx_forward_samples("):hdr.index("int gdx_set_layer_cache(")]
    for phrase in ("m % every == 0", "covers(K, c)", "ALL denoiser calls", "second call of gdx_plms_loop", "fl32(out[b,t,j] - in[b,t+1,j])",
                   "fl32(in'[b,t+1,j] + delta[b,t,j])", "rows 0 .. B-1", "not launched", "token-major", "block-wise",
                   "No counter lives in the", "gdx_bpd_loop", "gdx_ddim_reverse_loop", "eagerly", "trained", "1 .. num_layers - 1",
                   "before its first launch", "gdx_set_condition_text"):
        assert phrase in rule, phrase
    tap = hdr[hdr.index("Debug/parity taps"):hdr.index("int gdx_set_keep_taps(")]
    assert "which = L + 1" in tap and "stale" in tap


# ------------------------------------------------------------------------------------------------------------------- C ABI
def _lib_or_skip():
    from gesturediffusion_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgdx.so not built (run python __graft_entry__.py)")
    return _lib


def test_setter_and_counter_refusals():
    _lib = _lib_or_skip()
    lib = _lib.load()
    assert lib.gdx_set_layer_cache(None, 2, 1) == -1
    assert b"gdx_set_layer_cache: null handle" in lib.gdx_last_error()
    n = C.c_int64()
    assert lib.gdx_forward_layer_samples(None, C.byref(n)) == -1
    assert b"gdx_forward_layer_samples: null argument" in lib.gdx_last_error()
    h = C.c_void_p()
    cfg = _lib.Config(arch=1, njoints=16, latent_dim=128, ff_size=256, num_layers=4, num_heads=4, seed_poses=10, mfcc_dim=26,
                      cl_head=8, window=10)
    if lib.gdx_create(C.byref(cfg), C.byref(h)) == 0:          # where a handle can be made without a device
        assert lib.gdx_forward_layer_samples(h, None) == -1
        assert lib.gdx_forward_layer_samples(h, C.byref(n)) == 0 and n.value == 0
        for bad in (0, -1, -2**31):
            assert lib.gdx_set_layer_cache(h, bad, 1) == -1, bad
            assert b"gdx_set_layer_cache: every must be at least 1" in lib.gdx_last_error()
        for keep in (0, 4, -1, 100):
            assert lib.gdx_set_layer_cache(h, 2, keep) == -1, keep
            assert b"gdx_set_layer_cache: keep must lie in 1 .. num_layers - 1 = 3" in lib.gdx_last_error()
            assert lib.gdx_set_layer_cache(h, 1, keep) == 0, keep                      # every = 1: keep is not looked at
        for ok in ((2, 1), (2, 3), (2**31 - 1, 2), (1, 0)):
            assert lib.gdx_set_layer_cache(h, *ok) == 0, ok
        lib.gdx_destroy(h)


def test_layer_delta_refusals_precede_any_hip_call():
    """Every pointer is a made-up non-null address: a refusal that came after a launch could not return cleanly here."""
    _lib = _lib_or_skip()
    lib = _lib.load()
    f32, f16, bf16 = _lib.GDX_DTYPE_F32, _lib.GDX_DTYPE_F16, _lib.GDX_DTYPE_BF16
    good = dict(op=0, in_dtype=f32, out_dtype=f32, batch=2, frames=10, width=128, inp=0x1000, outc=0x2000, delta=0x3000)

    def call(**kw):
        a = dict(good, **kw)
        return lib.gdx_layer_delta(a["op"], a["in_dtype"], a["out_dtype"], a["batch"], a["frames"], a["width"], a["inp"], a["outc"],
                                   a["delta"], None)
    for op in (-1, 2, 7):
        assert call(op=op) == -1 and b"op must be 0 (store) or 1 (apply)" in lib.gdx_last_error()
    for pair in ((f16, f32), (f32, f16), (f16, bf16), (bf16, bf16), (bf16, f32), (bf16, f16), (f32, 3), (-1, f32), (7, 7)):
        assert call(in_dtype=pair[0], out_dtype=pair[1]) == -1, pair
        assert b"(fp32, fp32), (fp16, fp16) or (fp32, bf16)" in lib.gdx_last_error(), pair
    for op in (0, 1):
        for pair in ((f32, f32), (f16, f16), (f32, bf16)):
            ok = dict(op=op, in_dtype=pair[0], out_dtype=pair[1])
            for name in ("batch", "frames", "width"):
                for v in (0, -1):
                    assert call(**ok, **{name: v}) == -1 and b"must be positive" in lib.gdx_last_error(), (name, v)
            for width in (1, 8, 16, 48, 100, 127, 129):
                assert call(**ok, width=width) == -1 and b"width must be a multiple of 32" in lib.gdx_last_error(), width
            for name in ("inp", "outc", "delta"):
                assert call(**ok, **{name: None}) == -1 and b"gdx_layer_delta: null argument" in lib.gdx_last_error(), name
                for off in (2, 4, 8):
                    assert call(**ok, **{name: good[name] + off}) == -1, (name, off)
                    assert b"16-byte aligned" in lib.gdx_last_error(), (name, off)
