"""Host-side checks of the in-library PLMS loop (plms_sample_loop, gdx_plms_step, gdx_plms_loop): no GPU needed."""
import ctypes as C
import inspect
import os

import pytest


def _lib_or_skip():
    from gesturediffusion_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgdx.so not built (run python __graft_entry__.py)")
    return _lib


def _refused(lib, rc, text):
    return rc < 0 and text in lib.gdx_last_error()


def test_plms_step_refusals_without_gpu():
    """gdx_plms_step is stateless: every refusal is decided from the argument struct (addresses are never followed)."""
    _lib = _lib_or_skip()
    lib = _lib.load()
    P = 4096                                            # a non-null address; a refused call reads nothing through it
    assert _refused(lib, lib.gdx_plms_step(None, None), b"null argument")
    assert _refused(lib, lib.gdx_plms_step(C.byref(_lib.PlmsStepArgs()), None), b"null argument")
    ok = dict(kind=2, batch=2, njoints=3, frames=5, coef=P, x=P, x0_cond=P, out=P, eps_out=P)
    step = lambda **kw: lib.gdx_plms_step(C.byref(_lib.PlmsStepArgs(**{**ok, **kw})), None)   # noqa: E731
    for kind in (0, 7, -1):
        assert _refused(lib, step(kind=kind), b"bad kind")
    assert _refused(lib, step(batch=65536), b"bad shape")
    assert _refused(lib, step(x0_uncond=P), b"CFG needs scale")
    assert _refused(lib, step(inpaint_mask=P), b"mask without motion")
    assert _refused(lib, step(kind=2), b"missing history")             # order 2 reads one older eps
    assert _refused(lib, step(kind=1, eps_out=None), b"missing history")
    a = _lib.PlmsStepArgs(**{**ok, "kind": 4})
    a.eps_hist[0] = a.eps_hist[1] = P                                    # order 4 reads three
    assert _refused(lib, lib.gdx_plms_step(C.byref(a), None), b"missing history")
    assert _refused(lib, step(kind=5, eps_out=None), b"missing history")
    a = _lib.PlmsStepArgs(**{**ok, "kind": 5})
    a.eps_hist[0] = P
    assert _refused(lib, lib.gdx_plms_step(C.byref(a), None), b"x_eps and pred_prev")
    assert step(kind=1, batch=0) == 0                                    # nothing to do is not an error


def test_plms_loop_refusals_without_gpu():
    """The argument checks of gdx_plms_loop need no handle: they come first, then the null handle, then the readiness check."""
    _lib = _lib_or_skip()
    lib = _lib.load()
    P = 4096
    ok = dict(mode=0, order=2, num_steps=10, first_index=9, coef=P, timestep_map=P, x=P, eps_hist=P, scratch=P)
    loop = lambda **kw: lib.gdx_plms_loop(None, C.byref(_lib.PlmsLoopArgs(**{**ok, **kw})), None)   # noqa: E731
    assert _refused(lib, lib.gdx_plms_loop(None, None, None), b"null argument")
    for missing in ("coef", "timestep_map", "x"):
        assert _refused(lib, loop(**{missing: None}), b"null argument"), missing
    assert _refused(lib, loop(mode=3), b"bad mode") and _refused(lib, loop(mode=-1), b"bad mode")
    assert _refused(lib, loop(mode=2), b"needs scale")
    for bad in (dict(num_steps=0), dict(first_index=10), dict(first_index=-1), dict(k_base=-1), dict(run_steps=-1),
                dict(first_index=5, k_base=5), dict(first_index=3, run_steps=5)):
        assert _refused(lib, loop(**bad), b"bad step range"), bad
    for order in (0, 1, 5):
        assert _refused(lib, loop(order=order), b"order must be"), order
    assert _refused(lib, loop(inpaint_mask=P), b"mask without motion")
    assert _refused(lib, loop(eps_hist=None), b"missing history") and _refused(lib, loop(scratch=None), b"missing history")
    assert _refused(lib, loop(), b"null handle")               # every argument in order: only the handle is missing
    h = C.c_void_p()
    cfg = _lib.Config(arch=1, njoints=16, latent_dim=128, ff_size=256, num_layers=2, num_heads=4, seed_poses=10, mfcc_dim=26,
                      cl_head=8, window=10)
    if lib.gdx_create(C.byref(cfg), C.byref(h)) == 0:          # where a handle can be made without a device: not prepared
        assert _refused(lib, lib.gdx_plms_loop(h, C.byref(_lib.PlmsLoopArgs(**ok)), None), b"gdx_prepare")
        lib.gdx_destroy(h)


def test_parser_takes_plms_and_its_order():
    from gesturediffusion_amd.utils.parser_util import generate_args
    a = generate_args(["--synthetic", "--sampler", "plms", "--plms_order", "3"])
    assert a.sampler == "plms" and a.plms_order == 3
    assert generate_args(["--synthetic", "--sampler", "plms"]).plms_order == 2
    with pytest.raises(SystemExit):
        generate_args(["--synthetic", "--sampler", "plms", "--plms_order", "5"])
    with pytest.raises(SystemExit):
        generate_args(["--synthetic", "--sampler", "heun"])


def test_plms_sample_loop_keeps_the_reference_signature():
    from gesturediffusion_amd.diffusion import gaussian_diffusion as gd
    sig = inspect.signature(gd.GaussianDiffusion.plms_sample_loop)
    assert list(sig.parameters)[:15] == ["self", "model", "shape", "noise", "clip_denoised", "denoised_fn", "cond_fn",
                                         "model_kwargs", "device", "progress", "skip_timesteps", "init_image",
                                         "randomize_class", "cond_fn_with_grad", "order"]
    assert sig.parameters["order"].default == 2
    for extra, default in (("fused", True), ("rng", "torch"), ("philox_seed", 0), ("sample_offset", 0)):
        assert sig.parameters[extra].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[extra].default == default
