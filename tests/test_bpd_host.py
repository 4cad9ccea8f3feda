"""Host-side checks of the variational-bound feature (calc_bpd_loop, gdx_bpd_terms, gdx_bpd_loop): no GPU needed."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import bpd_restatement as R
from conftest import load_golden, weights_from

TINY = dict(njoints=16, nfeats=1, latent_dim=128, ff_size=256, num_layers=2, num_heads=4, seed_poses=10)
CASES = {  # fixture case -> (variance type, mean type, clip_denoised, cfg wrapper, inpainting)
    "small_noclip": ("FIXED_SMALL", "START_X", False, False, False),
    "small_clip": ("FIXED_SMALL", "START_X", True, False, False),
    "large": ("FIXED_LARGE", "START_X", True, False, False),
    "eps": ("FIXED_SMALL", "EPSILON", True, False, False),
    "cfg": ("FIXED_SMALL", "START_X", False, True, False),
    "inpaint": ("FIXED_SMALL", "START_X", True, False, True),
    "lin100": ("FIXED_SMALL", "START_X", True, False, False),
}


def case_schedule(case):
    """(betas of the case's diffusion, respaced index -> model timestep)."""
    from gesturediffusion_amd.diffusion import gaussian_diffusion as gd
    from gesturediffusion_amd.diffusion.respace import space_timesteps
    if case == "lin100":
        return gd.get_named_beta_schedule("linear", 100), list(range(100))
    tmap = sorted(space_timesteps(1000, [20]))
    return R.respaced_betas(gd.get_named_beta_schedule("cosine", 1000), tmap), tmap


def restated_case(arch, case, g, weights):
    """The fixture case recomputed by the fp64 restatement around the oracle's own (torch-CPU) denoiser."""
    from oracle import mdm_forward as omf
    var, mean, clip, wrap, inp = CASES[case]
    betas, tmap = case_schedule(case)
    tab = R.tables(betas, var)
    n1 = 1 if case == "lin100" else None
    x0 = g["x_start"][:n1]
    tape = g["tape100"] if case == "lin100" else g["tape"]
    y = {"seed": torch.from_numpy(g["seed"][:n1]), "mfcc": torch.from_numpy(g["mfcc"][:n1])}
    cfg = dict(TINY, arch=arch)

    def predict(x_t, i):
        x = torch.from_numpy(x_t).float()
        t = torch.full((x.shape[0],), tmap[i], dtype=torch.long)
        with torch.no_grad():
            if wrap:
                yy = dict(y, uncond=True)
                out, out_u = omf.forward(weights, cfg, x, t, y).numpy(), omf.forward(weights, cfg, x, t, yy).numpy()
                return R.blend(out, out_u, g["scale"], clip=clip)
            out = omf.forward(weights, cfg, x, t, y).numpy().astype(np.float64)
        if mean == "EPSILON":
            out = tab["sqrt_recip"][i] * x_t - tab["sqrt_recipm1"][i] * out
        return R.blend(out, mask=g["inpainting_mask"] if inp else None, motion=g["inpainted_motion"] if inp else None,
                       clip=clip)
    return R.loop(tab, x0, tape, predict)


@pytest.mark.parametrize("arch", ["mdm", "mdm_old"])
@pytest.mark.parametrize("case", list(CASES))
def test_restatement_reproduces_reference_fixture(arch, case):
    """The restatement is fp64, so it is held to the reference's fp64 run of each case (same allowances as the GPU tests)."""
    g = load_golden(f"bpd_{arch}_tiny.npz")
    w = weights_from(load_golden(f"loops_{arch}_tiny.npz"))
    R.assert_case(restated_case(arch, case, g, w), g, case, f"restatement-{arch}", against="fp64")


def test_fixture_exercises_both_edge_bins_and_reference_floor_is_recorded():
    for arch in ("mdm", "mdm_old"):
        g = load_golden(f"bpd_{arch}_tiny.npz")
        x = g["x_start"]
        assert (x < -0.999).any() and (x > 0.999).any() and (np.abs(x) < 0.999).any()
        for case in CASES:
            for k in R.OUTS:
                assert g[f"{case}.{k}"].dtype == np.float32 and g[f"{case}.{k}_fp64"].dtype == np.float64
        assert g["lin100.prior_bpd"].min() > 1e3 * g["small_clip.prior_bpd"].max()     # a prior term away from zero
        assert g["kl.loss"].shape == (3,) and np.allclose(g["rkl.loss"], 20 * g["kl.loss"], rtol=1e-6)


@pytest.mark.parametrize("var", ["FIXED_SMALL", "FIXED_LARGE"])
def test_bpd_table_rows_are_fp64_tables_rounded_once(var):
    from gesturediffusion_amd.diffusion import gaussian_diffusion as gd
    from gesturediffusion_amd.diffusion.respace import SpacedDiffusion, space_timesteps
    df = SpacedDiffusion(use_timesteps=space_timesteps(1000, [20]), betas=gd.get_named_beta_schedule("cosine", 1000),
                         model_mean_type=gd.ModelMeanType.START_X, model_var_type=getattr(gd.ModelVarType, var),
                         loss_type=gd.LossType.MSE)
    c = df.bpd_table("cpu").numpy()
    assert c.shape == (20, 8) and c.dtype == np.float32
    tab = R.tables(df.betas, var)
    for col, name in enumerate(("c1", "c2", "log_btilde", "log_sigma2", "sqrt_recip", "sqrt_abar", "sqrt_1m_abar", "sqrt_recipm1")):
        assert np.array_equal(c[:, col].astype(np.float64), tab[name]), name
    # columns 5 / 6 are what q_sample reads from the sampling rows
    from gesturediffusion_amd._lib import GDX_SAMPLER_P
    assert torch.equal(df.bpd_table("cpu")[:, 5:7], df.coef_table(GDX_SAMPLER_P, "cpu")[:, 5:7])
    assert df._prior_log_variance() == float(np.float32(tab["log_1m_abar"][-1]))
    learned = gd.GaussianDiffusion(betas=df.betas, model_mean_type=gd.ModelMeanType.START_X,
                                   model_var_type=gd.ModelVarType.LEARNED_RANGE, loss_type=gd.LossType.KL)
    with pytest.raises(NotImplementedError):
        learned.bpd_table("cpu")


def _lib_or_skip():
    from gesturediffusion_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgdx.so not built (run python __graft_entry__.py)")
    return _lib


def test_bpd_entry_points_refuse_null_arguments_without_gpu():
    _lib = _lib_or_skip()
    lib = _lib.load()
    assert lib.gdx_bpd_terms(None, None) < 0 and b"gdx_bpd_terms" in lib.gdx_last_error()
    assert lib.gdx_bpd_loop(None, C.byref(_lib.BpdLoopArgs()), None) < 0 and b"null handle" in lib.gdx_last_error()
    empty = _lib.BpdArgs()
    assert lib.gdx_bpd_terms(C.byref(empty), None) < 0 and b"null argument" in lib.gdx_last_error()
    h = C.c_void_p()
    cfg = _lib.Config(arch=1, njoints=16, latent_dim=128, ff_size=256, num_layers=2, num_heads=4, seed_poses=10, mfcc_dim=26,
                      cl_head=8, window=10)
    if lib.gdx_create(C.byref(cfg), C.byref(h)) == 0:          # a handle needs no device until weights arrive
        assert lib.gdx_bpd_loop(h, None, None) < 0 and b"null argument" in lib.gdx_last_error()
        assert lib.gdx_bpd_loop(h, C.byref(_lib.BpdLoopArgs()), None) < 0 and b"gdx_prepare" in lib.gdx_last_error()
        lib.gdx_destroy(h)


def test_calc_bpd_loop_has_the_reference_signature():
    import inspect
    from gesturediffusion_amd.diffusion import gaussian_diffusion as gd
    sig = inspect.signature(gd.GaussianDiffusion.calc_bpd_loop)
    assert list(sig.parameters)[:5] == ["self", "model", "x_start", "clip_denoised", "model_kwargs"]
    assert sig.parameters["clip_denoised"].default is True and sig.parameters["model_kwargs"].default is None
    for extra in ("rng", "philox_seed", "sample_offset", "noise_tape", "progress"):
        assert sig.parameters[extra].kind is inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(gd.GaussianDiffusion._vb_terms_bpd)
    assert list(sig.parameters) == ["self", "model", "x_start", "x_t", "t", "clip_denoised", "model_kwargs"]
    assert hasattr(gd.GaussianDiffusion, "_prior_bpd")
    assert sys.modules[gd.__name__] is gd
