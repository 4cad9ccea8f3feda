"""Host-side checks of DDIM inversion (gdx_ddim_reverse_step, gdx_ddim_reverse_loop, ddim_reverse_sample_loop, init_is_state,
--invert_gt): no GPU needed.  The restatements live in ddim_reverse_restatement.py."""
import ctypes as C
import os

import pytest
import torch

import ddim_reverse_restatement as R
from conftest import load_golden, rel_err, weights_from
from oracle import schedule as osch
from test_dpm_host import diffusion

TINY = dict(njoints=16, nfeats=1, latent_dim=128, ff_size=256, num_layers=2, num_heads=4, seed_poses=10)
ARCHS = ["mdm", "mdm_old"]

# Full inversion (until = 9) and re-generation on ddim10, tiny fixtures, x_start = tape[0], clip_denoised=False: the restatement's own
# spread -- its fp32 run against the same loop with tables and state in float64 (ddim_reverse_restatement.round_trip, wide=True),
# relative to the largest magnitude of the float64 result.  Measured on the CPU:
#                 latent (state at index 9)    re-generated sample
#     mdm         2.68e-7                      2.15e-4
#     mdm_old     3.85e-7                      1.42e-4
# The latent is ~600 in magnitude (index 0 divides by c1 = 0.0064) and each later step of the way down subtracts it again, which
# is where the sample's three orders of magnitude come from.  The GPU test allows four times the larger figure of each column and
# never less than test_gpu_parity.LOOP_TOL = 2e-4: latent max(4 * 3.86e-7, 2e-4) = 2e-4, sample 4 * 2.16e-4 = 8.64e-4.
SPREAD_LATENT, SPREAD_SAMPLE = 3.86e-7, 2.16e-4
LOOP_TOL = 2e-4
ROUND_TRIP_TOL = {"latent": max(4 * SPREAD_LATENT, LOOP_TOL), "sample": max(4 * SPREAD_SAMPLE, LOOP_TOL)}


def tiny_case(arch):
    """(weights, config, y, x_start, golden) of a tiny fixture on the host."""
    g = load_golden(f"loops_{arch}_tiny.npz")
    y = {"seed": torch.from_numpy(g["seed"]), "mfcc": torch.from_numpy(g["mfcc"])}
    return weights_from(g), dict(TINY, arch=arch), y, torch.from_numpy(g["tape"])[0], g


# ------------------------------------------------------------------------------------------------------------------- C ABI
def _lib_or_skip():
    from gesturediffusion_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgdx.so not built (run python __graft_entry__.py)")
    return _lib


def _refused(lib, rc, text):
    return rc < 0 and text in lib.gdx_last_error()


STEP_PARAMS = ["batch", "njoints", "frames", "coef", "t", "step_index", "x", "x0_cond", "x0_uncond", "scale", "inpaint_mask",
               "inpaint_motion", "clip_denoised", "out", "pred_out", "eps_out", "stream"]
LOOP_PARAMS = ["h", "mode", "num_steps", "first_index", "run_steps", "coef", "timestep_map", "x", "scale", "inpaint_mask",
               "inpaint_motion", "clip_denoised", "stream"]


def test_exports_come_from_the_header():
    """Both entries are declared in gdx.h with plain arguments (the header's set of argument structs is unchanged), so the binding
    derives them like every other export; no noise operand, no RNG among the step's parameters."""
    from gesturediffusion_amd import _lib
    assert "gdx_ddim_reverse_step" in _lib.EXPORTS and "gdx_ddim_reverse_loop" in _lib.EXPORTS
    protos = _lib.HEADER.prototypes
    assert [n for _, n in protos["gdx_ddim_reverse_step"][1]] == STEP_PARAMS
    assert [n for _, n in protos["gdx_ddim_reverse_loop"][1]] == LOOP_PARAMS
    assert protos["gdx_ddim_reverse_step"][0] == protos["gdx_ddim_reverse_loop"][0] == "int"
    assert not {"noise", "philox_seed", "rng_step"} & set(STEP_PARAMS)
    assert len(_lib.SIGNATURES["gdx_ddim_reverse_step"][1]) == 17 and len(_lib.SIGNATURES["gdx_ddim_reverse_loop"][1]) == 13


def test_step_refusals_without_gpu():
    """gdx_ddim_reverse_step is stateless: every refusal is decided from the arguments (addresses are never followed)."""
    _lib = _lib_or_skip()
    lib = _lib.load()
    P, Q, S = 4096, 8192, 12288                         # non-null addresses; a refused call reads nothing through them
    ok = dict(batch=2, njoints=3, frames=5, coef=P, step_index=0, clip_denoised=0, x=P, x0_cond=Q, out=P)
    step = lambda **kw: lib.gdx_ddim_reverse_step(*[{**ok, **kw}.get(n) for n in STEP_PARAMS])   # noqa: E731
    for missing in ("coef", "x", "x0_cond", "out"):
        assert _refused(lib, step(**{missing: None}), b"gdx_ddim_reverse_step: null argument"), missing
    assert _refused(lib, step(batch=65536), b"bad shape") and _refused(lib, step(frames=-1), b"bad shape")
    assert _refused(lib, step(x0_uncond=Q), b"CFG needs scale")
    assert _refused(lib, step(inpaint_mask=Q), b"mask without motion")
    assert _refused(lib, step(pred_out=S, eps_out=S), b"must differ")
    assert _refused(lib, step(pred_out=P), b"must differ") and _refused(lib, step(eps_out=P), b"must differ")
    assert step(batch=0) == 0 and step(frames=0, pred_out=S) == 0       # nothing to do is not an error


def test_loop_refusals_without_gpu():
    """The argument checks of gdx_ddim_reverse_loop need no handle: they come first, then the null handle, then the readiness
    check -- the order of gdx_dpm_loop."""
    _lib = _lib_or_skip()
    lib = _lib.load()
    P = 4096
    ok = dict(mode=0, num_steps=10, first_index=0, run_steps=9, coef=P, timestep_map=P, x=P, clip_denoised=0)
    loop = lambda **kw: lib.gdx_ddim_reverse_loop(*[{**ok, **kw}.get(n) for n in LOOP_PARAMS])   # noqa: E731
    for missing in ("coef", "timestep_map", "x"):
        assert _refused(lib, loop(**{missing: None}), b"gdx_ddim_reverse_loop: null argument"), missing
    assert _refused(lib, loop(mode=3), b"bad mode") and _refused(lib, loop(mode=-1), b"bad mode")
    assert _refused(lib, loop(mode=2), b"needs scale")
    for bad in (dict(run_steps=0), dict(run_steps=-1), dict(run_steps=11), dict(first_index=1, run_steps=10),
                dict(first_index=10, run_steps=1), dict(first_index=-1), dict(num_steps=0)):
        assert _refused(lib, loop(**bad), b"bad step range"), bad
    assert _refused(lib, loop(inpaint_mask=P), b"mask without motion")
    for fine in (dict(), dict(run_steps=10), dict(first_index=9, run_steps=1)):     # every argument in order: only the handle is missing
        assert _refused(lib, loop(**fine), b"null handle"), fine
    h = C.c_void_p()
    cfg = _lib.Config(arch=1, njoints=16, latent_dim=128, ff_size=256, num_layers=2, num_heads=4, seed_poses=10, mfcc_dim=26,
                      cl_head=8, window=10)
    if lib.gdx_create(C.byref(cfg), C.byref(h)) == 0:          # where a handle can be made without a device: not prepared
        assert _refused(lib, loop(h=h), b"gdx_prepare")
        lib.gdx_destroy(h)


# ------------------------------------------------------------------------------------------------------------------ Python
def test_python_refusals_need_no_device():
    from gesturediffusion_amd.model.cfg_sampler import ClassifierFreeSampleModel
    df = diffusion("cosine", "ddim10")
    x = torch.zeros(2, 3, 1, 4)
    for until in (0, 11, -1, 2.0, True):
        with pytest.raises(ValueError, match="until must be"):
            df.ddim_reverse_sample_loop(None, x, until=until)
        with pytest.raises(ValueError, match="until must be"):
            next(df.ddim_reverse_sample_loop_progressive(None, x, until=until))
    with pytest.raises(AssertionError, match="Reverse ODE only for deterministic path"):
        df.ddim_reverse_sample_loop(None, x, eta=0.5)
    with pytest.raises(AssertionError, match="Reverse ODE only for deterministic path"):
        next(df.ddim_reverse_sample_loop_progressive(None, x, eta=0.5))
    guided = object.__new__(ClassifierFreeSampleModel)       # only its type is looked at
    for fused in (True, False):
        with pytest.raises(ValueError, match="guidance_refresh"):
            df.ddim_reverse_sample_loop(guided, x, model_kwargs={"y": {"guidance_refresh": 2}}, fused=fused)
    with pytest.raises(ValueError, match="guidance_refresh"):
        next(df.ddim_reverse_sample_loop_progressive(guided, x, model_kwargs={"y": {"guidance_refresh": 2}}))
    with pytest.raises(ValueError, match="init_image must be None"):
        df.ddim_sample_loop(None, tuple(x.shape), noise=x, init_image=x, skip_timesteps=4, init_is_state=True)
    with pytest.raises(ValueError, match="needs the state"):
        df.ddim_sample_loop(None, tuple(x.shape), skip_timesteps=4, init_is_state=True)
    with pytest.raises(TypeError):                              # keyword-only
        df.ddim_sample_loop(None, tuple(x.shape), x, True, None, None, None, None, False, 0.0, 0, None, False, False, None, False,
                            "torch", 0, 0, None, True, True)


@pytest.mark.parametrize("schedule", ["cosine", "linear"])
@pytest.mark.parametrize("respacing", ["ddim10", "ddim100", [1000]])
def test_reverse_rows_are_the_restatement(schedule, respacing):
    """Columns 0..3 of coef_table(GDX_SAMPLER_DDIM, ., "reverse") are the restatement's rows bit for bit, column 4 (the noise
    weight) is zero, and the last row steps to abar_next = 0: (c2, c3) = (0, 1)."""
    from gesturediffusion_amd._lib import GDX_SAMPLER_DDIM
    df = diffusion(schedule, respacing)
    tab, _ = osch.make_tables(schedule, 1000, respacing)
    got = df.coef_table(GDX_SAMPLER_DDIM, "cpu", "reverse")
    assert got.dtype == torch.float32 and tuple(got.shape) == (df.num_timesteps, 8)
    assert torch.equal(got[:, :4], R.rows_of(tab, "next")) and bool((got[:, 4] == 0).all())
    assert got[-1, 2] == 0 and got[-1, 3] == 1
    assert torch.equal(df.coef_table(GDX_SAMPLER_DDIM, "cpu", 0.0)[:, :4], R.rows_of(tab, "prev"))     # the way back, eta = 0


def test_parser_invert_gt_errors(tmp_path):
    from gesturediffusion_amd.utils.parser_util import generate_args
    data = ["--dataset", "genea2023", "--data_dir", str(tmp_path)]
    a = generate_args(data + ["--sampler", "ddim", "--invert_gt"])
    assert a.invert_gt and a.sampler == "ddim"
    assert not generate_args(data + ["--sampler", "ddim"]).invert_gt
    for bad in (data + ["--invert_gt"],                                   # the default sampler is p
                data + ["--invert_gt", "--sampler", "unipc"],
                ["--synthetic", "--invert_gt", "--sampler", "ddim"],
                ["--synthetic", "--dataset", "genea2023", "--data_dir", str(tmp_path), "--invert_gt", "--sampler", "ddim"],
                ["--dataset", "genea2022", "--data_dir", str(tmp_path), "--invert_gt", "--sampler", "ddim"],
                data + ["--invert_gt", "--sampler", "ddim", "--guidance_refresh", "2"]):
        with pytest.raises(SystemExit):
            generate_args(bad)


def test_sample_chunks_refuses_inversion_for_other_samplers():
    from gesturediffusion_amd.sample.generate import sample_chunks
    seed = torch.zeros(2, 3, 1, 4)
    with pytest.raises(ValueError, match="needs sampler='ddim'"):
        sample_chunks(None, diffusion("cosine", "ddim10"), seed, None, 1, 10, 4, guidance_param=1.0, sampler="p",
                      invert_of_chunk=lambda c: None)


# ------------------------------------------------------------------------------------------------------------- restatements
@pytest.mark.parametrize("arch", ARCHS)
def test_restatements_reproduce_the_reference_golden(arch):
    """Three steps from tape[0] on ddim10 reproduce ddim10_reverse3 (< 2e-5, the bound of test_ddim_reverse_tiny): the oracle's
    loop, and the op-order step the kernel is compared with -- the two are the same arithmetic, so they agree bit for bit."""
    p, cfg, y, x, g = tiny_case(arch)
    tab, tmap = osch.make_tables("cosine", 1000, "ddim10")
    got = R.oracle_loop(p, cfg, tab, tmap, x, y, 3)
    assert rel_err(got, g["ddim10_reverse3"]) < 2e-5
    rows, mapt, xs = R.rows_of(tab, "next"), torch.tensor(tmap), x
    with torch.no_grad():
        for i in range(3):
            t = torch.full((x.shape[0],), i, dtype=torch.long)
            xs = R.step(rows[t], xs, R.x0_of(p, cfg, xs, mapt[t], y))[0]
    assert torch.equal(xs, got)
    assert torch.equal(R.oracle_loop(p, cfg, tab, tmap, R.oracle_loop(p, cfg, tab, tmap, x, y, 2), y, 3, first=2), got)


@pytest.mark.parametrize("arch", ARCHS)
def test_restatement_spread_is_inside_the_gpu_tolerance(arch):
    """Where ROUND_TRIP_TOL comes from (the table above): the spread measured here stays inside the bound the GPU is allowed, and
    the un-clamped state stays finite on these random weights (largest latent magnitude ~6e2), so the GPU case runs with
    clip_denoised=False."""
    p, cfg, y, x, _ = tiny_case(arch)
    tab, tmap = osch.make_tables("cosine", 1000, "ddim10")
    l32, s32 = R.round_trip(p, cfg, tab, tmap, x, y, 9)
    l64, s64 = R.round_trip(p, cfg, tab, tmap, x, y, 9, wide=True)
    assert l32.dtype == torch.float32 and l64.dtype == torch.float64 and torch.isfinite(l32).all() and torch.isfinite(s32).all()
    spread = {"latent": rel_err(l32, l64), "sample": rel_err(s32, s64)}
    print(f"{arch}: max|latent| {float(l32.abs().max()):.1f}, spread latent {spread['latent']:.3e} sample {spread['sample']:.3e}, "
          f"bounds {ROUND_TRIP_TOL}")
    for what in spread:
        assert 0 < spread[what] <= ROUND_TRIP_TOL[what], (what, spread[what])
    assert torch.equal(R.oracle_loop(p, cfg, tab, tmap, x, y, 9), l32)        # the oracle's loop is the same arithmetic


def test_round_trip_converges_for_an_exact_denoiser():
    """The level bookkeeping, checked where the answer is known: data N(0, 0.25 I) with its exact linear denoiser (float64, linear
    schedule).  Inversion to until = n - 1 and ddim_sample back is a first-order scheme, so the round-trip error falls about in
    proportion to the step count -- measured 0.440, 0.248, 0.107, 0.0553 at ddim10 / 20 / 50 / 100 -- and the latent approaches
    unit variance.  Asserted: strictly falling, and at ten times the steps less than a quarter of the error."""
    import dpm_restatement as DR
    x0 = 0.5 * torch.randn(2, 3, 1, 4, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    err, std = {}, {}
    for resp in ("ddim10", "ddim20", "ddim50", "ddim100"):
        tab, _ = osch.make_tables("linear", 1000, resp)
        gain = torch.from_numpy(DR.gaussian_gain(tab.alphas_cumprod, 0.25))
        up, down, n = R.rows_of(tab, "next", torch.float64), R.rows_of(tab, "prev", torch.float64), tab.num_timesteps
        x = x0
        for i in range(n - 1):
            x = R.step(up[[i, i]], x, gain[i] * x)[0]
        std[resp] = float(x.std())
        for i in range(n - 1, -1, -1):
            x = R.step(down[[i, i]], x, gain[i] * x)[0]
        err[resp] = float((x - x0).abs().max() / x0.abs().max())
    print(err, std)
    assert err["ddim10"] > err["ddim20"] > err["ddim50"] > err["ddim100"] > 0
    assert err["ddim100"] < err["ddim10"] / 4
    assert abs(std["ddim100"] - 1) < abs(std["ddim10"] - 1)
