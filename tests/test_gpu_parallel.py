"""Parallel-in-time sampling on the GPU (gdx_window_sweep, gdx_parallel_loop, parallel_sample_loop, sample.generate
--parallel_window; the rule is in include/gdx.h): the fused sweep against n successive gdx_sampler_update launches bit for bit, its
error output against float64, its memory safety; the loop at tolerance 0 against the sequential loops bit for bit, at an infinite
tolerance and at 1e-2 against the CPU restatement (parallel_restatement.py), issued in blocks, on a NaN, under guards, in the
16-bit modes; and the CLI.  Need an MI355X."""
import math
import os

import numpy as np
import pytest
import torch

import parallel_restatement as R
from conftest import rel_err
from oracle import schedule as osch
from test_gpu_dpm import _tiny
from test_gpu_parity import LOOP_TOL, _diffusion, dev
from test_parallel_host import ARCHS, B, tiny_case

pytestmark = pytest.mark.gpu
SENTINEL = 12345.0
CANARY = 64                      # floats behind the last plane
MID = (300, 700)                 # model timesteps of ddim10 are 0, 100, ..., 900: guidance begins at executed step 2, inside a window
SEED = 11


# ---------------------------------------------------------------------------------------------------------------- kernel
def _sweep_case(kind, eta, J, T, Bn, n, first, masked, tape_noise, gen):
    """One gdx_window_sweep launch and the same chain as n gdx_sampler_update launches -> (planes after the sweep [n + 3 planes and
    the canary], the chain's planes, the planes before, err)."""
    from gesturediffusion_amd import engine as E
    d = dev()
    coef = _diffusion("ddim10").coef_table(kind, d, eta)
    shape = (Bn, J, 1, T)
    per = Bn * J * T
    rnd = lambda *s: torch.randn(*s, generator=gen)   # noqa: E731
    before = torch.full(((n + 3) * per + CANARY,), SENTINEL)
    before[:(n + 1) * per] = rnd((n + 1) * per)
    x0 = (1.5 * rnd(n, *shape)).to(d)
    noise = rnd(n, *shape).to(d) if tape_noise else None
    mask = (torch.rand(shape, generator=gen) < 0.3).to(d) if masked else None
    motion = (0.5 * rnd(*shape)).to(d) if masked else None
    buf = before.to(d)
    planes = buf[:(n + 3) * per].view(n + 3, *shape)
    err = E.window_sweep(kind, coef, first, planes, x0, n_slots=n, inpaint_mask=mask, inpaint_motion=motion, clip_denoised=masked,
                         noise=noise, philox_seed=SEED, sample_offset=5, rng_step=3)
    chain = [before[:per].view(shape).to(d)]
    for j in range(n):
        out = torch.empty(shape, device=d)
        E.sampler_update(kind, coef, chain[-1], x0[j], out, step_index=first - j, inpaint_mask=mask, inpaint_motion=motion,
                         noise=noise[j] if tape_noise else None, philox_seed=SEED, sample_offset=5, rng_step=3 + j,
                         clip_denoised=masked)
        chain.append(out)
    return buf.cpu(), torch.stack(chain).cpu(), before, err.cpu()


@pytest.mark.parametrize("kind_name", ["p", "ddim"])
@pytest.mark.parametrize("n", [1, 2, 5])
@pytest.mark.parametrize("Bn", [1, 3])
@pytest.mark.parametrize("J,T", [(7, 5), (16, 20), (33, 128)])
def test_sweep_equals_successive_updates(J, T, Bn, n, kind_name):
    """gdx_window_sweep == n successive gdx_sampler_update launches on the same operands, planes bit-equal.  J*T = 35: the scalar
    path with a ragged last group; 320: the vector path; 4224: more than one GDX_BPD_CHUNK.  DDIM at eta = 0.5.  A window that ends
    at index 0 (first_index = n - 1) and one that does not; with and without an inpainting mask and clip_denoised; tape noise and
    Philox noise.  Plane 0 and everything behind plane n keep their bits (two poisoned planes and a canary behind them).  err ==
    the mean squared change of each plane per sample in float64 numpy, relative 1e-10 (far above J*T * 2^-52)."""
    from gesturediffusion_amd._lib import GDX_SAMPLER_DDIM, GDX_SAMPLER_P
    kind, eta = (GDX_SAMPLER_P, 0.0) if kind_name == "p" else (GDX_SAMPLER_DDIM, 0.5)
    gen = torch.Generator().manual_seed(J * T + 7 * Bn + n)
    per = Bn * J * T
    for first in (n - 1, 9):
        for masked in (False, True):
            for tape_noise in (False, True):
                what = (first, masked, tape_noise)
                after, chain, before, err = _sweep_case(kind, eta, J, T, Bn, n, first, masked, tape_noise, gen)
                assert torch.isfinite(chain).all()
                got = after[:(n + 1) * per].view(n + 1, Bn, J, 1, T)
                assert torch.equal(got.view(torch.int32), chain.view(torch.int32)), what
                assert torch.equal(after[:per].view(torch.int32), before[:per].view(torch.int32)), what          # plane 0 is only read
                assert bool((after[(n + 1) * per:] == SENTINEL).all()), what                                     # nothing behind plane n
                old = before[per:(n + 1) * per].view(n, Bn, -1).double().numpy()
                new = chain[1:].reshape(n, Bn, -1).double().numpy()
                want = ((new - old) ** 2).sum(-1) / (J * T)
                assert err.shape == (n, Bn) and np.all(want > 0)
                assert np.abs(err.numpy() - want).max() <= 1e-10 * want.max(), what
                assert np.all(np.abs(err.numpy() - want) <= 1e-10 * want), what


def test_sweep_misaligned_operands_take_the_scalar_path_with_the_same_bits():
    """Planes one float off 16-byte alignment: the scalar path, the bits of the vector path; a NaN in a plane reaches err."""
    from gesturediffusion_amd import engine as E
    from gesturediffusion_amd._lib import GDX_SAMPLER_P
    d = dev()
    coef = _diffusion("ddim10").coef_table(GDX_SAMPLER_P, d)
    gen = torch.Generator().manual_seed(3)
    n, shape = 3, (2, 16, 1, 20)
    per = 2 * 16 * 20
    start = torch.randn((n + 1) * per, generator=gen)
    x0 = torch.randn(n, *shape, generator=gen).to(d)
    outs = []
    for shift in (0, 1):
        buf = torch.full(((n + 1) * per + 1 + CANARY,), SENTINEL, device=d)
        buf[shift:shift + (n + 1) * per] = start.to(d)
        planes = buf[shift:shift + (n + 1) * per].view(n + 1, *shape)
        assert planes.data_ptr() % 16 == 4 * shift
        err = E.window_sweep(GDX_SAMPLER_P, coef, 9, planes, x0, philox_seed=SEED)
        assert bool((buf[shift + (n + 1) * per:] == SENTINEL).all())
        outs.append((planes.cpu().clone(), err.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    planes = start.to(d).view(n + 1, *shape).clone()
    planes[2, 1, 3, 0, 4] = float("nan")
    err = E.window_sweep(GDX_SAMPLER_P, coef, 9, planes, x0, philox_seed=SEED).cpu()
    assert torch.isnan(err[1, 1]) and torch.isfinite(err[0]).all() and torch.isfinite(err[:, 0]).all()


# ------------------------------------------------------------------------------------------------------------------ loop
COMBOS = [(20, "ddim10"), (10, [40])]
_MODELS = {}


def _model(arch, dtype="fp32"):
    if (arch, dtype) not in _MODELS:
        _MODELS[arch, dtype] = _tiny(arch, dtype)[1]
    return _MODELS[arch, dtype]


def _case(arch, T, resp, variant, dtype="fp32"):
    """(model, y on the device, host case of parallel_restatement, interval, diffusion) of a variant on the first B samples."""
    from gesturediffusion_amd.model.cfg_sampler import ClassifierFreeSampleModel
    df = _diffusion(resp)
    p, cfg, y, tape = tiny_case(arch, T, df.num_timesteps)
    model, interval = _model(arch, dtype), None
    if variant in ("cfg", "interval"):
        y = dict(y, scale=torch.tensor([2.5, -1.0]))
        model = ClassifierFreeSampleModel(model)
    d = dev()
    yd = {k: v.to(d) for k, v in y.items()}
    if variant == "interval":
        yd["guidance_interval"] = interval = MID
    return model, yd, (p, cfg, y, tape), interval, df


def _sequential(df, model, sampler, shape, **kw):
    if sampler == "p":
        return df.p_sample_loop(model, shape, **kw)
    return df.ddim_sample_loop(model, shape, eta=0.5, **kw)


@pytest.mark.parametrize("sampler", ["p", "ddim"])
@pytest.mark.parametrize("variant", ["plain", "cfg", "interval"])
@pytest.mark.parametrize("T,resp", COMBOS)
@pytest.mark.parametrize("arch", ARCHS)
def test_tolerance_0_has_the_bits_of_the_sequential_loop(arch, T, resp, variant, sampler):
    """fp32, tolerance 0, W in {1, 4, 32} (32 exceeds K for ddim10): torch.equal with p_sample_loop / ddim_sample_loop (eta = 0.5)
    under rng="philox", and again under a tape.  Plain, guided at scales (2.5, -1.0), and with a guidance interval that begins
    inside a window.  W = 1 equal but W > 1 not would mean a forward kernel depends on its row count at this shape."""
    model, y, (_, _, _, tape), interval, df = _case(arch, T, resp, variant)
    K = df.num_timesteps
    shape = tuple(tape[0].shape)
    if variant == "interval":
        flags = df.guided_steps(interval)
        first_guided = K - 1 - max(i for i, f in enumerate(flags) if f)
        assert 0 < first_guided < 4 or K > 10                     # ddim10: guidance begins at executed step 2, inside the first window
        assert any(flags) and not all(flags)
    tape_d = tape.to(dev())
    for noise in ("philox", "tape"):
        kw = dict(philox_seed=SEED, sample_offset=3) if noise == "philox" else dict(noise_tape=tape_d)
        want = _sequential(df, model, sampler, shape, clip_denoised=False, model_kwargs={"y": y},
                           **(dict(rng="philox", **kw) if noise == "philox" else kw))
        assert torch.isfinite(want).all()
        for W in (1, 4, 32):
            rep = {}
            got = df.parallel_sample_loop(model, shape, clip_denoised=False, model_kwargs={"y": y}, sampler=sampler, eta=0.5, window=W,
                                          tolerance=0.0, report=rep, **kw)
            assert sum(rep["strides"]) == K and rep["iterations"] == len(rep["strides"]) <= K
            assert torch.equal(got, want), (noise, W, rel_err(got.cpu(), want.cpu()))
            if W == 1:
                assert rep["strides"] == [1] * K


@pytest.mark.parametrize("variant", ["plain", "cfg"])
@pytest.mark.parametrize("T,resp", COMBOS)
@pytest.mark.parametrize("arch", ARCHS)
def test_infinite_tolerance_strides_whole_windows(arch, T, resp, variant):
    """tolerance 1e6: ceil(K / W) iterations, forward_samples = iterations * W * B * (1 or 2) with the ignored tail slots, and the
    sample within LOOP_TOL of the CPU restatement at the same tolerance, where the strides cannot differ."""
    model, y, (p, cfg, y_host, tape), _, df = _case(arch, T, resp, variant)
    K = df.num_timesteps
    tab, tmap = osch.make_tables("cosine", 1000, resp)
    for W in (4, 8):
        rep = {}
        got = df.parallel_sample_loop(model, tuple(tape[0].shape), clip_denoised=False, model_kwargs={"y": y}, sampler="p", window=W,
                                      tolerance=1e6, noise_tape=tape.to(dev()), report=rep)
        want, strides = R.parallel_loop(p, cfg, tab, tmap, tape, y_host, "p", W, 1e6)
        assert rep["iterations"] == math.ceil(K / W) == len(strides) and rep["strides"] == strides
        assert rep["forward_samples"] == rep["iterations"] * W * B * (2 if variant == "cfg" else 1)
        err = rel_err(got.cpu(), want)
        print(f"{arch} T={T} K={K} {variant} W={W}: rel err vs the CPU restatement {err:.3e}")
        assert torch.isfinite(got).all() and err < LOOP_TOL


@pytest.mark.parametrize("variant", ["plain", "cfg"])
@pytest.mark.parametrize("sampler", ["p", "ddim"])
@pytest.mark.parametrize("arch", ARCHS)
def test_tolerance_1e_2_stays_as_close_as_the_restatement(arch, sampler, variant):
    """tolerance 1e-2, W = 8 on the 40-step spacing: ceil(K / W) <= iterations <= K, the strides sum to K, and the deviation from the
    GPU's own sequential sample is at most 4 x the deviation the CPU restatement shows for the same inputs (the project's usual
    margin over a measured spread), plus LOOP_TOL."""
    T, resp, W, tau = 10, [40], 8, 1e-2
    model, y, (p, cfg, y_host, tape), _, df = _case(arch, T, resp, variant)
    K = df.num_timesteps
    shape = tuple(tape[0].shape)
    tab, tmap = osch.make_tables("cosine", 1000, resp)
    seq_cpu, _ = R.parallel_loop(p, cfg, tab, tmap, tape, y_host, sampler, 1, 0.0, eta=0.5)
    par_cpu, strides_cpu = R.parallel_loop(p, cfg, tab, tmap, tape, y_host, sampler, W, tau, eta=0.5)
    dev_cpu = rel_err(par_cpu, seq_cpu)
    tape_d = tape.to(dev())
    seq = _sequential(df, model, sampler, shape, clip_denoised=False, model_kwargs={"y": y}, noise_tape=tape_d)
    rep = {}
    par = df.parallel_sample_loop(model, shape, clip_denoised=False, model_kwargs={"y": y}, sampler=sampler, eta=0.5, window=W,
                                  tolerance=tau, noise_tape=tape_d, report=rep)
    dev_gpu = rel_err(par.cpu(), seq.cpu())
    print(f"{arch} {sampler} {variant}: iterations GPU {rep['iterations']} CPU {len(strides_cpu)} of K = {K}; deviation from the "
          f"sequential sample GPU {dev_gpu:.3e} CPU restatement {dev_cpu:.3e}")
    assert math.ceil(K / W) <= rep["iterations"] <= K and sum(rep["strides"]) == K
    assert all(1 <= s <= W for s in rep["strides"])
    assert torch.isfinite(par).all() and dev_gpu <= 4 * dev_cpu + LOOP_TOL


def _engine_loop(df, model, y, x_T, W, tau, max_iterations, tape=None):
    """gdx_parallel_loop driven through the engine as parallel_sample_loop drives it -> (sample, strides, calls)."""
    from gesturediffusion_amd._lib import GDX_SAMPLER_P
    eng, mode, scale, mask, motion = df._native_loop_setup(model, x_T, {"y": y}, window=W)
    planes = x_T.unsqueeze(0).repeat(W + 1, 1, 1, 1, 1)
    coef, tmap, thr = df.coef_table(GDX_SAMPLER_P, x_T.device), df._timestep_map(), df.parallel_threshold(tau)
    K = df.num_timesteps
    anchor, strides, calls = 0, [], 0
    while anchor < K:
        anchor, s = eng.parallel_loop(planes, GDX_SAMPLER_P, mode, coef, tmap, thr, K - 1, anchor=anchor, scale=scale, inpaint_mask=mask,
                                      inpaint_motion=motion, noise_tape=tape, philox_seed=SEED, max_iterations=max_iterations)
        strides += s
        calls += 1
        assert calls <= K
    return planes[0].clone(), strides, calls


@pytest.mark.parametrize("variant", ["plain", "cfg"])
@pytest.mark.parametrize("arch", ARCHS)
def test_blocks_of_one_iteration_equal_one_call(arch, variant):
    """max_iterations = 1 repeatedly == one call, bit for bit and stride for stride: nothing but the planes and the anchor is
    carried.  At tolerance 1e-2 (data-dependent strides) and with an inpainting mask."""
    model, y, (_, _, _, tape), _, df = _case(arch, 20, "ddim10", variant)
    g = _tiny(arch)[0]
    d = dev()
    y = dict(y, inpainting_mask=torch.from_numpy(g["inpainting_mask"])[:B].contiguous().to(d),
             inpainted_motion=torch.from_numpy(g["inpainted_motion"])[:B].contiguous().to(d))
    x_T = tape[0].to(d)
    whole, strides, calls = _engine_loop(df, model, y, x_T, 4, 1e-2, 0)
    assert calls == 1 and sum(strides) == 10
    blocks, strides_b, calls_b = _engine_loop(df, model, y, x_T, 4, 1e-2, 1)
    assert calls_b == len(strides) and strides_b == strides
    assert torch.isfinite(whole).all() and torch.equal(blocks, whole)
    assert torch.equal(df.parallel_sample_loop(model, tuple(x_T.shape), noise=x_T, clip_denoised=False, model_kwargs={"y": y},
                                               window=4, tolerance=1e-2, philox_seed=SEED), whole)


def test_a_nan_in_x_T_ends_after_k_iterations():
    model, y, (_, _, _, tape), _, df = _case("mdm", 20, "ddim10", "plain")
    x_T = tape[0].to(dev()).clone()
    x_T[1, 3, 0, 5] = float("nan")
    rep = {}
    out = df.parallel_sample_loop(model, tuple(x_T.shape), noise=x_T, clip_denoised=False, model_kwargs={"y": y}, window=4,
                                  tolerance=1e6, report=rep)
    assert rep["iterations"] == 10 and rep["strides"] == [1] * 10
    assert torch.isnan(out[1]).any()


@pytest.mark.parametrize("arch", ARCHS)
def test_guards_report_no_damaged_zone(arch):
    """gdx_set_guards: a canary zone behind every workspace buffer, the loop's own included; a guided window with a rescale."""
    model, y, (_, _, _, tape), _, df = _case(arch, 20, "ddim10", "cfg")
    inner = model.model
    eng = inner._get_engine(dev())
    eng.set_guards(True)
    try:
        rep = {}
        out = df.parallel_sample_loop(model, tuple(tape[0].shape), clip_denoised=False, model_kwargs={"y": dict(y, guidance_rescale=0.7)},
                                      window=4, tolerance=1e-2, philox_seed=SEED, report=rep)
        bad, first = eng.check_guards(dev())
        assert (bad, first) == (0, -1) and torch.isfinite(out).all() and sum(rep["strides"]) == 10
    finally:
        eng.set_guards(False)


def test_library_refuses_refresh_layer_cache_and_a_window_that_does_not_divide():
    from gesturediffusion_amd._lib import GDX_SAMPLER_P, GdxError
    model, y, (_, _, _, tape), _, df = _case("mdm", 20, "ddim10", "cfg")
    x_T = tape[0].to(dev())
    eng, mode, scale, _, _ = df._native_loop_setup(model, x_T, {"y": y}, window=4)
    planes = x_T.unsqueeze(0).repeat(5, 1, 1, 1, 1)
    keep = planes.clone()
    run = lambda p: eng.parallel_loop(p, GDX_SAMPLER_P, mode, df.coef_table(GDX_SAMPLER_P, x_T.device), df._timestep_map(),   # noqa: E731
                                      df.parallel_threshold(0.1), 9, scale=scale)
    eng.set_guidance_refresh(2)
    try:
        with pytest.raises(GdxError, match="guidance refresh"):
            run(planes)
    finally:
        eng.set_guidance_refresh(1)
    eng.set_layer_cache(2, 1)
    try:
        with pytest.raises(GdxError, match="layer cache"):
            run(planes)
    finally:
        eng.set_layer_cache(1, 0)
    with pytest.raises(GdxError, match="does not divide"):
        run(x_T.unsqueeze(0).repeat(4, 1, 1, 1, 1))                    # window 3 on a handle prepared for 4 x 2
    assert torch.equal(planes, keep)                                   # refused before anything ran


# ------------------------------------------------------------------------------------------------------------ 16-bit modes
@pytest.mark.parametrize("name", ["p20", "ddim10_cfg"])
@pytest.mark.parametrize("dtype", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("arch", ARCHS)
def test_compute_modes_against_the_reference_loops(arch, dtype, name):
    """tolerance 0 at W = 4 against the reference's own sequential loop (the golden p20 / ddim10_cfg, recorded tape): fp32 within
    LOOP_TOL, fp16 / bf16 within the modes' stated tolerance (numerics.py), as the sequential 16-bit loop tests hold them."""
    from gesturediffusion_amd.model.cfg_sampler import ClassifierFreeSampleModel
    from gesturediffusion_amd.numerics import stated_tolerance
    g = _tiny(arch)[0]
    d = dev()
    model = _model(arch, dtype)
    y = {"seed": torch.from_numpy(g["seed"]).to(d), "mfcc": torch.from_numpy(g["mfcc"]).to(d)}
    scale = None
    if "cfg" in name:
        y["scale"] = torch.from_numpy(g["scale"]).to(d)
        scale = float(np.abs(g["scale"]).max())
        model = ClassifierFreeSampleModel(model)
    df, sampler = (_diffusion([20]), "p") if name == "p20" else (_diffusion("ddim10"), "ddim")
    tape = torch.from_numpy(g["tape"]).to(d)
    rep = {}
    got = df.parallel_sample_loop(model, tuple(tape[0].shape), clip_denoised=False, model_kwargs={"y": y}, sampler=sampler, window=4,
                                  tolerance=0.0, noise_tape=tape, report=rep)
    tol = LOOP_TOL if dtype == "fp32" else stated_tolerance(dtype, scale)
    err = rel_err(got.cpu(), g[name])
    print(f"{arch} {dtype} {name}: rel err vs the reference's loop {err:.3e} (bound {tol:.3e}), {rep['iterations']} iterations")
    assert sum(rep["strides"]) == df.num_timesteps and err < tol


# --------------------------------------------------------------------------------------------------------------------- CLI
def test_generate_cli_parallel_window_writes_the_bits_of_the_sequential_run(tmp_path, capsys):
    """--parallel_window 4 --parallel_tolerance 0 --sampler ddim --timestep_respacing ddim10 --chunks 2 == the same run without the
    flags, rng philox on both sides; the CLI prints each chunk's iteration count."""
    from gesturediffusion_amd.sample import generate
    base = ["--synthetic", "--latent_dim", "128", "--layers", "2", "--num_samples", "3", "--chunks", "2", "--synthetic_njoints", "37",
            "--seed", "7", "--arch_version", "mdm", "--num_frames", "20", "--sampler", "ddim", "--timestep_respacing", "ddim10",
            "--rng", "philox"]
    res = {}
    for tag, extra in (("seq", []), ("par", ["--parallel_window", "4", "--parallel_tolerance", "0"])):
        out = str(tmp_path / tag)
        assert generate.main(base + extra + ["--output_dir", out]) == 0
        res[tag] = np.load(os.path.join(out, "results.npy"), allow_pickle=True).item()      # written a moment ago
    text = capsys.readouterr().out
    lines = [ln for ln in text.splitlines() if "parallel: " in ln]
    assert len(lines) == 2 and all(ln.endswith("iterations for 10 steps") for ln in lines), text
    assert np.isfinite(res["par"]["motion"]).all() and np.array_equal(res["par"]["motion"], res["seq"]["motion"])
