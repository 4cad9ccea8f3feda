"""SDE-DPM-Solver++ multistep sampling on the GPU (gdx_dpm_sde_step, gdx_dpm_sde_loop, dpm_solver_sde_sample{,_loop};
include/gdx.h): the fused noisy step against its op order in torch fp32, the in-library loop against the step-wise protocol bit
for bit under every noise source, eta = 0 against the ODE solver, order 1 at eta = 1 against p_sample, the analytic Gaussian
case against the fp64 restatement (dpm_sde_restatement.py) both deterministically and statistically, workspace guards and the
CLI.  The constants come from test_dpm_sde_host.py, where they are measured on the CPU."""
import itertools

import numpy as np
import pytest
import torch

import dpm_sde_restatement as S
from misaligned import shifted as _shifted
from test_dpm_host import S2, analytic_x_T, diffusion
from test_dpm_sde_host import (FP32_LOOP_TOL, P_SAMPLE_BOUND_UNITS, STAT_BOUND, STAT_SEED, STAT_SHAPE, analytic_tape,
                               p_sample_bound_unit, stat_prediction)
from test_gpu_dpm import ARCHS, B, VARIANTS, _tiny, _torch_step, _variant
from test_gpu_parity import dev

pytestmark = pytest.mark.gpu
SEED, OFFSET = 1234, 5


# ---------------------------------------------------------------------------------------------------------------- kernel
@pytest.mark.parametrize("J,T,shift", [(3, 4, False), (3, 5, False), (13, 80, False), (3, 4, True)])
@pytest.mark.parametrize("order", [1, 2])
def test_dpm_sde_step_bit_exact(order, J, T, shift):
    """gdx_dpm_sde_step == (a*x + D) + s*z in torch, one op per rounding, by torch.equal on out and pred_out.  J*T = 12 takes the
    128-bit path, 15 the scalar path with a 3-element tail group, 1040 = 260 groups a second block in x, and 12 with x and the
    tape one float off alignment the scalar path again.  z from a tape and from the in-kernel Philox draw (then the torch side
    takes it from engine.randn with the same seed, sample offset and draw); per-sample t and step_index; plain, CFG with two
    scales, CFG + inpainting + clamp; out aliasing x.  The history slot order 1 does not read holds NaN."""
    from gesturediffusion_amd import engine as E
    d = dev()
    coef = diffusion("linear", "logsnr20").dpm_sde_coef_table(d, 1.0)
    assert coef.shape[0] >= 10 and bool((coef[[3, 5, 7]][:, [0, 1, 2, 3, 7]] != 0).all())
    g = torch.Generator().manual_seed(100 * order + J * T)
    shape = (B, J, 1, T)
    rnd = lambda s=1.0: (torch.randn(shape, generator=g) * s).to(d)   # noqa: E731
    x, oc, ou, motion, m1, tape = rnd(), rnd(1.5), rnd(1.5), rnd(0.5), rnd(1.5), rnd()
    mask = (torch.rand(shape, generator=g) < 0.3).to(d)
    scale = torch.tensor([2.5, -1.0], device=d)
    hist_in = [m1 if order == 2 else torch.full(shape, float("nan"), device=d)]
    t_rows = torch.tensor([3, 7], device=d)
    z_philox = E.randn(shape, d, SEED, OFFSET, 9)
    ran = 0
    for (cfg, inp, clip), (t_mode, alias), philox in itertools.product(
            [(False, False, False), (True, False, False), (True, True, True)], [("t", False), (5, True)], [False, True]):
        kw_t = dict(t=t_rows) if t_mode == "t" else dict(step_index=t_mode)
        rows = coef[t_rows] if t_mode == "t" else coef[[t_mode, t_mode]]
        ops = dict(ou=ou if cfg else None, scale=scale if cfg else None, mask=mask if inp else None, motion=motion if inp else None)
        base, want_pred = _torch_step(order, rows, x, oc, ops["ou"], ops["scale"], ops["mask"], ops["motion"], clip, [m1])
        z = z_philox if philox else tape
        want_out = base + rows[:, 7].view(-1, 1, 1, 1) * z
        xin = _shifted(x.clone()) if shift else x.clone()
        out = xin if alias else torch.empty_like(x)
        pred = torch.empty_like(x)
        kw_z = dict(philox_seed=SEED, sample_offset=OFFSET, rng_step=9) if philox else dict(noise=_shifted(tape) if shift else tape)
        E.dpm_sde_step(order, coef, xin, oc, out, hist=hist_in, x0_uncond=ops["ou"], scale=ops["scale"], inpaint_mask=ops["mask"],
                       inpaint_motion=ops["motion"], clip_denoised=clip, pred_out=pred, **kw_t, **kw_z)
        tag = (order, J, T, shift, cfg, inp, clip, t_mode, alias, philox)
        for name, got, ref in (("out", out, want_out), ("pred", pred, want_pred)):
            assert torch.isfinite(got).all(), (name, tag)
            assert torch.equal(got, ref), (name, tag)
        assert not torch.equal(out, base), tag                            # the noise term is there
        ran += 1
    assert ran == 12


def test_philox_noise_does_not_depend_on_the_batch():
    """Sample b of a B = 3 call at sample_offset o equals sample 0 of a B = 1 call at sample_offset o + b."""
    from gesturediffusion_amd import engine as E
    d = dev()
    coef = diffusion("linear", "logsnr20").dpm_sde_coef_table(d, 1.0)
    g = torch.Generator().manual_seed(8)
    x, oc, m1 = ((torch.randn(3, 13, 1, 20, generator=g)).to(d) for _ in range(3))
    kw = dict(step_index=6, philox_seed=SEED, rng_step=4)
    for order in (1, 2):
        whole = E.dpm_sde_step(order, coef, x, oc, torch.empty_like(x), hist=[m1], sample_offset=OFFSET, **kw)
        for b in range(3):
            one = E.dpm_sde_step(order, coef, x[b:b + 1].contiguous(), oc[b:b + 1].contiguous(), torch.empty_like(x[:1]),
                                 hist=[m1[b:b + 1].contiguous()], sample_offset=OFFSET + b, **kw)
            assert torch.equal(whole[b:b + 1], one), (order, b)
        assert not torch.equal(whole[0], whole[1])


def test_dpm_sde_step_row_zero_returns_the_prediction():
    """Row 0 is (0, 1, 0, ..., 0): the step to sigma = 0 returns the (clamped) prediction itself, whatever x and the noise hold."""
    from gesturediffusion_amd import engine as E
    d = dev()
    coef = diffusion("cosine", "ddim10").dpm_sde_coef_table(d, 1.0)
    g = torch.Generator().manual_seed(3)
    x, oc, z = ((torch.randn(2, 16, 1, 20, generator=g) * 2).to(d) for _ in range(3))
    for kw in (dict(noise=z), dict(philox_seed=SEED, rng_step=10)):
        out, pred = torch.empty_like(x), torch.empty_like(x)
        E.dpm_sde_step(1, coef, x, oc, out, step_index=0, clip_denoised=True, pred_out=pred, **kw)
        assert torch.equal(pred, oc.clamp(-1, 1)) and torch.equal(out, pred)


# ------------------------------------------------------------------------------------------------------------------ loop
def _tape(g, n, seed=21):
    """A noise tape of n + 1 entries (entry 0 = x_T) for the first B samples of the tiny fixtures' shape."""
    shape = tuple(torch.from_numpy(g["tape"])[0, :B].shape)
    return torch.randn(n + 1, *shape, generator=torch.Generator().manual_seed(seed)).to(dev())


NOISE = ["tape", "philox", "torch"]


def _noise_kw(source, tape):
    if source == "tape":
        return dict(noise_tape=tape)
    if source == "philox":
        return dict(rng="philox", philox_seed=SEED, sample_offset=OFFSET)
    return dict(rng="torch")


def _run(df, model, shape, source, kw, **extra):
    if source == "torch":
        torch.manual_seed(4321)
    return df.dpm_solver_sde_sample_loop(model, shape, **kw, **extra)


def _hand_loop(df, model, tape, y, order, eta, clip_denoised=False, skip_timesteps=0, init_image=None):
    """The loop written out over dpm_solver_sde_sample with a tape, as a caller of the step-wise protocol would."""
    idx = list(range(df.num_timesteps - skip_timesteps))[::-1]
    img = tape[0]
    if init_image is not None:
        img = df.q_sample(init_image, torch.full((img.shape[0],), idx[0], device=img.device, dtype=torch.long), img)
    old = None
    for k, i in enumerate(idx):
        t = torch.full((img.shape[0],), i, device=img.device, dtype=torch.long)
        old = df.dpm_solver_sde_sample(model, img, t, clip_denoised=clip_denoised, model_kwargs={"y": y}, order=order, eta=eta,
                                       old_out=old, noise=tape[1 + k])
        assert len(old["old_pred"]) <= order - 1
        img = old["sample"]
    return img


def _count_calls(monkeypatch):
    from gesturediffusion_amd.engine import Engine
    calls = {"dpm_sde_loop": 0, "forward": 0}
    for name in calls:
        orig = getattr(Engine, name)

        def counted(self, *a, _orig=orig, _name=name, **k):
            calls[_name] += 1
            return _orig(self, *a, **k)
        monkeypatch.setattr(Engine, name, counted)
    return calls


@pytest.mark.parametrize("arch", ARCHS)
@pytest.mark.parametrize("resp", ["ddim10", "logsnr20"])
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("eta", [0.5, 1.0])
def test_fused_loop_equals_stepwise_bit_for_bit(arch, resp, order, eta, monkeypatch):
    """dpm_solver_sde_sample_loop(fused=True) == fused=False on the tiny V1 / V2 under a tape, Philox and torch's generator
    (re-seeded per route), and == a hand loop over dpm_solver_sde_sample under the tape: conditional, CFG, inpainting,
    clip_denoised, init_image + skip_timesteps=3 and the single-step loop; the fused route is one gdx_dpm_sde_loop call and no
    step-wise forward, the step-wise route one denoiser call per step."""
    g, m = _tiny(arch)
    df = diffusion("cosine", resp)
    n = df.num_timesteps
    tape = _tape(g, n)
    shape = tuple(tape.shape[1:])
    calls = _count_calls(monkeypatch)
    results = {}
    for name, source in itertools.product(VARIANTS, NOISE):
        model, y, kw = _variant(name, g, m, n)
        kw = dict(kw, model_kwargs={"y": y}, order=order, eta=eta, **_noise_kw(source, tape))
        steps = n - kw.get("skip_timesteps", 0)
        calls.update(dpm_sde_loop=0, forward=0)
        fused = _run(df, model, shape, source, kw)
        assert calls == {"dpm_sde_loop": 1, "forward": 0}, (name, source, calls)
        step = _run(df, model, shape, source, kw, fused=False)
        assert calls == {"dpm_sde_loop": 1, "forward": steps}, (name, source, calls)
        assert torch.isfinite(fused).all() and torch.equal(fused, step), (name, source)
        if source == "tape":
            hand = _hand_loop(df, model, tape, y, order, eta, kw["clip_denoised"], kw.get("skip_timesteps", 0), kw.get("init_image"))
            assert torch.equal(fused, hand), name
        results[name, source] = fused
    assert not torch.equal(results["cond", "tape"], results["cond", "philox"])           # the noise reaches the sample
    assert not torch.equal(results["cond", "tape"], results["cond", "torch"])


@pytest.mark.parametrize("arch", ARCHS)
@pytest.mark.parametrize("run_steps", [1, 3])
def test_one_call_equals_blockwise_issue(arch, run_steps, monkeypatch):
    """run_steps / k_base: the loop issued in blocks of 1 or 3 steps (progress=True) carries its history in the caller's buffer,
    takes tape slice / Philox draw / generator draw k of executed step k, and gives the bits of one call."""
    from gesturediffusion_amd.diffusion import gaussian_diffusion as gd
    g, m = _tiny(arch)
    for resp, name, order, source in [("logsnr20", "cfg", 2, "tape"), ("ddim10", "cond", 2, "philox"), ("ddim10", "inpaint", 2, "torch"),
                                      ("logsnr20", "init_skip3", 2, "philox"), ("ddim10", "cond", 1, "tape")]:
        df = diffusion("cosine", resp)
        tape = _tape(g, df.num_timesteps)
        shape = tuple(tape.shape[1:])
        model, y, kw = _variant(name, g, m, df.num_timesteps)
        kw = dict(kw, model_kwargs={"y": y}, order=order, eta=1.0, **_noise_kw(source, tape))
        one = _run(df, model, shape, source, kw)
        calls = _count_calls(monkeypatch)
        monkeypatch.setattr(gd, "NOISE_BLOCK", run_steps)
        blocks = _run(df, model, shape, source, kw, progress=True)
        monkeypatch.undo()
        assert calls["dpm_sde_loop"] == -(-(df.num_timesteps - kw.get("skip_timesteps", 0)) // run_steps)
        assert torch.equal(one, blocks), (resp, name, order, source)


@pytest.mark.parametrize("order", [1, 2])
def test_eta_zero_is_the_ode_solver(order):
    """At eta = 0 the rows are dpm_coef_table's and s = 0: the loop gives dpm_solver_sample_loop's sample from the same x_T,
    through the library loops and through the step entry points (gdx_dpm_sde_step / gdx_dpm_step, fused=False) alike -- the
    noisy and the noise-free instantiations of the one step kernel agree."""
    g, m = _tiny("mdm")
    df = diffusion("cosine", "logsnr20")
    tape = _tape(g, df.num_timesteps)
    model, y, kw = _variant("cfg", g, m, df.num_timesteps)
    kw = dict(kw, model_kwargs={"y": y}, order=order)
    ode = df.dpm_solver_sample_loop(model, tuple(tape.shape[1:]), noise=tape[0].clone(), **kw)
    sde = df.dpm_solver_sde_sample_loop(model, tuple(tape.shape[1:]), eta=0.0, noise_tape=tape, **kw)
    assert torch.isfinite(sde).all() and torch.equal(sde, ode)
    ode_step = df.dpm_solver_sample_loop(model, tuple(tape.shape[1:]), noise=tape[0].clone(), fused=False, **kw)
    sde_step = df.dpm_solver_sde_sample_loop(model, tuple(tape.shape[1:]), eta=0.0, noise_tape=tape, fused=False, **kw)
    assert torch.equal(sde_step, ode_step) and torch.equal(sde_step, sde)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_fused_equals_stepwise_in_the_16_bit_modes(dtype):
    """Both routes use the same forward, so the bits stay equal under compute_dtype fp16 / bf16."""
    g, m = _tiny("mdm", dtype)
    df = diffusion("cosine", "logsnr20")
    tape = _tape(g, df.num_timesteps)
    model, y, kw = _variant("cfg", g, m, df.num_timesteps)
    kw = dict(kw, model_kwargs={"y": y}, order=2, eta=1.0, noise_tape=tape)
    fused = df.dpm_solver_sde_sample_loop(model, tuple(tape.shape[1:]), **kw)
    step = df.dpm_solver_sde_sample_loop(model, tuple(tape.shape[1:]), fused=False, **kw)
    assert torch.isfinite(fused).all() and torch.equal(fused, step)


def test_fused_loop_leaves_the_workspace_guards_intact():
    g, m = _tiny("mdm")
    d = dev()
    df = diffusion("cosine", "logsnr20")
    tape = _tape(g, df.num_timesteps)
    eng = m._get_engine(d)
    eng.set_guards(True)
    try:
        model, y, kw = _variant("cfg", g, m, df.num_timesteps)
        for source in NOISE:
            r = _run(df, model, tuple(tape.shape[1:]), source, dict(kw, model_kwargs={"y": y}, order=2, **_noise_kw(source, tape)))
            bad, zone = eng.check_guards(d)
            assert bad == 0, f"{source}: {bad} canary bytes overwritten, first in workspace allocation #{zone}"
            assert torch.isfinite(r).all()
    finally:
        eng.set_guards(False)


def test_refusals_come_before_the_library_is_called(monkeypatch):
    g, m = _tiny("mdm")
    df = diffusion("cosine", "ddim10")
    model, y, kw = _variant("cond", g, m, 10)
    tape = _tape(g, 10)
    calls = _count_calls(monkeypatch)
    for bad in (dict(order=0), dict(order=3), dict(eta=-1.0)):
        with pytest.raises(ValueError, match="order is invalid|eta must be"):
            df.dpm_solver_sde_sample_loop(model, tuple(tape.shape[1:]), noise_tape=tape, model_kwargs={"y": y}, **bad, **kw)
    t = torch.tensor([3, 4], device=dev())
    with pytest.raises(ValueError, match="same for the whole batch"):
        df.dpm_solver_sde_sample(model, tape[0], t, model_kwargs={"y": y})
    assert calls == {"dpm_sde_loop": 0, "forward": 0}


# ------------------------------------------------------------------------------------------- order 1, eta = 1 against p_sample
def test_order_one_at_eta_one_is_the_ancestral_step():
    """One step on the same x, model output and noise at t in {5, 9} of ddim10: dpm_solver_sde_sample(order=1, eta=1) and p_sample
    (FIXED_SMALL) are two fp32 evaluations of one real number, so they differ by at most P_SAMPLE_BOUND_UNITS = 4.8 units of
    p_sample_bound_unit (test_dpm_sde_host.py: twice the 2.4 units either op order keeps to the fp64 value on the CPU);
    pred_xstart is bit-equal.  p_sample draws its noise from torch's generator: the same seed gives the step the same z."""
    d = dev()
    df = diffusion("cosine", "ddim10")
    sde, rows = df.dpm_sde_coef_table(d, 1.0), torch.from_numpy(df.dpm_sde_coef_rows(1.0)).to(d)
    g = torch.Generator().manual_seed(12)
    for t in (5, 9):
        tt = torch.full((B,), t, device=d, dtype=torch.long)
        x, m0 = torch.randn(B, 16, 1, 20, generator=g).to(d), (torch.randn(B, 16, 1, 20, generator=g) * 1.5).to(d)
        model = lambda xx, ts, y: m0   # noqa: E731
        torch.manual_seed(70 + t)
        b = df.p_sample(model, x, tt, clip_denoised=False, model_kwargs={"y": {}})
        torch.manual_seed(70 + t)
        z = torch.randn_like(x)
        a = df.dpm_solver_sde_sample(model, x, tt, clip_denoised=False, model_kwargs={"y": {}}, order=1, eta=1.0, noise=z)
        assert torch.equal(a["pred_xstart"], b["pred_xstart"]) and torch.equal(a["pred_xstart"], m0)
        unit = p_sample_bound_unit(sde[tt], x, m0, z)
        ratio = float(((a["sample"].double() - b["sample"].double()).abs() / unit.clamp_min(1e-300)).max())
        v64 = rows[t, 0] * x.double() + rows[t, 1] * m0.double() + rows[t, 7] * z.double()
        own = float(((a["sample"].double() - v64).abs() / unit.clamp_min(1e-300)).max())
        print(f"t={t}: order 1 vs p_sample {ratio:.3f} units (bound {P_SAMPLE_BOUND_UNITS}); order 1 vs fp64 {own:.3f}")
        assert ratio <= P_SAMPLE_BOUND_UNITS, (t, ratio)
        assert own <= P_SAMPLE_BOUND_UNITS / 2, (t, own)


# ------------------------------------------------------------------------------------------------------ analytic Gaussian case
def _exact_denoiser(d):
    from gesturediffusion_amd.diffusion import gaussian_diffusion as gd
    abar_orig, _ = S.schedule(gd.get_named_beta_schedule("linear", 1000))
    gain = torch.from_numpy(S.gaussian_gain(abar_orig, S2)).float().to(d)
    return lambda x, t, y: gain[t].view(-1, 1, 1, 1) * x   # noqa: E731


def test_analytic_gaussian_case_matches_the_fp64_restatement():
    """Data N(0, 0.25 I) with its exact linear denoiser as a Python callable on the ORIGINAL timestep, through the step-wise route
    with a tape: linear schedule, logsnr20 / logsnr40, orders 1..2, eta = 1.  The result agrees with the fp64 restatement run on
    the same x_T and tape within FP32_LOOP_TOL = 8.48e-7 (4x the worst error of the restatement's own recurrence in torch fp32
    on the CPU, 2.12e-7: test_dpm_sde_host.py)."""
    d = dev()
    x_T = analytic_x_T()
    model = _exact_denoiser(d)
    for sp in ("logsnr20", "logsnr40"):
        df = diffusion("linear", sp)
        ab, abp = df.alphas_cumprod, df.alphas_cumprod_prev
        g64 = S.gaussian_gain(ab, S2)
        tape = analytic_tape(len(ab))
        full = torch.cat([x_T[None], tape]).float().to(d)
        for order in (1, 2):
            got = df.dpm_solver_sde_sample_loop(model, tuple(x_T.shape), clip_denoised=False, model_kwargs={"y": {}}, device=d,
                                                order=order, eta=1.0, noise_tape=full).double().cpu().numpy()
            want = S.sde_loop(ab, abp, x_T.numpy(), lambda x, i: g64[i] * x, order, 1.0, tape.numpy())
            rel = float(np.abs(got - want).max() / np.abs(want).max())
            print(f"{sp} order {order}: rel err vs the fp64 restatement {rel:.3e} (tolerance {FP32_LOOP_TOL:.3e})")
            assert rel <= FP32_LOOP_TOL, (sp, order, rel)


def test_analytic_gaussian_case_has_the_predicted_variance():
    """The same denoiser under in-kernel Philox noise, linear schedule, logsnr20, eta = 1, N = 8 * 16 * 256 = 32 768 elements, x_T
    = Philox draw 0 scaled to the exact marginal: the sample variance over the covariance recursion's prediction, minus 1, lies
    within 5*sqrt(2/N) = 3.9 % for order 2 and for order 1, each against its own prediction.  The two predictions are 44 points
    of the data's variance apart (+7.0 % and -37.2 %), so a missing or mis-scaled noise term cannot pass; with STAT_SEED the CPU
    restatement driven by oracle/philox.py measured +0.7 % for both orders (test_dpm_sde_host.py)."""
    from gesturediffusion_amd import engine as E
    d = dev()
    df = diffusion("linear", "logsnr20")
    ab = df.alphas_cumprod
    model = _exact_denoiser(d)
    x_T = E.randn(STAT_SHAPE, d, STAT_SEED, 0, 0) * float(np.sqrt(ab[-1] * S2 + 1.0 - ab[-1]))
    for order in (2, 1):
        got = df.dpm_solver_sde_sample_loop(model, STAT_SHAPE, noise=x_T, clip_denoised=False, model_kwargs={"y": {}}, device=d,
                                            order=order, eta=1.0, rng="philox", philox_seed=STAT_SEED).double()
        rel = float((got * got).mean()) / stat_prediction(order) - 1.0
        print(f"order {order}: sample variance / prediction - 1 = {rel:+.3%} (bound {STAT_BOUND:.3%})")
        assert abs(rel) <= STAT_BOUND, (order, rel)


# --------------------------------------------------------------------------------------------------------------------- CLI
def test_generate_cli_dpmpp_sde_equals_a_direct_call(tmp_path):
    """`sample.generate --synthetic --sampler dpmpp_sde --dpm_order 2 --timestep_respacing logsnr20 --rng philox` at a small
    width: results.npy holds the samples a direct sample_chunks call produces on the inputs the CLI builds from its seed."""
    from gesturediffusion_amd.model.cfg_sampler import ClassifierFreeSampleModel
    from gesturediffusion_amd.sample import generate
    from gesturediffusion_amd.utils.init import MFCC_DIM, init_state_dict
    from gesturediffusion_amd.utils.model_util import create_model_and_diffusion
    from gesturediffusion_amd.utils.parser_util import generate_args
    out = tmp_path / "out"
    argv = ["--synthetic", "--latent_dim", "128", "--layers", "2", "--num_samples", "3", "--chunks", "2", "--synthetic_njoints", "37",
            "--output_dir", str(out), "--seed", "7", "--arch_version", "mdm", "--num_frames", "20", "--sampler", "dpmpp_sde",
            "--dpm_order", "2", "--timestep_respacing", "logsnr20", "--rng", "philox"]
    assert generate.main(argv) == 0
    res = np.load(out / "results.npy", allow_pickle=True).item()      # written by this test a moment ago
    assert res["motion"].shape == (3, 37, 1, 40) and np.isfinite(res["motion"]).all()
    d = dev()
    args = generate_args(argv)
    args.mfcc_input = True
    model, df = create_model_and_diffusion(args, None)
    assert 10 <= df.num_timesteps <= 20 and args.dpm_eta == 1.0
    cfg = dict(arch="mdm", njoints=37, nfeats=1, latent_dim=128, ff_size=1024, num_layers=2, num_heads=4, seed_poses=args.seed_poses)
    model.load_state_dict(init_state_dict(cfg, seed=7), strict=False)
    if args.guidance_param != 1:
        model = ClassifierFreeSampleModel(model)
    model = model.to(d).eval()
    gen = torch.Generator().manual_seed(7)
    seedp = torch.randn(3, 37, 1, args.seed_poses, generator=gen).to(d)
    mfcc_of_chunk = lambda chunk: torch.randn(3, MFCC_DIM, 1, 20, generator=gen).to(d)   # noqa: E731  (called once per chunk, in order)
    outs = generate.sample_chunks(model, df, seedp, mfcc_of_chunk, 2, 20, args.seed_poses, guidance_param=args.guidance_param,
                                  sampler="dpmpp_sde", eta=args.dpm_eta, rng="philox", philox_seed=7, sample_offset=0, dpm_order=2)
    want = torch.cat(outs, dim=3).cpu().numpy()
    assert np.array_equal(res["motion"], want)
