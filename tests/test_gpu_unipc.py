"""UniPC sampling on the GPU (gdx_unipc_step, gdx_unipc_loop, unipc_sample{,_loop}; include/gdx.h): the fused step against its op
order in torch fp32, the in-library loop against the step-wise protocol and the block-wise issue bit for bit, the predictor alone
against DPM-Solver++, the analytic Gaussian case against the fp64 restatement (unipc_restatement.py), the guidance plan,
workspace guards and the CLI.  Tiny models and variants: test_gpu_dpm.py."""
import itertools

import numpy as np
import pytest
import torch

import dpm_restatement as R
import unipc_restatement as U
from misaligned import shifted as _shifted
from test_dpm_host import S2, analytic_x_T, diffusion
from test_gpu_dpm import ARCHS, B, VARIANTS, _tiny, _variant, _x_T
from test_gpu_parity import dev
from test_unipc_host import UNIPC_FP32_LOOP_TOL, assert_gain

pytestmark = pytest.mark.gpu
PAIRS = [(0, 1), (1, 1), (1, 2), (2, 2), (3, 2), (2, 3), (3, 3)]          # (corr_order, pred_order) the order rule reaches


# ---------------------------------------------------------------------------------------------------------------- kernel
def _torch_step(corr, pred, rows, rows_up, rows_c, x, oc, ou, scale, mask, motion, clip, hist):
    """The kernel's op order in torch fp32 on the device, one torch op per rounding -> (out, xc, m0).  rows = coef[idx],
    rows_up = coef[idx + 1], rows_c = coef_c[idx + 1], each [B, ...]."""
    m0 = oc
    if ou is not None:
        m0 = ou + scale.view(-1, 1, 1, 1) * (oc - ou)
    if mask is not None:
        m0 = torch.where(mask, motion, m0)
    if clip:
        m0 = m0.clamp(-1, 1)
    xc = x
    if corr:
        c = lambda j: rows_c[:, 4 * (corr - 1) + j].view(-1, 1, 1, 1)   # noqa: E731
        acc = c(0) * m0
        for j in range(corr):
            acc = acc + c(1 + j) * hist[j]
        xc = rows_up[:, 0].view(-1, 1, 1, 1) * x + acc
    col = 1 + (pred - 1) * pred // 2
    w = lambda j: rows[:, col + j].view(-1, 1, 1, 1)   # noqa: E731
    acc = w(0) * m0
    for j in range(pred - 1):
        acc = acc + w(j + 1) * hist[j]
    return rows[:, 0].view(-1, 1, 1, 1) * xc + acc, xc, m0


@pytest.mark.parametrize("J,T,shift", [(3, 4, False), (3, 5, False), (13, 80, False), (3, 4, True)])
@pytest.mark.parametrize("corr,pred", PAIRS)
def test_unipc_step_bit_exact(corr, pred, J, T, shift):
    """gdx_unipc_step == its op order in torch by torch.equal on out, base_out and pred_out.  J*T = 12 takes the 128-bit path, 15
    the scalar path with a 3-element tail group, 1040 = 260 groups a second block in x, and 12 with x one float off alignment the
    scalar path again.  Per-sample t (two different rows) and step_index; plain, CFG with two scales, CFG + inpainting + clamp;
    base_out aliasing x, and out aliasing x.  History slots the pair does not read hold NaN; at corr_order 0 base_out has x's
    bits."""
    from gesturediffusion_amd import engine as E
    d = dev()
    coef, coef_c = diffusion("linear", "logsnr20").unipc_coef_tables(d)
    assert coef.shape[0] >= 10 and bool((coef[[3, 5, 7]][:, :7] != 0).all())
    assert bool((coef_c[[4, 6, 8]][:, [0, 1, 4, 5, 6, 8, 9, 10, 11]] != 0).all())
    g = torch.Generator().manual_seed(1000 * corr + 100 * pred + J * T)
    shape = (B, J, 1, T)
    rnd = lambda s=1.0: (torch.randn(shape, generator=g) * s).to(d)   # noqa: E731
    x, oc, ou, motion = rnd(), rnd(1.5), rnd(1.5), rnd(0.5)
    hist = [rnd(1.5) for _ in range(3)]
    mask = (torch.rand(shape, generator=g) < 0.3).to(d)
    scale = torch.tensor([2.5, -1.0], device=d)
    nan = torch.full(shape, float("nan"), device=d)
    hist_in = [hist[i] if i < max(corr, pred - 1) else nan for i in range(3)]
    t_rows = torch.tensor([3, 7], device=d)
    ran = 0
    for (cfg, inp, clip), (t_mode, alias) in itertools.product(
            [(False, False, False), (True, False, False), (True, True, True)],
            [("t", None), ("t", "base"), (5, None), (5, "out")]):
        kw_t = dict(t=t_rows) if t_mode == "t" else dict(step_index=t_mode)
        idx = t_rows if t_mode == "t" else torch.tensor([t_mode, t_mode], device=d)
        ops = dict(ou=ou if cfg else None, scale=scale if cfg else None, mask=mask if inp else None, motion=motion if inp else None)
        want_out, want_base, want_pred = _torch_step(corr, pred, coef[idx], coef[idx + 1], coef_c[idx + 1], x, oc, ops["ou"],
                                                     ops["scale"], ops["mask"], ops["motion"], clip, hist)
        xin = _shifted(x.clone()) if shift else x.clone()
        out = xin if alias == "out" else torch.empty_like(x)
        base = xin if alias == "base" else torch.empty_like(x)
        p_out = torch.empty_like(x)
        E.unipc_step(corr, pred, coef, coef_c, xin, oc, out, base, hist=hist_in, x0_uncond=ops["ou"], scale=ops["scale"],
                     inpaint_mask=ops["mask"], inpaint_motion=ops["motion"], clip_denoised=clip, pred_out=p_out, **kw_t)
        tag = (corr, pred, J, T, shift, cfg, inp, clip, t_mode, alias)
        for name, got, ref in (("out", out, want_out), ("base", base, want_base), ("pred", p_out, want_pred)):
            assert torch.isfinite(got).all(), (name, tag)
            assert torch.equal(got, ref), (name, tag)
        if corr == 0:
            assert torch.equal(base.view(torch.int32), x.view(torch.int32)), tag
        ran += 1
    assert ran == 12


def test_unipc_step_row_zero_returns_the_prediction():
    """Row 0 is (0, 1, 0, ...): the step to sigma = 0 returns the (clamped) prediction itself, whatever x holds -- without a
    corrector (the loop's rule at index 0) and with one, whose corrected state is then finite but unused."""
    from gesturediffusion_amd import engine as E
    d = dev()
    coef, coef_c = diffusion("cosine", "ddim10").unipc_coef_tables(d)
    g = torch.Generator().manual_seed(3)
    x, oc, h0 = ((torch.randn(2, 16, 1, 20, generator=g) * 2).to(d) for _ in range(3))
    for corr in (0, 1):
        out, base, pred = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
        E.unipc_step(corr, 1, coef, coef_c, x, oc, out, base, hist=[h0], step_index=0, clip_denoised=True, pred_out=pred)
        assert torch.equal(pred, oc.clamp(-1, 1)) and torch.equal(out, pred)
        assert torch.equal(base, x) if corr == 0 else torch.isfinite(base).all()


# ------------------------------------------------------------------------------------------------------------------ loop
def _hand_loop(df, model, x_T, y, order, clip_denoised=False, skip_timesteps=0, init_image=None):
    """The loop written out over unipc_sample, as a caller of the step-wise protocol would."""
    idx = list(range(df.num_timesteps - skip_timesteps))[::-1]
    img = x_T
    if init_image is not None:
        img = df.q_sample(init_image, torch.full((x_T.shape[0],), idx[0], device=x_T.device, dtype=torch.long), x_T)
    old = None
    for i in idx:
        t = torch.full((x_T.shape[0],), i, device=x_T.device, dtype=torch.long)
        old = df.unipc_sample(model, img, t, clip_denoised=clip_denoised, model_kwargs={"y": y}, order=order, old_out=old)
        assert len(old["old_pred"]) <= order and set(old) == {"sample", "pred_xstart", "old_pred", "base"}
        img = old["sample"]
    return img


def _count_calls(monkeypatch):
    from gesturediffusion_amd.engine import Engine
    calls = {"unipc_loop": 0, "forward": 0}
    for name in calls:
        orig = getattr(Engine, name)

        def counted(self, *a, _orig=orig, _name=name, **k):
            calls[_name] += 1
            return _orig(self, *a, **k)
        monkeypatch.setattr(Engine, name, counted)
    return calls


@pytest.mark.parametrize("arch", ARCHS)
@pytest.mark.parametrize("resp", ["ddim10", "logsnr20"])
@pytest.mark.parametrize("order", [1, 2, 3])
def test_fused_loop_equals_stepwise_and_blockwise_bit_for_bit(arch, resp, order, monkeypatch):
    """unipc_sample_loop(fused=True) == fused=False == a hand loop over unipc_sample == the loop issued in blocks of 1 and 3 steps
    (run_steps / k_base: the ring and the corrected state live in the caller's buffers), on the tiny V1 / V2: conditional, CFG,
    inpainting, clip_denoised, init_image + skip_timesteps=3 and the single-step loop; the fused route is one gdx_unipc_loop call
    and no step-wise forward."""
    from gesturediffusion_amd.diffusion import gaussian_diffusion as gd
    g, m = _tiny(arch)
    df = diffusion("cosine", resp)
    n = df.num_timesteps
    x_T = _x_T(g)
    calls = _count_calls(monkeypatch)
    for name in VARIANTS:
        model, y, kw = _variant(name, g, m, n)
        kw = dict(kw, noise=x_T.clone(), model_kwargs={"y": y}, order=order)
        steps = n - kw.get("skip_timesteps", 0)
        calls.update(unipc_loop=0, forward=0)
        fused = df.unipc_sample_loop(model, tuple(x_T.shape), **kw)
        assert calls == {"unipc_loop": 1, "forward": 0}, (name, calls)
        step = df.unipc_sample_loop(model, tuple(x_T.shape), fused=False, **kw)
        assert calls == {"unipc_loop": 1, "forward": steps}, (name, calls)
        hand = _hand_loop(df, model, x_T, y, order, kw["clip_denoised"], kw.get("skip_timesteps", 0), kw.get("init_image"))
        assert torch.isfinite(fused).all() and torch.equal(fused, step) and torch.equal(fused, hand), name
        for run_steps in (1, 3):
            calls.update(unipc_loop=0)
            with monkeypatch.context() as mp:
                mp.setattr(gd, "NOISE_BLOCK", run_steps)
                blocks = df.unipc_sample_loop(model, tuple(x_T.shape), progress=True, **kw)
            assert calls["unipc_loop"] == -(-steps // run_steps), (name, run_steps)
            assert torch.equal(fused, blocks), (name, run_steps)
        assert torch.equal(x_T, _x_T(g))                                  # the caller's x_T is not written


def test_the_corrector_acts():
    """Not a tautology: at every order the UniPC sample differs from the DPM-Solver++ sample of that order on the same inputs."""
    g, m = _tiny("mdm")
    df = diffusion("cosine", "logsnr20")
    x_T = _x_T(g)
    model, y, kw = _variant("cond", g, m, df.num_timesteps)
    for order in (1, 2, 3):
        kw_o = dict(kw, noise=x_T.clone(), model_kwargs={"y": y}, order=order)
        assert not torch.equal(df.unipc_sample_loop(model, tuple(x_T.shape), **kw_o),
                               df.dpm_solver_sample_loop(model, tuple(x_T.shape), **kw_o)), order


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_fused_equals_stepwise_in_the_16_bit_modes(dtype):
    """Both routes use the same forward, so the bits stay equal under compute_dtype fp16 / bf16."""
    g, m = _tiny("mdm", dtype)
    df = diffusion("cosine", "logsnr20")
    x_T = _x_T(g)
    model, y, kw = _variant("cfg", g, m, df.num_timesteps)
    kw = dict(kw, noise=x_T.clone(), model_kwargs={"y": y}, order=3)
    fused = df.unipc_sample_loop(model, tuple(x_T.shape), **kw)
    step = df.unipc_sample_loop(model, tuple(x_T.shape), fused=False, **kw)
    assert torch.isfinite(fused).all() and torch.equal(fused, step)


@pytest.mark.parametrize("arch", ARCHS)
def test_order_one_without_the_corrector_is_dpm_solver_order_one(arch):
    """The (0, 1) pair at every step -- the predictor alone -- runs dpm_solver_sample_loop(order=1)'s arithmetic: equal bits."""
    from gesturediffusion_amd import engine as E
    g, m = _tiny(arch)
    df = diffusion("cosine", "logsnr20")
    x_T = _x_T(g)
    model, y, kw = _variant("cfg", g, m, df.num_timesteps)
    want = df.dpm_solver_sample_loop(model, tuple(x_T.shape), noise=x_T.clone(), model_kwargs={"y": y}, order=1, **kw)
    coef, coef_c = df.unipc_coef_tables(x_T.device)
    x = x_T.clone()
    for i in range(df.num_timesteps - 1, -1, -1):
        t = torch.full((B,), i, device=x.device, dtype=torch.long)
        pred = df._pred_xstart(model, x, t, kw["clip_denoised"], None, {"y": y})
        x = E.unipc_step(0, 1, coef, coef_c, x, pred, torch.empty_like(x), torch.empty_like(x), step_index=i)
    assert torch.equal(x, want)


def test_fused_loop_leaves_the_workspace_guards_intact():
    g, m = _tiny("mdm")
    d = dev()
    df = diffusion("cosine", "logsnr20")
    x_T = _x_T(g)
    eng = m._get_engine(d)
    eng.set_guards(True)
    try:
        model, y, kw = _variant("cfg", g, m, df.num_timesteps)
        r = df.unipc_sample_loop(model, tuple(x_T.shape), noise=x_T.clone(), model_kwargs={"y": y}, order=3, **kw)
        bad, zone = eng.check_guards(d)
        assert bad == 0, f"{bad} canary bytes overwritten, first in workspace allocation #{zone}"
        assert torch.isfinite(r).all()
    finally:
        eng.set_guards(False)


def test_refusals_come_before_the_library_is_called(monkeypatch):
    g, m = _tiny("mdm")
    df = diffusion("cosine", "ddim10")
    model, y, kw = _variant("cond", g, m, 10)
    x_T = _x_T(g)
    calls = _count_calls(monkeypatch)
    for order in (0, 4):
        with pytest.raises(ValueError, match="order is invalid"):
            df.unipc_sample_loop(model, tuple(x_T.shape), noise=x_T.clone(), model_kwargs={"y": y}, order=order, **kw)
    t = torch.tensor([3, 4], device=dev())
    with pytest.raises(ValueError, match="same for the whole batch"):
        df.unipc_sample(model, x_T, t, model_kwargs={"y": y})
    df.rescale_timesteps = True
    with pytest.raises(NotImplementedError, match="rescale_timesteps"):
        df.unipc_sample_loop(model, tuple(x_T.shape), noise=x_T.clone(), model_kwargs={"y": y}, **kw)
    assert calls == {"unipc_loop": 0, "forward": 0}


# ------------------------------------------------------------------------------------------------------ analytic Gaussian case
def test_analytic_gaussian_case_matches_the_fp64_restatement():
    """Data N(0, 0.25 I) with its exact linear denoiser as a Python callable on the ORIGINAL timestep, through the step-wise route:
    linear schedule, logsnr20 / logsnr40, orders 1..3.  The result agrees with the fp64 restatement run on the same x_T within
    UNIPC_FP32_LOOP_TOL = 1.83e-6 (4x the worst error of the restatement's own recurrence in torch fp32 on the CPU, 4.574e-7:
    test_unipc_host.py), and the GPU results show the issue's three inequalities against DPM-Solver++ in fp64."""
    from gesturediffusion_amd.diffusion import gaussian_diffusion as gd
    d = dev()
    x_T = analytic_x_T()
    abar_orig, _ = R.schedule(gd.get_named_beta_schedule("linear", 1000))
    gain = torch.from_numpy(R.gaussian_gain(abar_orig, S2)).float().to(d)
    model = lambda x, t, y: gain[t].view(-1, 1, 1, 1) * x   # noqa: E731
    err = {}
    for sp in ("logsnr20", "logsnr40"):
        df = diffusion("linear", sp)
        ab, abp = df.alphas_cumprod, df.alphas_cumprod_prev
        g64 = R.gaussian_gain(ab, S2)
        den = lambda x, i: g64[i] * x   # noqa: E731
        for order in (1, 2, 3):
            got = df.unipc_sample_loop(model, tuple(x_T.shape), noise=x_T.float().to(d), clip_denoised=False,
                                       model_kwargs={"y": {}}, device=d, order=order).double().cpu().numpy()
            want = U.unipc_loop(ab, abp, x_T.numpy(), den, order)
            rel = float(np.abs(got - want).max() / np.abs(want).max())
            print(f"{sp} order {order}: rel err vs the fp64 restatement {rel:.3e} (tolerance {UNIPC_FP32_LOOP_TOL:.3e})")
            assert rel <= UNIPC_FP32_LOOP_TOL, (sp, order, rel)
            err["unipc", sp, order] = R.gaussian_error(got, x_T.numpy(), ab[-1], S2)
            err["dpm", sp, order] = R.gaussian_error(R.dpm_loop(ab, abp, x_T.numpy(), den, order), x_T.numpy(), ab[-1], S2)
    assert_gain(err)


# --------------------------------------------------------------------------------------------------------------- guidance plan
@pytest.mark.parametrize("arch,T", [("mdm", 20), ("mdm_old", 12)])
def test_interval_rescale_and_refresh_together_equal_a_hand_loop(arch, T):
    """One combined case: guidance interval (300, 700) + guidance_rescale 0.7 + guidance_refresh 2 on the ten steps of logsnr10,
    order 2.  The fused loop == a hand loop over unipc_sample whose model is built from the step-wise pieces (the conditional
    forward, the unconditional one on a refresh, torch.sub for the difference, gdx_cfg_rescale for the blend), torch.equal; and it
    pushes as many samples through the denoiser as dpm_solver_sample_loop does under the same keys: one call per step."""
    from test_gpu_guidance_interval import MID, _cfg, _inputs, _model, _ys
    from test_gpu_guidance_refresh import PHI, _HandModel, _plan
    m = _model(arch, "fp32")
    df = diffusion("linear", "logsnr10")
    plan = _plan(df, 2, "dpmpp", MID)
    assert plan == df.guidance_plan(MID, 2) and {"off", "refresh", "reuse"} <= set(plan) and len(plan) == df.num_timesteps
    y = dict(_ys(T, "plain", MID)[0], guidance_refresh=2, guidance_rescale=PHI)
    tape = _inputs(T)[1]["tape"]
    shape = tuple(tape.shape[1:])
    eng = m._get_engine(dev())
    kw = dict(noise=tape[0].clone(), clip_denoised=False, model_kwargs={"y": y}, order=2)
    before = eng.forward_samples()
    fused = df.unipc_sample_loop(_cfg(m), shape, **kw)
    ran = eng.forward_samples() - before
    before = eng.forward_samples()
    df.dpm_solver_sample_loop(_cfg(m), shape, **kw)
    assert ran == eng.forward_samples() - before == sum(2 * B if what == "refresh" else B for what in plan)
    hand_model = _HandModel(m, plan, PHI)
    x, old = tape[0], None
    for i in range(df.num_timesteps - 1, -1, -1):
        t = torch.full((B,), i, device=x.device, dtype=torch.long)
        old = df.unipc_sample(hand_model, x, t, clip_denoised=False, model_kwargs={"y": _ys(T)[0]}, order=2, old_out=old)
        x = old["sample"]
    assert hand_model.seen == list(plan)
    assert torch.isfinite(fused).all() and torch.equal(fused, x)
    with pytest.raises(ValueError, match="guidance_refresh"):                 # the step-wise route cannot carry the difference
        df.unipc_sample_loop(_cfg(m), shape, fused=False, **kw)


# --------------------------------------------------------------------------------------------------------------------- CLI
def test_generate_cli_unipc_equals_a_direct_call(tmp_path):
    """`sample.generate --synthetic --arch_version mdm --num_frames 20 --chunks 2 --sampler unipc --unipc_order 3
    --timestep_respacing logsnr20` at a small width: results.npy holds finite motion of the expected shape, and its first
    chunk is a direct unipc_sample_loop call on the inputs the CLI builds from its seed."""
    from gesturediffusion_amd.model.cfg_sampler import ClassifierFreeSampleModel
    from gesturediffusion_amd.sample import generate
    from gesturediffusion_amd.utils.init import MFCC_DIM, init_state_dict
    from gesturediffusion_amd.utils.model_util import create_model_and_diffusion
    from gesturediffusion_amd.utils.parser_util import generate_args
    out = tmp_path / "out"
    argv = ["--synthetic", "--latent_dim", "128", "--layers", "2", "--num_samples", "3", "--chunks", "2", "--synthetic_njoints", "37",
            "--output_dir", str(out), "--seed", "7", "--arch_version", "mdm", "--num_frames", "20", "--sampler", "unipc",
            "--unipc_order", "3", "--timestep_respacing", "logsnr20", "--rng", "philox"]
    assert generate.main(argv) == 0
    res = np.load(out / "results.npy", allow_pickle=True).item()      # written by this test a moment ago
    assert res["motion"].shape == (3, 37, 1, 40) and np.isfinite(res["motion"]).all()
    d = dev()
    args = generate_args(argv)
    args.mfcc_input = True
    model, df = create_model_and_diffusion(args, None)
    assert 10 <= df.num_timesteps <= 20
    cfg = dict(arch="mdm", njoints=37, nfeats=1, latent_dim=128, ff_size=1024, num_layers=2, num_heads=4, seed_poses=args.seed_poses)
    model.load_state_dict(init_state_dict(cfg, seed=7), strict=False)
    model = ClassifierFreeSampleModel(model).to(d).eval()
    gen = torch.Generator().manual_seed(7)
    seedp = torch.randn(3, 37, 1, args.seed_poses, generator=gen)
    mfcc = torch.randn(3, MFCC_DIM, 1, 20, generator=gen)
    y = {"seed": seedp.to(d), "mfcc": mfcc.to(d), "scale": torch.ones(3, device=d) * args.guidance_param}
    want = df.unipc_sample_loop(model, (3, 37, 1, 20), clip_denoised=False, model_kwargs={"y": y}, order=3, rng="philox",
                                philox_seed=7)
    assert np.array_equal(res["motion"][..., :20], want.cpu().numpy())
    other = df.unipc_sample_loop(model, (3, 37, 1, 20), clip_denoised=False, model_kwargs={"y": y}, order=2, rng="philox",
                                 philox_seed=7)
    assert not np.array_equal(res["motion"][..., :20], other.cpu().numpy())      # --unipc_order reached the sampler
