"""DPM-Solver++ multistep sampling on the GPU (gdx_dpm_step, gdx_dpm_loop, dpm_solver_sample{,_loop}; include/gdx.h): the fused
step against its op order in torch fp32, the in-library loop against the step-wise protocol bit for bit, order 1 against DDIM,
the analytic Gaussian case against the fp64 restatement (dpm_restatement.py), workspace guards and the CLI."""
import itertools

import numpy as np
import pytest
import torch

import dpm_restatement as R
from conftest import load_golden, weights_from
from misaligned import shifted as _shifted
from test_dpm_host import (DDIM_BOUND_ULPS, FP32_LOOP_TOL, S2, analytic_x_T, assert_convergence, ddim_bound_ulps,
                           ddim_bound_unit, diffusion)
from test_gpu_parity import TINY, build_model, dev

pytestmark = pytest.mark.gpu
ARCHS = ["mdm", "mdm_old"]
B = 2


# ---------------------------------------------------------------------------------------------------------------- kernel
def _torch_step(order, rows, x, oc, ou, scale, mask, motion, clip, hist):
    """The kernel's op order in torch fp32 on the device, one torch op per rounding -> (out, m0)."""
    m0 = oc
    if ou is not None:
        m0 = ou + scale.view(-1, 1, 1, 1) * (oc - ou)
    if mask is not None:
        m0 = torch.where(mask, motion, m0)
    if clip:
        m0 = m0.clamp(-1, 1)
    col = 1 + (order - 1) * order // 2
    w = lambda j: rows[:, col + j].view(-1, 1, 1, 1)   # noqa: E731
    acc = w(0) * m0
    for j in range(order - 1):
        acc = acc + w(j + 1) * hist[j]
    return rows[:, 0].view(-1, 1, 1, 1) * x + acc, m0


@pytest.mark.parametrize("J,T,shift", [(3, 4, False), (3, 5, False), (13, 80, False), (3, 4, True)])
@pytest.mark.parametrize("order", [1, 2, 3])
def test_dpm_step_bit_exact(order, J, T, shift):
    """gdx_dpm_step == its op order in torch by torch.equal on out and pred_out.  J*T = 12 takes the 128-bit path, 15 the scalar
    path with a 3-element tail group, 1040 = 260 groups a second block in x, and 12 with x one float off alignment the scalar
    path again.  Per-sample t (two different rows) and step_index; plain, CFG with two scales, CFG + inpainting + clamp; out
    aliasing x.  History slots the order does not read hold NaN."""
    from gesturediffusion_amd import engine as E
    d = dev()
    coef = diffusion("linear", "logsnr20").dpm_coef_table(d)
    assert coef.shape[0] >= 10 and bool((coef[[3, 5, 7]][:, :7] != 0).all())
    g = torch.Generator().manual_seed(100 * order + J * T)
    shape = (B, J, 1, T)
    rnd = lambda s=1.0: (torch.randn(shape, generator=g) * s).to(d)   # noqa: E731
    x, oc, ou, motion = rnd(), rnd(1.5), rnd(1.5), rnd(0.5)
    hist = [rnd(1.5) for _ in range(2)]
    mask = (torch.rand(shape, generator=g) < 0.3).to(d)
    scale = torch.tensor([2.5, -1.0], device=d)
    nan = torch.full(shape, float("nan"), device=d)
    hist_in = [hist[i] if i < order - 1 else nan for i in range(2)]
    t_rows = torch.tensor([3, 7], device=d)
    ran = 0
    for (cfg, inp, clip), (t_mode, alias) in itertools.product([(False, False, False), (True, False, False), (True, True, True)],
                                                                [("t", False), ("t", True), (5, False), (5, True)]):
        kw_t = dict(t=t_rows) if t_mode == "t" else dict(step_index=t_mode)
        rows = coef[t_rows] if t_mode == "t" else coef[[t_mode, t_mode]]
        ops = dict(ou=ou if cfg else None, scale=scale if cfg else None, mask=mask if inp else None, motion=motion if inp else None)
        want_out, want_pred = _torch_step(order, rows, x, oc, ops["ou"], ops["scale"], ops["mask"], ops["motion"], clip, hist)
        xin = _shifted(x.clone()) if shift else x.clone()
        out = xin if alias else torch.empty_like(x)
        pred = torch.empty_like(x)
        E.dpm_step(order, coef, xin, oc, out, hist=hist_in, x0_uncond=ops["ou"], scale=ops["scale"], inpaint_mask=ops["mask"],
                   inpaint_motion=ops["motion"], clip_denoised=clip, pred_out=pred, **kw_t)
        tag = (order, J, T, shift, cfg, inp, clip, t_mode, alias)
        for name, got, ref in (("out", out, want_out), ("pred", pred, want_pred)):
            assert torch.isfinite(got).all(), (name, tag)
            assert torch.equal(got, ref), (name, tag)
        ran += 1
    assert ran == 12


def test_dpm_step_row_zero_returns_the_prediction():
    """Row 0 is (0, 1, 0, ...): the step to sigma = 0 returns the (clamped) prediction itself, whatever x holds."""
    from gesturediffusion_amd import engine as E
    d = dev()
    coef = diffusion("cosine", "ddim10").dpm_coef_table(d)
    g = torch.Generator().manual_seed(3)
    x, oc = ((torch.randn(2, 16, 1, 20, generator=g) * 2).to(d) for _ in range(2))
    out, pred = torch.empty_like(x), torch.empty_like(x)
    E.dpm_step(1, coef, x, oc, out, step_index=0, clip_denoised=True, pred_out=pred)
    assert torch.equal(pred, oc.clamp(-1, 1)) and torch.equal(out, pred)


# ------------------------------------------------------------------------------------------------------------------ loop
def _tiny(arch, dtype="fp32"):
    g = load_golden(f"loops_{arch}_tiny.npz")
    m = build_model(arch, TINY, weights_from(g))
    m.compute_dtype = dtype
    return g, m


VARIANTS = ["cond", "cfg", "inpaint", "clip", "init_skip3", "single_step"]


def _variant(name, g, m, n):
    """(model, y, keywords of dpm_solver_sample_loop) of a variant on the first B samples of the tiny fixtures' inputs; n = the
    diffusion's step count."""
    from gesturediffusion_amd.model.cfg_sampler import ClassifierFreeSampleModel
    d = dev()
    Tn = lambda k: torch.from_numpy(g[k])[:B].contiguous().to(d)   # noqa: E731
    y, kw, model = {"seed": Tn("seed"), "mfcc": Tn("mfcc")}, dict(clip_denoised=False), m
    if name == "cfg":
        y["scale"] = Tn("scale")
        model = ClassifierFreeSampleModel(m)
    if name == "inpaint":
        y["inpainting_mask"], y["inpainted_motion"] = Tn("inpainting_mask"), Tn("inpainted_motion")
    if name == "clip":
        kw["clip_denoised"] = True
    if name == "init_skip3":
        kw.update(init_image=Tn("init_image"), skip_timesteps=3)
    if name == "single_step":                       # one step at index 0: first order, x' = the prediction
        kw.update(init_image=Tn("init_image"), skip_timesteps=n - 1)
    return model, y, kw


def _x_T(g):
    return torch.from_numpy(g["tape"])[0, :B].contiguous().to(dev())


def _hand_loop(df, model, x_T, y, order, clip_denoised=False, skip_timesteps=0, init_image=None):
    """The loop written out over dpm_solver_sample, as a caller of the step-wise protocol would."""
    idx = list(range(df.num_timesteps - skip_timesteps))[::-1]
    img = x_T
    if init_image is not None:
        img = df.q_sample(init_image, torch.full((x_T.shape[0],), idx[0], device=x_T.device, dtype=torch.long), x_T)
    old = None
    for i in idx:
        t = torch.full((x_T.shape[0],), i, device=x_T.device, dtype=torch.long)
        old = df.dpm_solver_sample(model, img, t, clip_denoised=clip_denoised, model_kwargs={"y": y}, order=order, old_out=old)
        assert len(old["old_pred"]) <= order - 1
        img = old["sample"]
    return img


def _count_calls(monkeypatch):
    from gesturediffusion_amd.engine import Engine
    calls = {"dpm_loop": 0, "forward": 0}
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
def test_fused_loop_equals_stepwise_bit_for_bit(arch, resp, order, monkeypatch):
    """dpm_solver_sample_loop(fused=True) == fused=False == a hand loop over dpm_solver_sample on the tiny V1 / V2: conditional,
    CFG, inpainting, clip_denoised, init_image + skip_timesteps=3 and the single-step loop; the fused route is one gdx_dpm_loop
    call and no step-wise forward."""
    g, m = _tiny(arch)
    df = diffusion("cosine", resp)
    n = df.num_timesteps
    x_T = _x_T(g)
    calls = _count_calls(monkeypatch)
    for name in VARIANTS:
        model, y, kw = _variant(name, g, m, n)
        kw = dict(kw, noise=x_T.clone(), model_kwargs={"y": y}, order=order)
        calls.update(dpm_loop=0, forward=0)
        fused = df.dpm_solver_sample_loop(model, tuple(x_T.shape), **kw)
        assert calls == {"dpm_loop": 1, "forward": 0}, (name, calls)
        step = df.dpm_solver_sample_loop(model, tuple(x_T.shape), fused=False, **kw)
        assert calls == {"dpm_loop": 1, "forward": n - kw.get("skip_timesteps", 0)}, (name, calls)
        hand = _hand_loop(df, model, x_T, y, order, kw["clip_denoised"], kw.get("skip_timesteps", 0), kw.get("init_image"))
        assert torch.isfinite(fused).all() and torch.equal(fused, step) and torch.equal(fused, hand), name
        assert torch.equal(x_T, _x_T(g))                                  # the caller's x_T is not written


@pytest.mark.parametrize("arch", ARCHS)
@pytest.mark.parametrize("run_steps", [1, 3])
def test_one_call_equals_blockwise_issue(arch, run_steps, monkeypatch):
    """run_steps / k_base: the loop issued in blocks of 1 or 3 steps (progress=True) carries its history in the caller's buffer
    and gives the bits of one call."""
    from gesturediffusion_amd.diffusion import gaussian_diffusion as gd
    g, m = _tiny(arch)
    x_T = _x_T(g)
    for resp, name, order in [("logsnr20", "cfg", 3), ("ddim10", "cond", 2), ("ddim10", "inpaint", 3), ("logsnr20", "init_skip3", 2),
                              ("ddim10", "cond", 1)]:
        df = diffusion("cosine", resp)
        model, y, kw = _variant(name, g, m, df.num_timesteps)
        kw = dict(kw, noise=x_T.clone(), model_kwargs={"y": y}, order=order)
        one = df.dpm_solver_sample_loop(model, tuple(x_T.shape), **kw)
        calls = _count_calls(monkeypatch)
        monkeypatch.setattr(gd, "NOISE_BLOCK", run_steps)
        blocks = df.dpm_solver_sample_loop(model, tuple(x_T.shape), progress=True, **kw)
        monkeypatch.undo()
        assert calls["dpm_loop"] == -(-(df.num_timesteps - kw.get("skip_timesteps", 0)) // run_steps)
        assert torch.equal(one, blocks), (resp, name, order)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_fused_equals_stepwise_in_the_16_bit_modes(dtype):
    """Both routes use the same forward, so the bits stay equal under compute_dtype fp16 / bf16."""
    g, m = _tiny("mdm", dtype)
    df = diffusion("cosine", "logsnr20")
    x_T = _x_T(g)
    model, y, kw = _variant("cfg", g, m, df.num_timesteps)
    kw = dict(kw, noise=x_T.clone(), model_kwargs={"y": y}, order=3)
    fused = df.dpm_solver_sample_loop(model, tuple(x_T.shape), **kw)
    step = df.dpm_solver_sample_loop(model, tuple(x_T.shape), fused=False, **kw)
    assert torch.isfinite(fused).all() and torch.equal(fused, step)


def test_fused_loop_leaves_the_workspace_guards_intact():
    g, m = _tiny("mdm")
    d = dev()
    df = diffusion("cosine", "logsnr20")
    x_T = _x_T(g)
    eng = m._get_engine(d)
    eng.set_guards(True)
    try:
        model, y, kw = _variant("cfg", g, m, df.num_timesteps)
        r = df.dpm_solver_sample_loop(model, tuple(x_T.shape), noise=x_T.clone(), model_kwargs={"y": y}, order=3, **kw)
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
            df.dpm_solver_sample_loop(model, tuple(x_T.shape), noise=x_T.clone(), model_kwargs={"y": y}, order=order, **kw)
    t = torch.tensor([3, 4], device=dev())
    with pytest.raises(ValueError, match="same for the whole batch"):
        df.dpm_solver_sample(model, x_T, t, model_kwargs={"y": y})
    df.rescale_timesteps = True
    with pytest.raises(NotImplementedError, match="rescale_timesteps"):
        df.dpm_solver_sample_loop(model, tuple(x_T.shape), noise=x_T.clone(), model_kwargs={"y": y}, **kw)
    assert calls == {"dpm_loop": 0, "forward": 0}


# ----------------------------------------------------------------------------------------------------- order 1 against DDIM
def test_order_one_is_ddim_at_eta_zero():
    """One step on the same x and the same model output at t in {0, 1, 5, 9} of ddim10: dpm_solver_sample(order=1) and
    ddim_sample(eta=0) are two fp32 evaluations of one real number, so their samples differ by at most ddim_bound_ulps(t) units
    of ddim_bound_unit (test_dpm_host.py: 8, and the constant widened at t = 1 where the CPU check showed the DDIM table's own
    fp32 coefficient to be off); pred_xstart is bit-equal."""
    d = dev()
    df = diffusion("cosine", "ddim10")
    ddim, dpm = df.coef_table(1, d, 0.0), df.dpm_coef_table(d)
    g = torch.Generator().manual_seed(11)
    for t in (0, 1, 5, 9):
        tt = torch.full((B,), t, device=d, dtype=torch.long)
        x, m0 = torch.randn(B, 16, 1, 20, generator=g).to(d), (torch.randn(B, 16, 1, 20, generator=g) * 1.5).to(d)
        model = lambda xx, ts, y: m0   # noqa: E731
        a = df.dpm_solver_sample(model, x, tt, clip_denoised=False, model_kwargs={"y": {}}, order=1)
        b = df.ddim_sample(model, x, tt, clip_denoised=False, model_kwargs={"y": {}}, eta=0.0)
        assert torch.equal(a["pred_xstart"], b["pred_xstart"]) and torch.equal(a["pred_xstart"], m0)
        unit = ddim_bound_unit(ddim[tt], dpm[tt], x, m0)
        ratio = float(((a["sample"].double() - b["sample"].double()).abs() / unit.clamp_min(1e-300)).max())
        print(f"t={t}: order 1 vs DDIM {ratio:.3f} units (bound {ddim_bound_ulps(t)})")
        assert ratio <= ddim_bound_ulps(t), (t, ratio)
        # against the fp64 value the new step needs no widening anywhere
        rows = torch.from_numpy(df.dpm_coef_rows()).to(d)
        v64 = rows[t, 0] * x.double() + rows[t, 1] * m0.double()
        assert float(((a["sample"].double() - v64).abs() / unit.clamp_min(1e-300)).max()) <= DDIM_BOUND_ULPS, t


# ------------------------------------------------------------------------------------------------------ analytic Gaussian case
def test_analytic_gaussian_case_matches_the_fp64_restatement():
    """Data N(0, 0.25 I) with its exact linear denoiser as a Python callable on the ORIGINAL timestep, through the step-wise route:
    linear schedule, logsnr20 / logsnr40, orders 1..3.  The result agrees with the fp64 restatement run on the same x_T within
    FP32_LOOP_TOL = 1.57e-6 (4x the worst error of the restatement's own recurrence in torch fp32 on the CPU, 3.92e-7:
    test_dpm_host.py), and the GPU results show the three convergence inequalities against the exact end point."""
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
        for order in (1, 2, 3):
            got = df.dpm_solver_sample_loop(model, tuple(x_T.shape), noise=x_T.float().to(d), clip_denoised=False,
                                            model_kwargs={"y": {}}, device=d, order=order).double().cpu().numpy()
            want = R.dpm_loop(ab, abp, x_T.numpy(), lambda x, i: g64[i] * x, order)
            rel = float(np.abs(got - want).max() / np.abs(want).max())
            print(f"{sp} order {order}: rel err vs the fp64 restatement {rel:.3e} (tolerance {FP32_LOOP_TOL:.3e})")
            assert rel <= FP32_LOOP_TOL, (sp, order, rel)
            err[sp, order] = R.gaussian_error(got, x_T.numpy(), ab[-1], S2)
    assert_convergence(err)


# --------------------------------------------------------------------------------------------------------------------- CLI
def test_generate_cli_dpmpp_equals_a_direct_call(tmp_path):
    """`sample.generate --synthetic --arch_version mdm --num_frames 20 --chunks 2 --sampler dpmpp --dpm_order 2
    --timestep_respacing logsnr20` at a small width: results.npy holds finite motion of the expected shape, and its first
    chunk is a direct dpm_solver_sample_loop call on the inputs the CLI builds from its seed."""
    from gesturediffusion_amd.model.cfg_sampler import ClassifierFreeSampleModel
    from gesturediffusion_amd.sample import generate
    from gesturediffusion_amd.utils.init import MFCC_DIM, init_state_dict
    from gesturediffusion_amd.utils.model_util import create_model_and_diffusion
    from gesturediffusion_amd.utils.parser_util import generate_args
    out = tmp_path / "out"
    argv = ["--synthetic", "--latent_dim", "128", "--layers", "2", "--num_samples", "3", "--chunks", "2", "--synthetic_njoints", "37",
            "--output_dir", str(out), "--seed", "7", "--arch_version", "mdm", "--num_frames", "20", "--sampler", "dpmpp",
            "--dpm_order", "2", "--timestep_respacing", "logsnr20", "--rng", "philox"]
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
    want = df.dpm_solver_sample_loop(model, (3, 37, 1, 20), clip_denoised=False, model_kwargs={"y": y}, order=2, rng="philox",
                                     philox_seed=7)
    assert np.array_equal(res["motion"][..., :20], want.cpu().numpy())
