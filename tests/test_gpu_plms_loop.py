"""plms_sample_loop inside libgdx (gdx_plms_step, gdx_plms_loop; include/gdx.h): the fused step against the three launches it
replaces and the in-library loop against the step-wise protocol, both bit for bit; the reference's PLMS fixtures within the
bounds of test_gpu_parity.py::test_plms_loops_vs_reference_golden."""
import itertools

import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err, weights_from
from misaligned import shifted as _shifted
from test_gpu_parity import LOOP_TOL, TINY, _diffusion, build_model, dev

pytestmark = pytest.mark.gpu
ARCHS = ["mdm", "mdm_old"]
DTYPES = ["fp32", "fp16", "bf16"]


# ---------------------------------------------------------------------------------------------------------------- kernel
def _three_launches(kind, coef, x, oc, ou, scale, mask, motion, clip, t, hist, x_eps, t_eps, pred_prev):
    """Today's composition: gdx_sampler_update's pred_xstart (zero noise) -> gdx_plms_update kind 0 -> kind 1..6.
    Returns (out, eps, pred)."""
    from gesturediffusion_amd import engine as E

    def pred_eps(xx, tt):
        pred = torch.empty_like(xx)
        E.sampler_update(0, coef, xx, oc, torch.empty_like(xx), t=tt, x0_uncond=ou, scale=scale, inpaint_mask=mask,
                         inpaint_motion=motion, noise=torch.zeros_like(xx), pred_xstart=pred, clip_denoised=clip)
        return pred, E.plms_update(0, coef, tt, xx, pred)
    if kind == 5:
        pred2, eps2 = pred_eps(x_eps, t_eps)
        return E.plms_update(5, coef, t, x, pred_prev, eps=[hist[0], eps2]), eps2, pred2
    pred, eps = pred_eps(x, t)
    if kind == 6:
        return E.plms_update(6, coef, t, None, pred, eps=[eps]), eps, pred
    return E.plms_update(kind, coef, t, x, pred, eps=[eps] + hist[:kind - 1]), eps, pred


@pytest.mark.parametrize("J,T", [(263, 196), (150, 60), (7, 9)])
@pytest.mark.parametrize("kind", [1, 2, 3, 4, 5, 6])
def test_plms_step_equals_the_three_launches(kind, J, T):
    """gdx_plms_step == sampler_update(pred_xstart) -> plms_update(0) -> plms_update(kind) by torch.equal on out, eps and
    pred: with / without CFG, inpainting and clamping, per-sample t (rows 0, 1, middle, last) and step_index (0 and 5), out
    aliasing x, operands one float off alignment; J*T = 51548 and 9000 are multiples of 4, 63 is not.  History slots (and the
    kind-5 operands) a kind must not read hold NaN."""
    from gesturediffusion_amd import engine as E
    d = dev()
    df = _diffusion([10])
    n = df.num_timesteps
    coef = df.coef_table(1, d, 0.0)
    g = torch.Generator().manual_seed(100 * kind + J)
    B = 5
    shape = (B, J, 1, T)
    rnd = lambda s=1.0: (torch.randn(shape, generator=g) * s).to(d)   # noqa: E731
    x, oc, ou, motion, x_eps, pred_prev = rnd(), rnd(1.5), rnd(1.5), rnd(0.5), rnd(), rnd()
    hist = [rnd() for _ in range(3)]
    mask = (torch.rand(shape, generator=g) < 0.3).to(d)
    scale = torch.tensor([2.5, 1.0, 0.0, -1.0, 3.0], device=d)
    older = kind - 1 if kind <= 4 else (1 if kind == 5 else 0)
    nan = torch.full(shape, float("nan"), device=d)
    hist_in = [hist[i] if i < older else nan for i in range(3)]
    t_rows = torch.tensor([0, 1, n // 2, n - 1, 0], device=d)
    t2_rows = (t_rows - 1) % n
    ran = 0
    for cfg, inp, clip in itertools.product([False, True], repeat=3):
        for t_mode, alias, shift in [("t", False, False), (0, False, False), (5, True, False), ("t", True, True)]:
            if t_mode == "t":
                t, t_eps, kw_t = t_rows, t2_rows, dict(t=t_rows, t_eps=t2_rows)
            else:
                t, t_eps = torch.full((B,), t_mode, device=d), torch.full((B,), (t_mode - 1) % n, device=d)
                kw_t = dict(step_index=t_mode, step_index_eps=(t_mode - 1) % n)
            f = _shifted if shift else (lambda v: v)
            ops = dict(ou=ou if cfg else None, scale=scale if cfg else None, mask=mask if inp else None,
                       motion=motion if inp else None)
            want = _three_launches(kind, coef, x, oc, ops["ou"], ops["scale"], ops["mask"], ops["motion"], clip, t, hist, x_eps,
                                   t_eps, pred_prev)
            xin = f(x.clone())
            out = xin if alias else f(torch.empty_like(x))
            eps, pred = f(torch.empty_like(x)), f(torch.empty_like(x))
            E.plms_step(kind, coef, xin, f(oc), out, eps_out=eps, eps_hist=[f(h) for h in hist_in],
                        x0_uncond=f(ou) if cfg else None, scale=ops["scale"], inpaint_mask=ops["mask"],
                        inpaint_motion=f(motion) if inp else None, clip_denoised=clip, pred_xstart=pred,
                        x_eps=f(x_eps if kind == 5 else nan), pred_prev=f(pred_prev if kind == 5 else nan), **kw_t)
            tag = (kind, J, T, cfg, inp, clip, t_mode, alias, shift)
            for name, got, ref in zip(("out", "eps", "pred"), (out, eps, pred), want):
                assert torch.isfinite(got).all(), (name, tag)
                assert torch.equal(got, ref), (name, tag)
            ran += 1
    assert ran == 32


def test_plms_step_first_row_returns_pred_where_nz_is_zero():
    """Row 0 has nz = 0: the step returns the (clamped) pred_xstart itself, as the reference's mask does (:1073-1077)."""
    from gesturediffusion_amd import engine as E
    d = dev()
    coef = _diffusion([10]).coef_table(1, d, 0.0)
    g = torch.Generator().manual_seed(3)
    x, oc, e1 = ((torch.randn(2, 16, 1, 20, generator=g) * 2).to(d) for _ in range(3))
    out, eps, pred = (torch.empty_like(x) for _ in range(3))
    E.plms_step(2, coef, x, oc, out, eps_out=eps, eps_hist=[e1], step_index=0, clip_denoised=True, pred_xstart=pred)
    assert torch.equal(pred, oc.clamp(-1, 1)) and torch.equal(out, pred)


# ------------------------------------------------------------------------------------------------------------------ loop
def _tiny(arch, dtype):
    g = load_golden(f"loops_{arch}_tiny.npz")
    m = build_model(arch, TINY, weights_from(g))
    m.compute_dtype = dtype
    return g, m


VARIANTS = ["cond", "uncond", "cfg", "inpaint", "clip", "init_skip3", "single_step"]


def _variant(name, g, m):
    """(model, y, keywords of plms_sample_loop) of a variant on the tiny fixtures' inputs."""
    from gesturediffusion_amd.model.cfg_sampler import ClassifierFreeSampleModel
    d = dev()
    T = lambda k: torch.from_numpy(g[k]).to(d)   # noqa: E731
    y, kw, model = {"seed": T("seed"), "mfcc": T("mfcc")}, dict(clip_denoised=False), m
    if name == "uncond":
        y["uncond"] = True
    if name == "cfg":
        y["scale"] = T("scale")
        model = ClassifierFreeSampleModel(m)
    if name == "inpaint":
        y["inpainting_mask"], y["inpainted_motion"] = T("inpainting_mask"), T("inpainted_motion")
    if name == "clip":
        kw["clip_denoised"] = True
    if name == "init_skip3":
        kw.update(init_image=T("init_image"), skip_timesteps=3)
    if name == "single_step":                       # one step at index 0: the second forward's t - 1 wraps to the last row
        kw.update(init_image=T("init_image"), skip_timesteps=9)
    return model, y, kw


def _count_calls(monkeypatch):
    from gesturediffusion_amd.engine import Engine
    calls = {"plms_loop": 0, "forward": 0}
    for name in calls:
        orig = getattr(Engine, name)

        def counted(self, *a, _orig=orig, _name=name, **k):
            calls[_name] += 1
            return _orig(self, *a, **k)
        monkeypatch.setattr(Engine, name, counted)
    return calls


@pytest.mark.parametrize("arch", ARCHS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("order", [2, 3, 4])
def test_fused_loop_equals_stepwise_bit_for_bit(arch, dtype, order, monkeypatch):
    """plms_sample_loop(fused=True) == fused=False on the tiny V1 / V2 in every compute mode: conditional, unconditional, CFG,
    inpainting, clip_denoised, init_image + skip_timesteps=3, and the single-step loop; the fused route is one gdx_plms_loop
    call and no step-wise forward."""
    g, m = _tiny(arch, dtype)
    df = _diffusion([10])
    x_T = torch.from_numpy(g["tape"])[0].to(dev())
    calls = _count_calls(monkeypatch)
    for name in VARIANTS:
        model, y, kw = _variant(name, g, m)
        kw = dict(kw, noise=x_T.clone(), model_kwargs={"y": y}, order=order)
        calls.update(plms_loop=0, forward=0)
        fused = df.plms_sample_loop(model, tuple(x_T.shape), **kw)
        assert calls == {"plms_loop": 1, "forward": 0}, (name, calls)
        step = df.plms_sample_loop(model, tuple(x_T.shape), fused=False, **kw)
        steps = 10 - kw.get("skip_timesteps", 0)
        assert calls == {"plms_loop": 1, "forward": steps + 1}, (name, calls)
        assert torch.isfinite(fused).all() and torch.equal(fused, step), name
        assert torch.equal(x_T, torch.from_numpy(g["tape"])[0].to(dev()))          # the caller's x_T is not written


@pytest.mark.parametrize("arch", ARCHS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_call_equals_blocks_of_three_steps(arch, dtype, monkeypatch):
    """run_steps / k_base: the loop issued in blocks of 3 steps (progress=True) carries its eps history in the caller's buffer
    and gives the bits of one call."""
    from gesturediffusion_amd.diffusion import gaussian_diffusion as gd
    g, m = _tiny(arch, dtype)
    df = _diffusion([10])
    x_T = torch.from_numpy(g["tape"])[0].to(dev())
    for name, order in [("cfg", 4), ("cond", 2), ("inpaint", 3), ("init_skip3", 4)]:
        model, y, kw = _variant(name, g, m)
        kw = dict(kw, noise=x_T.clone(), model_kwargs={"y": y}, order=order)
        one = df.plms_sample_loop(model, tuple(x_T.shape), **kw)
        calls = _count_calls(monkeypatch)
        monkeypatch.setattr(gd, "NOISE_BLOCK", 3)
        blocks = df.plms_sample_loop(model, tuple(x_T.shape), progress=True, **kw)
        monkeypatch.undo()
        assert calls["plms_loop"] == -(-(10 - kw.get("skip_timesteps", 0)) // 3)
        assert torch.equal(one, blocks), name


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("arch,B,T,J", [("mdm", 4, 60, 150), ("mdm_old", 2, 196, 263)])
def test_fused_equals_stepwise_at_real_shapes(arch, B, T, J, dtype):
    """d = 512, L = 8 on a 10-step respacing: V2 B=4 T=60 J=150 and V1 B=2 T=196 J=263 (J*T = 51548), plain and guided."""
    from gesturediffusion_amd.model.cfg_sampler import ClassifierFreeSampleModel
    from gesturediffusion_amd.utils.init import init_state_dict, synthetic_inputs
    cfg = dict(arch=arch, njoints=J, nfeats=1, latent_dim=512, ff_size=1024, num_layers=8, num_heads=4, seed_poses=10)
    m = build_model(arch, cfg, init_state_dict(cfg, seed=0))
    m.compute_dtype = dtype
    d = dev()
    x, seedp, mfcc = synthetic_inputs(cfg, B, T, seed=10)
    df = _diffusion([10])
    for guided, order in [(False, 3), (True, 2)]:
        y = {"seed": seedp.to(d), "mfcc": mfcc.to(d)}
        model = m
        if guided:
            y["scale"] = torch.full((B,), 2.5, device=d)
            model = ClassifierFreeSampleModel(m)
        kw = dict(noise=x.to(d), clip_denoised=False, model_kwargs={"y": y}, order=order)
        fused = df.plms_sample_loop(model, (B, J, 1, T), **kw)
        step = df.plms_sample_loop(model, (B, J, 1, T), fused=False, **kw)
        assert torch.isfinite(fused).all() and torch.equal(fused, step), (guided, order)


@pytest.mark.parametrize("arch", ARCHS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_loop_leaves_the_workspace_guards_intact(arch, dtype):
    g, m = _tiny(arch, dtype)
    d = dev()
    df = _diffusion([10])
    x_T = torch.from_numpy(g["tape"])[0].to(d)
    eng = m._get_engine(d)
    eng.set_guards(True)
    try:
        for name, order in [("cfg", 4), ("inpaint", 2), ("single_step", 3)]:
            model, y, kw = _variant(name, g, m)
            r = df.plms_sample_loop(model, tuple(x_T.shape), noise=x_T.clone(), model_kwargs={"y": y}, order=order, **kw)
            bad, zone = eng.check_guards(d)
            assert bad == 0, f"{name}: {bad} canary bytes overwritten, first in workspace allocation #{zone}"
            assert torch.isfinite(r).all()
    finally:
        eng.set_guards(False)


@pytest.mark.parametrize("arch", ARCHS)
@pytest.mark.parametrize("name,order", [("plms10_o2", 2), ("plms10_o3", 3), ("plms10_o4_cfg", 4), ("plms10_o2_inpaint", 2),
                                        ("plms10_o2_init_skip", 2)])
def test_fused_loop_vs_reference_golden(arch, name, order):
    """The reference's own PLMS runs, bounds as in test_gpu_parity.py::test_plms_loops_vs_reference_golden (LOOP_TOL; 2e-3 at
    order 4, where the multistep weights amplify fp32 forward differences)."""
    g, m = _tiny(arch, "fp32")
    gp = load_golden(f"plms_{arch}_tiny.npz")
    variant = "cfg" if "cfg" in name else "inpaint" if "inpaint" in name else "init_skip3" if "init" in name else "cond"
    model, y, kw = _variant(variant, g, m)
    x_T = torch.from_numpy(g["tape"])[0].to(dev())
    r = _diffusion([10]).plms_sample_loop(model, tuple(x_T.shape), noise=x_T.clone(), model_kwargs={"y": y}, order=order,
                                          fused=True, **kw)
    err = rel_err(r.cpu(), gp[name])
    print(f"plms-golden {arch} {name}: rel err {err:.3g}")
    assert err < (2e-3 if order == 4 else LOOP_TOL), name


def test_order_errors_are_raised_before_the_library_is_called(monkeypatch):
    g, m = _tiny("mdm", "fp32")
    model, y, kw = _variant("cond", g, m)
    x_T = torch.from_numpy(g["tape"])[0].to(dev())
    df = _diffusion([10])
    calls = _count_calls(monkeypatch)
    with pytest.raises(TypeError):
        df.plms_sample_loop(model, tuple(x_T.shape), noise=x_T.clone(), model_kwargs={"y": y}, order=1, fused=True, **kw)
    for order in (0, 5):
        with pytest.raises(ValueError, match="order is invalid"):
            df.plms_sample_loop(model, tuple(x_T.shape), noise=x_T.clone(), model_kwargs={"y": y}, order=order, fused=True, **kw)
    with pytest.raises(ValueError, match="rng must be"):
        df.plms_sample_loop(model, tuple(x_T.shape), model_kwargs={"y": y}, rng="numpy", **kw)
    assert calls == {"plms_loop": 0, "forward": 0}


def test_unprepared_handle_is_refused():
    """The one refusal of gdx_plms_loop that needs a handle."""
    import ctypes as C
    from gesturediffusion_amd import _lib
    from gesturediffusion_amd.engine import Engine
    fresh = Engine(1, 16, 128, 256, 2, 4, 10)
    a = _lib.PlmsLoopArgs(mode=0, order=2, num_steps=10, first_index=9, coef=4096, timestep_map=4096, x=4096, eps_hist=4096,
                          scratch=4096)
    assert fresh.lib.gdx_plms_loop(fresh.handle, C.byref(a), None) < 0 and b"gdx_prepare" in fresh.lib.gdx_last_error()


@pytest.mark.parametrize("arch", ARCHS)
def test_philox_x_T_is_shard_invariant(arch):
    """rng="philox": x_T is keyed by the global sample index, so a batch of 4 run as two shards of 2 (sample_offset 0 and 2)
    equals the whole batch bit for bit, on the fused and the step-wise route."""
    from gesturediffusion_amd.utils.init import synthetic_inputs
    g, m = _tiny(arch, "fp32")
    d = dev()
    cfg = dict(TINY, arch=arch)
    _, seedp, mfcc = synthetic_inputs(cfg, 4, 20, seed=4)
    y = {"seed": seedp.to(d), "mfcc": mfcc.to(d)}
    df = _diffusion([10])
    kw = dict(clip_denoised=False, order=3, rng="philox", philox_seed=21)
    whole = df.plms_sample_loop(m, (4, 16, 1, 20), model_kwargs={"y": y}, **kw)
    for lo in (0, 2):
        ys = {k: v[lo:lo + 2].contiguous() for k, v in y.items()}
        shard = df.plms_sample_loop(m, (2, 16, 1, 20), model_kwargs={"y": ys}, sample_offset=lo, **kw)
        assert torch.equal(shard, whole[lo:lo + 2]), lo
    assert torch.equal(whole, df.plms_sample_loop(m, (4, 16, 1, 20), model_kwargs={"y": y}, fused=False, **kw))
    other = df.plms_sample_loop(m, (4, 16, 1, 20), model_kwargs={"y": y}, **dict(kw, philox_seed=22))
    assert not torch.equal(other, whole)


def test_generate_cli_plms_equals_a_direct_call(tmp_path):
    """`sample.generate --synthetic --sampler plms --timestep_respacing ddim10`: the saved samples are those of a direct
    plms_sample_loop call on the inputs the CLI builds from its seed (weights, seed poses, MFCCs, Philox x_T)."""
    from gesturediffusion_amd.model.cfg_sampler import ClassifierFreeSampleModel
    from gesturediffusion_amd.sample import generate
    from gesturediffusion_amd.utils.init import MFCC_DIM, init_state_dict
    from gesturediffusion_amd.utils.model_util import create_model_and_diffusion
    from gesturediffusion_amd.utils.parser_util import generate_args
    out = tmp_path / "out"
    argv = ["--synthetic", "--latent_dim", "128", "--layers", "2", "--num_samples", "3", "--chunks", "1", "--synthetic_njoints", "37",
            "--output_dir", str(out), "--seed", "7", "--arch_version", "mdm", "--num_frames", "20", "--sampler", "plms",
            "--plms_order", "3", "--timestep_respacing", "ddim10", "--rng", "philox"]
    assert generate.main(argv) == 0
    res = np.load(out / "results.npy", allow_pickle=True).item()      # written by this test a moment ago
    assert res["motion"].shape == (3, 37, 1, 20) and np.isfinite(res["motion"]).all()
    d = dev()
    args = generate_args(argv)
    args.mfcc_input = True
    model, df = create_model_and_diffusion(args, None)
    assert df.num_timesteps == 10
    cfg = dict(arch="mdm", njoints=37, nfeats=1, latent_dim=128, ff_size=1024, num_layers=2, num_heads=4, seed_poses=args.seed_poses)
    model.load_state_dict(init_state_dict(cfg, seed=7), strict=False)
    model = ClassifierFreeSampleModel(model).to(d).eval()
    gen = torch.Generator().manual_seed(7)
    seedp = torch.randn(3, 37, 1, args.seed_poses, generator=gen)
    mfcc = torch.randn(3, MFCC_DIM, 1, 20, generator=gen)
    y = {"seed": seedp.to(d), "mfcc": mfcc.to(d), "scale": torch.ones(3, device=d) * args.guidance_param}
    want = df.plms_sample_loop(model, (3, 37, 1, 20), clip_denoised=False, model_kwargs={"y": y}, order=3, rng="philox",
                               philox_seed=7)
    assert np.array_equal(res["motion"], want.cpu().numpy())
