#!/usr/bin/env python3
"""Outputs of the sampler kernels of two builds of libgdx.so, bit for bit (needs an MI355X).

    python tools/sampler_ab.py OLD_LIBGDX_SO NEW_LIBGDX_SO

Each library runs, in a fresh child process of its own (GDX_LIBGDX), one after the other, every public sampler entry point on
the same seeded inputs and reports a SHA-256 per output: gdx_sampler_update (P / DDIM x CFG x inpainting x clip x tape /
Philox x cond_grad), gdx_plms_update kinds 0-8, gdx_plms_step kinds 1-6, gdx_dpm_step orders 1-3, gdx_dpm_sde_step orders 1-2
(tape / Philox), gdx_cfg_rescale, gdx_bpd_terms (also with its mask one byte off) and its prior mode, gdx_q_sample(_t) and
gdx_randn, each at (B, J, T) = (5, 16, 20) and (5, 7, 9) and with the operands one float off 16-byte alignment; then 6-step
loops of the tiny model (T = 20, CFG + clip): gdx_sample_loop (Philox noise: the token-major path), plms_sample_loop,
dpm_solver_sample_loop (order 3) and dpm_solver_sde_sample_loop (order 2, Philox), in fp32, fp16 and bf16.
Prints one line per output and a summary line; exit status 1 on any difference."""
import hashlib
import itertools
import json
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(arch="mdm", njoints=16, nfeats=1, latent_dim=128, ff_size=256, num_layers=2, num_heads=4, seed_poses=10)


def child(out_path):
    sys.path.insert(0, REPO)
    import torch
    from gesturediffusion_amd import engine as E
    from gesturediffusion_amd.diffusion import gaussian_diffusion as gd
    from gesturediffusion_amd.diffusion.respace import SpacedDiffusion, space_timesteps
    from gesturediffusion_amd.model.cfg_sampler import ClassifierFreeSampleModel
    from gesturediffusion_amd.model.mdm import MDM
    from gesturediffusion_amd.utils.init import init_state_dict, synthetic_inputs
    dev = torch.device("cuda:0")
    report = {}

    def put(name, *tensors):
        for i, t in enumerate(tensors):
            if t is not None:
                report[f"{name}.{i}"] = hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()

    def shifted(t):
        buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        return v

    def diffusion(resp, var="FIXED_SMALL"):
        return SpacedDiffusion(use_timesteps=space_timesteps(1000, resp), betas=gd.get_named_beta_schedule("cosine", 1000),
                               model_mean_type=gd.ModelMeanType.START_X, model_var_type=getattr(gd.ModelVarType, var),
                               loss_type=gd.LossType.MSE)

    df = diffusion([20])
    n = df.num_timesteps
    coefs = {0: df.coef_table(0, dev, 0.0), 1: df.coef_table(1, dev, 0.5)}
    bpd_coef = diffusion([20], "FIXED_LARGE").bpd_table(dev)
    dpm_coef, sde_coef = df.dpm_coef_table(dev), df.dpm_sde_coef_table(dev, 1.0)

    class Lib:                                           # Engine.cfg_rescale needs nothing of a handle but the library
        lib = E._lib.load()
    for (J, T), shift in [((16, 20), False), ((7, 9), False), ((16, 20), True)]:
        tag = f"J{J}T{T}{'s' if shift else ''}"
        shape = (5, J, 1, T)
        g = torch.Generator().manual_seed(J * T)
        f = shifted if shift else (lambda v: v)
        rnd = lambda s=1.0: f((torch.randn(shape, generator=g) * s).to(dev))   # noqa: E731
        x, oc, ou, motion, z, grad, x_eps, pred_prev = rnd(), rnd(1.5), rnd(1.5), rnd(1.2), rnd(), rnd(0.1), rnd(), rnd()
        hist = [rnd() for _ in range(3)]
        mask = f((torch.rand(shape, generator=g) < 0.3).to(dev))
        scale = torch.tensor([2.5, 1.0, 0.0, -1.0, 3.0], device=dev)
        t = torch.tensor([0, 1, n // 2, n - 1, 3], device=dev)
        t2 = (t - 1) % n
        s1m = torch.linspace(0.05, 0.95, n, device=dev)
        new = lambda: f(torch.empty(shape, device=dev))   # noqa: E731
        for kind, cfg, inp, clip, tape, cond in itertools.product((0, 1), *[(False, True)] * 5):
            out, pred = new(), new()
            E.sampler_update(kind, coefs[kind], x, oc, out, t=t, x0_uncond=ou if cfg else None, scale=scale if cfg else None,
                             inpaint_mask=mask if inp else None, inpaint_motion=motion if inp else None,
                             noise=z if tape else None, philox_seed=77, sample_offset=3, rng_step=5, pred_xstart=pred,
                             cond_grad=grad if cond else None, cond_coef=s1m if cond and kind else None, clip_denoised=clip)
            put(f"update.{tag}.k{kind}.cfg{cfg:d}.inp{inp:d}.clip{clip:d}.tape{tape:d}.cond{cond:d}", out, pred)
        for kind in range(9):
            e = [hist[0], s1m, hist[2], hist[1]] if kind == 7 else [hist[0], hist[1], hist[2], x_eps]
            put(f"plms_update.{tag}.k{kind}", E.plms_update(kind, coefs[1], t, x, oc, eps=e, out=new()))
        for kind, cfg, inp, clip in itertools.product(range(1, 7), *[(False, True)] * 3):
            out, eps, pred = new(), new(), new()
            E.plms_step(kind, coefs[1], x, oc, out, eps_out=eps, eps_hist=hist, t=t, x0_uncond=ou if cfg else None,
                        scale=scale if cfg else None, inpaint_mask=mask if inp else None,
                        inpaint_motion=motion if inp else None, clip_denoised=clip, pred_xstart=pred,
                        x_eps=x_eps if kind == 5 else None, t_eps=t2 if kind == 5 else None,
                        pred_prev=pred_prev if kind == 5 else None)
            put(f"plms_step.{tag}.k{kind}.cfg{cfg:d}.inp{inp:d}.clip{clip:d}", out, eps, pred)
        for order, cfg, inp, clip in itertools.product((1, 2, 3), *[(False, True)] * 3):
            guide = dict(t=t, x0_uncond=ou if cfg else None, scale=scale if cfg else None, inpaint_mask=mask if inp else None,
                         inpaint_motion=motion if inp else None, clip_denoised=clip)
            out, pred = new(), new()
            E.dpm_step(order, dpm_coef, x, oc, out, hist=hist[:order - 1], pred_out=pred, **guide)
            put(f"dpm_step.{tag}.o{order}.cfg{cfg:d}.inp{inp:d}.clip{clip:d}", out, pred)
            for tape in (False, True) if order < 3 else ():
                out, pred = new(), new()
                E.dpm_sde_step(order, sde_coef, x, oc, out, hist=hist[:order - 1], pred_out=pred, noise=z if tape else None,
                               philox_seed=77, sample_offset=3, rng_step=5, **guide)
                put(f"dpm_sde_step.{tag}.o{order}.cfg{cfg:d}.inp{inp:d}.clip{clip:d}.tape{tape:d}", out, pred)
        for tt, iv in ((None, None), (t, (1, n // 2))):
            put(f"cfg_rescale.{tag}.t{tt is not None:d}", *E.Engine.cfg_rescale(Lib, oc, ou, scale, 0.7, t=tt, interval=iv, out=new()))
        x0 = rnd(0.6)
        xt = f(E.q_sample_t(x0, z, coefs[0], t))
        put(f"q_sample_t.{tag}", xt, E.q_sample(x0, z, coefs[0], 7))
        for cfg, inp, clip in itertools.product((False, True), repeat=3):
            put(f"bpd_terms.{tag}.cfg{cfg:d}.inp{inp:d}.clip{clip:d}",
                *E.bpd_terms(bpd_coef, x0, xt, oc, noise=z, t=t, x0_uncond=ou if cfg else None, scale=scale if cfg else None,
                             inpaint_mask=mask if inp else None, inpaint_motion=motion if inp else None, clip_denoised=clip))
        mask1 = torch.zeros(mask.numel() + 8, dtype=torch.bool, device=dev)[1:1 + mask.numel()].view(shape)
        mask1.copy_(mask)
        put(f"bpd_terms.{tag}.mask1", *E.bpd_terms(bpd_coef, x0, xt, oc, noise=z, t=t, x0_uncond=ou, scale=scale, inpaint_mask=mask1,
                                                    inpaint_motion=motion, clip_denoised=True))
        put(f"bpd_terms.{tag}.mean", *E.bpd_terms(bpd_coef, x0, xt, oc, noise=z, t=t, model_mean=pred_prev))
        put(f"bpd_prior.{tag}", E.bpd_prior(bpd_coef, x0, n - 1, -0.25))
        z_out = new()
        E._lib.check(E._lib.load().gdx_randn(z_out.data_ptr(), 5, J * T, 123456789012345, 5, 17, E._stream(dev)), E._lib.load())
        put(f"randn.{tag}", z_out)

    loop_df = diffusion([6])
    for dtype in ("fp32", "fp16", "bf16"):
        m = MDM(njoints=16, nfeats=1, translation=True, pose_rep="rot6d", glob=True, glob_rot=True, latent_dim=128, ff_size=256,
                num_layers=2, num_heads=4, data_rep="genea_vec", cond_mask_prob=0.1, dataset="genea2023", mfcc_input=True,
                seed_poses=10, compute_dtype=dtype)
        m.load_state_dict(init_state_dict(TINY, seed=31, perturb=True), strict=False)
        m.to(dev).eval()
        _, seedp, mfcc = synthetic_inputs(TINY, 3, 20, seed=5)
        y = {"seed": seedp.to(dev), "mfcc": mfcc.to(dev), "scale": torch.tensor([2.5, 1.0, 0.5], device=dev)}
        kw = dict(clip_denoised=True, model_kwargs={"y": y}, rng="philox", philox_seed=9)
        cfg_model = ClassifierFreeSampleModel(m)
        put(f"sample_loop.{dtype}", loop_df.p_sample_loop(cfg_model, (3, 16, 1, 20), **kw))
        put(f"plms_loop.{dtype}", loop_df.plms_sample_loop(cfg_model, (3, 16, 1, 20), order=2, **kw))
        put(f"dpm_loop.{dtype}", loop_df.dpm_solver_sample_loop(cfg_model, (3, 16, 1, 20), order=3, **kw))
        put(f"dpm_sde_loop.{dtype}", loop_df.dpm_solver_sde_sample_loop(cfg_model, (3, 16, 1, 20), order=2, **kw))
    json.dump(report, open(out_path, "w"))


def main():
    if sys.argv[1] == "--child":
        return child(sys.argv[2])
    libs = [os.path.abspath(p) for p in sys.argv[1:3]]
    reports = []
    with tempfile.TemporaryDirectory() as tmp:
        for i, lib in enumerate(libs):
            path = os.path.join(tmp, f"report{i}.json")
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], check=True, timeout=240,
                           env=dict(os.environ, GDX_LIBGDX=lib))
            reports.append(json.load(open(path)))
    old, new = reports
    bad = 0
    for name in sorted(set(old) | set(new)):
        same = old.get(name) == new.get(name)
        bad += not same
        print("%-60s old %s  new %s  %s" % (name, old.get(name), new.get(name), "identical" if same else "DIFFERENT"))
    print("# %d outputs compared, %d differences" % (len(set(old) | set(new)), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
