"""The pose-layout sampler kernels behind their float4 dispatch (sampler.hip; gdx_pose_host.h: vec_ok; gdx_pose_device.h: pred_xstart4, update_value): every
CFG / inpainting / clip_denoised combination of gdx_sampler_update against the torch-CPU expressions of oracle/sampler.py,
and gdx_bpd_terms on operands off 16-byte alignment against itself on aligned ones -- all by torch.equal."""
import itertools

import pytest
import torch

from misaligned import shifted as _shifted
from test_gpu_parity import dev

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("layout", ["tail", "float4", "shifted"])
@pytest.mark.parametrize("kind", ["p", "ddim_eta"])
def test_sampler_update_every_blend_bit_exact(kind, layout):
    """pred_xstart and out of gdx_sampler_update (ancestral, and DDIM with eta = 0.5) == u + s*(c - u) -> inpainting -> clamp
    -> p_sample_step / ddim_step on the CPU, for all eight CFG x inpainting x clip_denoised combinations; per-sample t rows
    0, 1, n//2, n-1, 3 and scales 2.5, 1, 0, -1, 3.  (5, 7, 1, 9): 63 elements per sample, the scalar tail; (5, 16, 1, 20): the
    float4 path; shifted: that shape with every tensor operand one element off alignment (the scalar path again)."""
    from gesturediffusion_amd import engine as E
    from gesturediffusion_amd._lib import GDX_SAMPLER_DDIM, GDX_SAMPLER_P
    from gesturediffusion_amd.diffusion import gaussian_diffusion as gd
    from gesturediffusion_amd.diffusion.respace import SpacedDiffusion, space_timesteps
    from oracle import sampler as osamp
    from oracle import schedule as osch
    d = dev()
    resp, eta, code = ([20], 0.0, GDX_SAMPLER_P) if kind == "p" else ("ddim100", 0.5, GDX_SAMPLER_DDIM)
    df = SpacedDiffusion(use_timesteps=space_timesteps(1000, resp), betas=gd.get_named_beta_schedule("cosine", 1000),
                         model_mean_type=gd.ModelMeanType.START_X, model_var_type=gd.ModelVarType.FIXED_SMALL,
                         loss_type=gd.LossType.MSE)
    tab, _ = osch.make_tables("cosine", 1000, resp)
    coef = df.coef_table(code, d, eta)
    n = tab.num_timesteps
    shape = (5, 7, 1, 9) if layout == "tail" else (5, 16, 1, 20)
    g = torch.Generator().manual_seed(11)
    c, u, x, z, motion = (torch.randn(*shape, generator=g) * s for s in (1.5, 1.5, 1.0, 1.0, 1.2))
    mask = torch.rand(*shape, generator=g) < 0.3
    scale = torch.tensor([2.5, 1.0, 0.0, -1.0, 3.0])
    t = torch.tensor([0, 1, n // 2, n - 1, 3])
    f = _shifted if layout == "shifted" else (lambda v: v)
    on = lambda v: f(v.to(d))   # noqa: E731
    for cfg, inp, clip in itertools.product([False, True], repeat=3):
        x0 = u + (scale.view(-1, 1, 1, 1) * (c - u)) if cfg else c
        if inp:
            x0 = osamp.inpaint(x0, {"inpainting_mask": mask, "inpainted_motion": motion})
        x0 = osamp.process_xstart(x0, clip_denoised=clip)
        want = osamp.p_sample_step(tab, x0, x, t, z) if kind == "p" else osamp.ddim_step(tab, x0, x, t, z, eta)
        out, pred = f(torch.empty(shape, device=d)), f(torch.empty(shape, device=d))
        E.sampler_update(code, coef, on(x), on(c), out, t=t.to(d), x0_uncond=on(u) if cfg else None,
                         scale=on(scale) if cfg else None, inpaint_mask=on(mask) if inp else None,
                         inpaint_motion=on(motion) if inp else None, noise=on(z), pred_xstart=pred, clip_denoised=clip)
        assert torch.equal(pred.cpu(), x0), (cfg, inp, clip)
        assert torch.equal(out.cpu(), want), (cfg, inp, clip)


def test_bpd_terms_shifted_operands_give_the_aligned_bits():
    """gdx_bpd_terms at (5, 16, 1, 20): operands one element off alignment take the scalar path, whose summation order is the
    float4 path's (a function of J*T alone), so the three sums and pred_xstart are those of the aligned call."""
    from gesturediffusion_amd import engine as E
    from gesturediffusion_amd.diffusion import gaussian_diffusion as gd
    d = dev()
    df = gd.GaussianDiffusion(betas=gd.get_named_beta_schedule("cosine", 1000), model_mean_type=gd.ModelMeanType.START_X,
                              model_var_type=gd.ModelVarType.FIXED_LARGE, loss_type=gd.LossType.MSE)
    coef = df.bpd_table(d)
    gen = torch.Generator().manual_seed(320)
    shape = (5, 16, 1, 20)
    x0, z, oc, ou, motion = ((torch.randn(*shape, generator=gen) * s).to(d) for s in (0.6, 1.0, 0.9, 0.9, 0.5))
    mask = (torch.rand(*shape, generator=gen) < 0.2).to(d)
    t = torch.tensor([0, 1, 17, 500, 999], device=d)
    scale = torch.tensor([2.5, 1.0, 0.0, -1.0, 3.0], device=d)
    xt = df.q_sample(x0, t, noise=z)
    for cfg, inp in itertools.product([False, True], repeat=2):
        def run(f):
            return E.bpd_terms(coef, f(x0), f(xt), f(oc), noise=f(z), t=t, x0_uncond=f(ou) if cfg else None,
                               scale=scale if cfg else None, inpaint_mask=f(mask) if inp else None,
                               inpaint_motion=f(motion) if inp else None, clip_denoised=True)
        for name, a, w in zip(("vb", "xstart_mse", "mse", "pred_xstart"), run(_shifted), run(lambda v: v)):
            assert torch.isfinite(w).all(), (name, cfg, inp)
            assert torch.equal(a, w), (name, cfg, inp)
