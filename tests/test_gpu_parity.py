"""Parity tests proper: the HIP path (through the C ABI, via the drop-in nn.Modules) against
the golden fixtures produced by the reference and against the CPU oracle.  Need an MI355X.

Tolerances (fp32 path): sampler update bit-exact; single forward
maxabs(err) <= 1e-4 * maxabs(ref); end of loop (tape-replayed noise) <= 1e-3 * maxabs(ref).
Measured values are far inside these; the asserts use 2e-5 / 2e-4 so regressions show early.
"""
import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err, weights_from

pytestmark = pytest.mark.gpu

FWD_TOL = 2e-5
LOOP_TOL = 2e-4
TINY = dict(njoints=16, nfeats=1, latent_dim=128, ff_size=256, num_layers=2, num_heads=4, seed_poses=10)


def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


def build_model(arch, cfg, weights, cond_mask_prob=0.1):
    from gesturediffusion_amd.model.mdm import MDM
    from gesturediffusion_amd.model.mdm_old import MDM_Old
    kw = dict(njoints=cfg["njoints"], nfeats=1, translation=True, pose_rep="rot6d", glob=True, glob_rot=True,
              latent_dim=cfg["latent_dim"], ff_size=cfg["ff_size"], num_layers=cfg["num_layers"],
              num_heads=cfg["num_heads"], dropout=0.1, activation="gelu", data_rep="genea_vec",
              cond_mask_prob=cond_mask_prob, dataset="genea2023", use_text=False, mfcc_input=True, use_wav_enc=False,
              seed_poses=cfg["seed_poses"], use_audio=False, modeltype="", clip_version="ViT-B/32")
    m = (MDM if arch == "mdm" else MDM_Old)(**kw)
    missing, unexpected = m.load_state_dict(weights, strict=False)
    assert not unexpected
    assert all(k.endswith(".pe") or k.endswith("inv_freq") for k in missing), missing
    m.to(dev())
    m.eval()
    return m


def test_library_loaded_is_in_tree():
    from gesturediffusion_amd import _lib
    lib = _lib.load()
    assert _lib.LIB_PATH.endswith("gesturediffusion_amd/csrc/libgdx.so")
    assert lib.gdx_forward is not None


@pytest.mark.parametrize("arch", ["mdm", "mdm_old"])
@pytest.mark.parametrize("uncond", [False, True])
def test_forward_tiny_vs_reference_golden(arch, uncond):
    g = load_golden(f"forward_{arch}_tiny.npz")
    m = build_model(arch, TINY, weights_from(g))
    d = dev()
    y = {"seed": torch.from_numpy(g["seed"]).to(d), "mfcc": torch.from_numpy(g["mfcc"]).to(d)}
    if uncond:
        y["uncond"] = True
    eng = m._get_engine(d)
    eng.keep_taps(True)
    out = m(torch.from_numpy(g["x"]).to(d), torch.from_numpy(g["t"]).to(d), y)
    tag = "uncond." if uncond else "cond."
    B, T, dm = g["x"].shape[0], g["x"].shape[-1], TINY["latent_dim"]
    S = T + 1
    # stage by stage: encoder input and every encoder layer ([S,B,d] in the reference, [B,S,d] here)
    want = torch.from_numpy(g[tag + "tap.enc_in"]).permute(1, 0, 2).reshape(B * S, dm)
    got = eng.tap(0, 2 * B * S, dm, d)[: B * S].cpu()
    assert rel_err(got, want) < FWD_TOL, "encoder input"
    for l in range(TINY["num_layers"]):
        want = torch.from_numpy(g[tag + f"tap.seqTransEncoder.layers.{l}.out"]).permute(1, 0, 2).reshape(B * S, dm)
        got = eng.tap(l + 1, 2 * B * S, dm, d)[: B * S].cpu()
        assert rel_err(got, want) < FWD_TOL, f"layer {l}"
    assert out.shape == g[tag + "out"].shape
    assert rel_err(out.cpu(), g[tag + "out"]) < FWD_TOL
    eng.keep_taps(False)


@pytest.mark.parametrize("arch", ["mdm", "mdm_old"])
def test_forward_error_vs_fp64_is_at_noise_floor(arch):
    g = load_golden(f"forward_{arch}_tiny.npz")
    m = build_model(arch, TINY, weights_from(g))
    d = dev()
    y = {"seed": torch.from_numpy(g["seed"]).to(d), "mfcc": torch.from_numpy(g["mfcc"]).to(d)}
    out = m(torch.from_numpy(g["x"]).to(d), torch.from_numpy(g["t"]).to(d), y).cpu()
    floor = rel_err(g["cond.out"], g["cond.out_fp64"])       # the reference's own fp32 error
    ours = rel_err(out, g["cond.out_fp64"])
    assert ours < 10 * max(floor, 1e-7), (ours, floor)


@pytest.mark.parametrize("kind", ["p", "ddim", "ddim_eta"])
def test_sampler_update_bit_exact(kind):
    from gesturediffusion_amd import engine as E
    from gesturediffusion_amd._lib import GDX_SAMPLER_DDIM, GDX_SAMPLER_P
    from gesturediffusion_amd.diffusion import gaussian_diffusion as gd
    from gesturediffusion_amd.diffusion.respace import SpacedDiffusion, space_timesteps
    from oracle import sampler as osamp
    from oracle import schedule as osch
    d = dev()
    resp = [20] if kind == "p" else "ddim100"
    eta = 0.5 if kind == "ddim_eta" else 0.0
    df = SpacedDiffusion(use_timesteps=space_timesteps(1000, resp), betas=gd.get_named_beta_schedule("cosine", 1000),
                         model_mean_type=gd.ModelMeanType.START_X, model_var_type=gd.ModelVarType.FIXED_SMALL,
                         loss_type=gd.LossType.MSE)
    tab, _ = osch.make_tables("cosine", 1000, resp)
    g = torch.Generator().manual_seed(5)
    B, J, T = 5, 37, 23          # per-sample count not a multiple of 4 -> scalar tail path
    for shape in [(B, J, 1, T), (B, 16, 1, 20)]:
        x0, x, z = (torch.randn(*shape, generator=g) for _ in range(3))
        n = tab.num_timesteps
        t = torch.tensor([0, 1, n // 2, n - 1, 3][: shape[0]])
        k = GDX_SAMPLER_P if kind == "p" else GDX_SAMPLER_DDIM
        out = torch.empty(shape, device=d)
        E.sampler_update(k, df.coef_table(k, d, eta), x.to(d), x0.to(d), out, t=t.to(d), noise=z.to(d))
        want = osamp.p_sample_step(tab, x0, x, t, z) if kind == "p" else osamp.ddim_step(tab, x0, x, t, z, eta)
        assert torch.equal(out.cpu(), want), kind


def test_sampler_update_cfg_inpaint_bit_exact():
    from gesturediffusion_amd import engine as E
    from gesturediffusion_amd._lib import GDX_SAMPLER_P
    from gesturediffusion_amd.diffusion import gaussian_diffusion as gd
    from oracle import sampler as osamp
    from oracle import schedule as osch
    d = dev()
    df = gd.GaussianDiffusion(betas=gd.get_named_beta_schedule("cosine", 1000), model_mean_type=gd.ModelMeanType.START_X,
                              model_var_type=gd.ModelVarType.FIXED_SMALL, loss_type=gd.LossType.MSE)
    tab, _ = osch.make_tables("cosine", 1000, "")
    g = torch.Generator().manual_seed(6)
    shape = (3, 16, 1, 20)
    c, u, x, z, motion = (torch.randn(*shape, generator=g) for _ in range(5))
    mask = torch.rand(*shape, generator=g) < 0.3
    scale = torch.tensor([2.5, 1.0, 0.0])
    t = torch.tensor([999, 500, 0])
    out = torch.empty(shape, device=d)
    pred = torch.empty(shape, device=d)
    E.sampler_update(GDX_SAMPLER_P, df.coef_table(GDX_SAMPLER_P, d), x.to(d), c.to(d), out, t=t.to(d), x0_uncond=u.to(d),
                     scale=scale.to(d), inpaint_mask=mask.to(d), inpaint_motion=motion.to(d), noise=z.to(d),
                     pred_xstart=pred)
    x0 = u + (scale.view(-1, 1, 1, 1) * (c - u))
    x0 = osamp.inpaint(x0, {"inpainting_mask": mask, "inpainted_motion": motion})
    assert torch.equal(pred.cpu(), x0)
    assert torch.equal(out.cpu(), osamp.p_sample_step(tab, x0, x, t, z))


def test_philox_matches_oracle():
    from gesturediffusion_amd import engine as E
    from oracle import philox as op
    d = dev()
    for shape, seed, off, step in [((3, 16, 1, 20), 10, 0, 0), ((2, 7, 1, 9), 123456789012345, 5, 17)]:
        got = E.randn(shape, d, seed, off, step).cpu().numpy().reshape(shape[0], -1)
        want = op.normal(shape[0], got.shape[1], seed, off, step)
        assert np.abs(got - want).max() < 2e-5          # libm vs device log/sin/cos rounding
    big = E.randn((64, 263, 1, 196), d, 10, 0, 3)
    assert abs(float(big.mean())) < 2e-3 and abs(float(big.std()) - 1) < 2e-3
    # shard invariance: samples 8..11 drawn as a shard equal rows 8..11 of the full batch
    part = E.randn((4, 263, 1, 196), d, 10, 8, 3)
    assert torch.equal(part, big[8:12])


def _diffusion(resp):
    from gesturediffusion_amd.diffusion import gaussian_diffusion as gd
    from gesturediffusion_amd.diffusion.respace import SpacedDiffusion, space_timesteps
    return SpacedDiffusion(use_timesteps=space_timesteps(1000, resp), betas=gd.get_named_beta_schedule("cosine", 1000),
                           model_mean_type=gd.ModelMeanType.START_X, model_var_type=gd.ModelVarType.FIXED_SMALL,
                           loss_type=gd.LossType.MSE)


LOOPS = ["p20", "p20_cfg", "ddim10", "ddim10_cfg", "ddim10_eta05", "p20_const_noise", "p20_dump", "p20_init_skip",
         "p20_skip_only", "p20_inpaint", "p20_cfg_inpaint"]


@pytest.mark.parametrize("arch", ["mdm", "mdm_old"])
@pytest.mark.parametrize("name", LOOPS)
@pytest.mark.parametrize("fused", [True, False])
def test_loops_tiny_vs_reference_golden(arch, name, fused):
    """Whole sampling loops with the reference's recorded noise tape: fused C++ loop
    (gdx_sample_loop) and the step-wise callable protocol (model(x, t, y) + gdx_sampler_update)."""
    _run_loop_case(arch, name, fused, "fp32", LOOP_TOL)


def _run_loop_case(arch, name, fused, compute_dtype, tol):
    from gesturediffusion_amd.model.cfg_sampler import ClassifierFreeSampleModel
    g = load_golden(f"loops_{arch}_tiny.npz")
    d = dev()
    m = build_model(arch, TINY, weights_from(g))
    m.compute_dtype = compute_dtype
    tape = torch.from_numpy(g["tape"]).to(d)
    y = {"seed": torch.from_numpy(g["seed"]).to(d), "mfcc": torch.from_numpy(g["mfcc"]).to(d)}
    model = m
    if "cfg" in name:
        y["scale"] = torch.from_numpy(g["scale"]).to(d)
        model = ClassifierFreeSampleModel(m)
    if "inpaint" in name:
        y["inpainting_mask"] = torch.from_numpy(g["inpainting_mask"]).to(d)
        y["inpainted_motion"] = torch.from_numpy(g["inpainted_motion"]).to(d)
    kw = dict(clip_denoised=False, model_kwargs={"y": y}, progress=False)
    if name.startswith("p20"):
        df, fn = _diffusion([20]), "p_sample_loop"
    else:
        df, fn = _diffusion("ddim10"), "ddim_sample_loop"
    if name == "p20_const_noise":
        kw["const_noise"] = True
    if name == "p20_dump":
        kw["dump_steps"] = [0, 9, 19]
    if name == "p20_init_skip":
        kw.update(init_image=torch.from_numpy(g["init_image"]).to(d), skip_timesteps=5)
    if name == "p20_skip_only":
        kw["skip_timesteps"] = 8
    if name == "ddim10_eta05":
        kw["eta"] = 0.5
    shape = tuple(tape[0].shape)
    if fused:
        r = getattr(df, fn)(model, shape, noise_tape=tape, **kw)
    else:
        # step-wise path with torch.randn_like replaced by the tape (harness-side, like the fixture generator)
        k = {"i": 1}
        orig = torch.randn_like

        def fake(x, *a, **kk):
            z = tape[k["i"]]
            k["i"] += 1
            return z
        torch.randn_like = fake
        try:
            r = getattr(df, fn)(model, shape, noise=tape[0].clone(), fused=False, **kw)
        finally:
            torch.randn_like = orig
    r = torch.stack(list(r)) if isinstance(r, list) else r
    assert rel_err(r.cpu(), g[name]) < tol, name


@pytest.mark.parametrize("arch", ["mdm", "mdm_old"])
def test_ddim_reverse_vs_reference_golden(arch):
    g = load_golden(f"loops_{arch}_tiny.npz")
    d = dev()
    m = build_model(arch, TINY, weights_from(g))
    y = {"seed": torch.from_numpy(g["seed"]).to(d), "mfcc": torch.from_numpy(g["mfcc"]).to(d)}
    df = _diffusion("ddim10")
    x = torch.from_numpy(g["tape"])[0].to(d)
    for ti in (0, 1, 2):
        x = df.ddim_reverse_sample(m, x, torch.full((x.shape[0],), ti, device=d), clip_denoised=False,
                                   model_kwargs={"y": y})["sample"]
    assert rel_err(x.cpu(), g["ddim10_reverse3"]) < LOOP_TOL


def _real_cfg(arch, J, d):
    return dict(arch=arch, njoints=J, nfeats=1, latent_dim=d, ff_size=1024, num_layers=8, num_heads=4, seed_poses=10)


@pytest.mark.parametrize("name,arch,J,dm", [("c1_v2", "mdm", 150, 512), ("c2_v1", "mdm_old", 263, 512),
                                            ("c2_v2", "mdm", 263, 512), ("c5_v2", "mdm", 498, 1024)])
def test_real_shapes_vs_reference_golden(name, arch, J, dm):
    """BASELINE.json configs at their real model sizes (small batch): outputs produced by the
    reference, weights/inputs regenerated here from the deterministic initialiser."""
    from gesturediffusion_amd.utils.init import init_state_dict, synthetic_inputs
    g = load_golden("real_shapes.npz")
    B, T = int(g[name + ".meta"][0]), int(g[name + ".meta"][1])
    cfg = _real_cfg(arch, J, dm)
    m = build_model(arch, cfg, init_state_dict(cfg, seed=0))
    x, seedp, mfcc = synthetic_inputs(cfg, B, T, seed=10)
    d = dev()
    t = torch.from_numpy(g[name + ".t"]).to(d)
    y = {"seed": seedp.to(d), "mfcc": mfcc.to(d)}
    out = m(x.to(d), t, y)
    assert rel_err(out.cpu(), g[name + ".out"]) < FWD_TOL
    out_u = m(x.to(d), t, dict(y, uncond=True))
    assert rel_err(out_u.cpu(), g[name + ".out_uncond"]) < FWD_TOL
    if name == "c1_v2":
        # config 1 end to end: 10-step DDIM, B=4, T=60 against the reference's own loop
        gen = torch.Generator().manual_seed(77)
        tape = torch.randn(11, B, J, 1, T, generator=gen).to(d)
        r = _diffusion("ddim10").ddim_sample_loop(m, (B, J, 1, T), noise_tape=tape, clip_denoised=False,
                                                   model_kwargs={"y": y})
        assert rel_err(r.cpu(), g["c1_v2.ddim10"]) < LOOP_TOL


@pytest.mark.parametrize("arch,dm,H,T,B", [("mdm_old", 256, 4, 37, 3), ("mdm", 256, 4, 40, 2), ("mdm_old", 512, 4, 15, 5),
                                            ("mdm_old", 128, 2, 250, 1), ("mdm", 512, 8, 30, 2), ("mdm", 1024, 4, 20, 2),
                                            ("mdm", 512, 4, 10, 3), ("mdm", 256, 4, 70, 5),
                                            ("mdm_old", 96, 3, 37, 3), ("mdm", 96, 3, 40, 2)])
def test_forward_vs_oracle_odd_shapes(arch, dm, H, T, B):
    """Shapes outside the fixtures: head_dim 64 (attention3's second instantiation), sequences that are
    not multiples of the 16/32-token blocks, a single sample, 8 heads, K = 263+ tails -- against the CPU oracle.  The V2
    rows run the fp32-MFMA local-attention front end at its three head widths (d / 8 = 32, 64, 128), with one window
    only (T = 10), and with a work count that is not a multiple of the four waves of a block (5 x 8 x 7 windows).
    The d = 96 rows (3 heads, ff_size 160) are the widths that are multiples of 32 but not of 64: every encoder GEMM
    (N = 96, 288, 160) is refused by the persistent kernel and runs on csrc/gemm.hip (tests/test_gpu_gemm_f32.py tests that
    kernel alone at these widths)."""
    from gesturediffusion_amd.utils.init import init_state_dict, synthetic_inputs
    from oracle import mdm_forward as omf
    cfg = dict(arch=arch, njoints=37, nfeats=1, latent_dim=dm, ff_size=160 if dm == 96 else 192, num_layers=2, num_heads=H,
               seed_poses=10)
    sd = init_state_dict(cfg, seed=5, perturb=True)
    m = build_model(arch, cfg, sd)
    d = dev()
    x, seedp, mfcc = synthetic_inputs(cfg, B, T, seed=11)
    t = (torch.arange(B) * 97 + 3) % 1000
    out = m(x.to(d), t.to(d), {"seed": seedp.to(d), "mfcc": mfcc.to(d)})
    with torch.no_grad():
        want = omf.forward(sd, cfg, x, t, {"seed": seedp, "mfcc": mfcc})
    assert rel_err(out.cpu(), want) < FWD_TOL


def test_cfg_forward_matches_two_pass_blend():
    from gesturediffusion_amd.model.cfg_sampler import ClassifierFreeSampleModel
    from gesturediffusion_amd.utils.init import init_state_dict, synthetic_inputs
    cfg = _real_cfg("mdm_old", 263, 512)
    m = build_model("mdm_old", cfg, init_state_dict(cfg, seed=0))
    d = dev()
    x, seedp, mfcc = synthetic_inputs(cfg, 3, 196, seed=4)
    t = torch.tensor([10, 500, 999], device=d)
    y = {"seed": seedp.to(d), "mfcc": mfcc.to(d), "scale": torch.tensor([2.5, 0.0, 1.0], device=d)}
    c = m(x.to(d), t, y)
    u = m(x.to(d), t, dict(y, uncond=True))
    blend = ClassifierFreeSampleModel(m)(x.to(d), t, y)
    want = u + y["scale"].view(-1, 1, 1, 1) * (c - u)
    assert rel_err(blend.cpu(), want.cpu()) < 1e-6
    assert rel_err(blend[1].cpu(), u[1].cpu()) < 1e-6       # scale 0 -> uncond
    assert rel_err(blend[2].cpu(), c[2].cpu()) < 1e-6       # scale 1 -> cond


def test_full_size_properties_config2():
    """BASELINE config 2 size (B=64, T=196, d=512, L=8): size-independent properties.
    (a) samples are independent: row b of a batch-64 forward equals the same sample run in a
        batch of 2, bit for bit (same kernels, same per-row arithmetic);
    (b) against the CPU oracle on 2 rows of the full batch (the oracle at B=64 takes ~1.5 s/step);
    (c) Philox loop is shard invariant: samples 8..11 sampled as a 4-sample shard with
        sample_offset=8 equal rows 8..11 of the 64-sample run (5 steps)."""
    from gesturediffusion_amd.utils.init import init_state_dict, synthetic_inputs
    from oracle import mdm_forward as omf
    cfg = _real_cfg("mdm_old", 263, 512)
    sd = init_state_dict(cfg, seed=0)
    m = build_model("mdm_old", cfg, sd)
    d = dev()
    B, T = 64, 196
    x, seedp, mfcc = synthetic_inputs(cfg, B, T, seed=10)
    t = torch.full((B,), 321, device=d)
    y = {"seed": seedp.to(d), "mfcc": mfcc.to(d)}
    full = m(x.to(d), t, y)
    assert torch.isfinite(full).all()
    sub = m(x[40:42].to(d), t[:2], {"seed": seedp[40:42].to(d), "mfcc": mfcc[40:42].to(d)})
    assert torch.equal(full[40:42], sub)
    with torch.no_grad():
        want = omf.forward(sd, cfg, x[40:42], torch.full((2,), 321), {"seed": seedp[40:42], "mfcc": mfcc[40:42]})
    assert rel_err(full[40:42].cpu(), want) < FWD_TOL
    df = _diffusion([5])
    r64 = df.p_sample_loop(m, (B, 263, 1, T), clip_denoised=False, model_kwargs={"y": y}, rng="philox", philox_seed=10)
    y4 = {"seed": seedp[8:12].to(d), "mfcc": mfcc[8:12].to(d)}
    r4 = df.p_sample_loop(m, (4, 263, 1, T), clip_denoised=False, model_kwargs={"y": y4}, rng="philox", philox_seed=10,
                          sample_offset=8)
    assert torch.equal(r64[8:12], r4)


@pytest.mark.parametrize("arch,B,T", [("mdm_old", 256, 196), ("mdm", 64, 200), ("mdm", 256, 200)])
def test_full_size_properties_configs_3_4(arch, B, T):
    """BASELINE configs 3 / 4 per-GPU sizes (B = 256, with classifier-free guidance an effective batch of 512 rows:
    M = 100 864 GEMM rows, 2 048 attention workgroups) and the V2 topology at its full size: rows of the big batch equal
    the same samples run as a batch of 2, bit for bit, for the plain forward and for the guided blend."""
    from gesturediffusion_amd.model.cfg_sampler import ClassifierFreeSampleModel
    from gesturediffusion_amd.utils.init import init_state_dict, synthetic_inputs
    cfg = _real_cfg(arch, 263, 512)
    m = build_model(arch, cfg, init_state_dict(cfg, seed=0))
    d = dev()
    x, seedp, mfcc = synthetic_inputs(cfg, B, T, seed=10)
    t = torch.full((B,), 77, device=d)
    lo = B - 3
    y = {"seed": seedp.to(d), "mfcc": mfcc.to(d)}
    y2 = {"seed": seedp[lo:lo + 2].to(d), "mfcc": mfcc[lo:lo + 2].to(d)}
    full = m(x.to(d), t, y)
    assert torch.isfinite(full).all()
    assert torch.equal(full[lo:lo + 2], m(x[lo:lo + 2].to(d), t[:2], y2))
    g = ClassifierFreeSampleModel(m)
    full_g = g(x.to(d), t, dict(y, scale=torch.full((B,), 2.5, device=d)))
    assert torch.isfinite(full_g).all()
    assert torch.equal(full_g[lo:lo + 2], g(x[lo:lo + 2].to(d), t[:2], dict(y2, scale=torch.full((2,), 2.5, device=d))))


def test_error_behaviour_matches_reference(golden_dir):
    import os
    from gesturediffusion_amd.utils.init import init_state_dict, synthetic_inputs
    want = dict(l.strip().split("=") for l in open(os.path.join(golden_dir, "negative_cases.txt")))
    cfg = dict(TINY, arch="mdm")
    m = build_model("mdm", cfg, init_state_dict(cfg, seed=1))
    d = dev()
    x, seedp, mfcc = synthetic_inputs(cfg, 2, 16, seed=3)
    t = torch.tensor([1, 2], device=d)
    with pytest.raises(Exception) as ei:
        m(x.to(d), t, {"seed": seedp.to(d), "mfcc": mfcc.to(d)})
    assert type(ei.value).__name__ == want["v2_T_not_multiple_of_10"]
    x, seedp, mfcc = synthetic_inputs(cfg, 2, 20, seed=3)
    with pytest.raises(KeyError):
        m(x.to(d), t, {"mfcc": mfcc.to(d)})
    with pytest.raises(KeyError):
        m(x.to(d), t, {"seed": seedp.to(d)})
    with pytest.raises(Exception):            # CPU tensors never fall back to a CPU path
        m(x, t.cpu(), {"seed": seedp, "mfcc": mfcc})
    assert m.eval() is m                      # superset of the reference (which returns None)


@pytest.mark.parametrize("extra", [["--arch_version", "mdm_old", "--num_frames", "23", "--guidance_param", "1"],
                                   ["--arch_version", "mdm", "--num_frames", "20", "--compute_dtype", "fp16"],
                                   ["--arch_version", "mdm_old", "--num_frames", "20", "--compute_dtype", "bf16", "--rng", "philox"],
                                   ["--arch_version", "mdm", "--num_frames", "20", "--synthetic_njoints", "48"],
                                   ["--arch_version", "mdm_old", "--num_frames", "31", "--synthetic_audio"],
                                   ["--arch_version", "mdm", "--num_frames", "20", "--rng", "philox"],
                                   ["--arch_version", "mdm", "--num_frames", "20", "--sampler", "ddim", "--timestep_respacing", "ddim10"]])
def test_generate_cli_synthetic(tmp_path, extra):
    """The sample.generate CLI end to end (args -> factory -> CFG wrapper -> chunked autoregressive sampling with
    seed chaining -> results.npy) on synthetic conditioning."""
    from gesturediffusion_amd.sample import generate
    out = tmp_path / "out"
    base = ["--synthetic", "--latent_dim", "128", "--layers", "2", "--num_samples", "3", "--chunks", "2",
            "--synthetic_njoints", "37", "--output_dir", str(out), "--seed", "7"]
    if "--timestep_respacing" not in extra:
        base += ["--timestep_respacing", "25"]
    assert generate.main(base + extra) == 0
    res = np.load(out / "results.npy", allow_pickle=True).item()      # written by this test a moment ago
    frames = int(extra[extra.index("--num_frames") + 1])
    if "--synthetic_njoints" in extra:          # 6 features per joint: de-normalised positions + rotations (gdx_postprocess)
        assert res["motion"].shape == (3, 8, 3, 2 * frames) and res["motion_rot"].shape == (3, 8, 3, 2 * frames)
        assert np.isfinite(res["motion_rot"]).all()
    else:
        assert res["motion"].shape == (3, 37, 1, 2 * frames)
    assert np.isfinite(res["motion"]).all() and np.abs(res["motion"]).max() > 0


# ---------------------------------------------------------------------------------------------------------------
# fp16 compute mode (BASELINE config 5's reduced-precision variant): fp16 MFMA operands, fp32 accumulate.
# Tolerance from SURVEY.md section 8d: <= 2e-2 of max|ref| against the reference's fp32 outputs (measured ~6e-4).
F16_TOL = 2e-2


@pytest.mark.parametrize("M,N,K,gelu", [(1000, 1024, 512, 0), (333, 320, 576, 0), (257, 1536, 512, 1), (64, 64, 64, 1),
                                        (4100, 512, 1024, 0), (16000, 3072, 128, 1)])   # the last one takes the 256x256 kernel
def test_fp16_gemm_vs_torch(M, N, K, gelu):
    """csrc/gemmh.hip through the C ABI: exact products of the fp16-rounded operands, fp32 accumulate -> the fp32
    output matches an fp64 reference on the same rounded operands to fp32 round-off; the fp16 output to fp16 round-off."""
    import ctypes as C
    from gesturediffusion_amd import _lib
    lib = _lib.load()
    d = dev()
    g = torch.Generator(device=d).manual_seed(M + N)
    A = torch.randn(M, K, device=d, generator=g)
    W = torch.randn(N, K, device=d, generator=g) / K ** 0.5
    b = torch.randn(N, device=d, generator=g)
    C32 = torch.full((M, N), float("nan"), device=d)
    C16 = torch.full((M, N), float("nan"), device=d)
    vp = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.gdx_linear_f16(vp(A), vp(W), vp(b), vp(C32), vp(C16), M, N, K, gelu, s), lib)
    ref = A.half().double() @ W.half().double().t() + b.double()
    if gelu:
        ref = torch.nn.functional.gelu(ref)
    dev_err = lambda c: float(((c.double() - ref).abs().max() / ref.abs().max()).item())   # noqa: E731
    assert dev_err(C32) < (3e-5 if gelu else 2e-6)    # GELU: polynomial erf, |err| <= 1.1e-5 |x|
    assert dev_err(C16) < 1e-3


@pytest.mark.parametrize("B,S,H,dm", [(2, 197, 4, 512), (1, 521, 4, 1024), (3, 250, 2, 128), (2, 31, 8, 512), (2, 1, 4, 512),
                                      (1, 300, 4, 256), (2, 77, 4, 128), (40, 197, 4, 512), (33, 100, 4, 1024), (20, 130, 8, 512),
                                      (130, 100, 4, 512), (64, 300, 8, 512), (44, 521, 4, 1024)])
def test_fp16_attention_vs_torch(B, S, H, dm):
    """csrc/attentionh.hip (head_dim 32/64/128/256, ragged sequence lengths, single token; shapes 8-10 have enough
    workgroups to take the 8-wave x 2-block kernel, the last three at least two work items per CU: the persistent form,
    head_dim 128 / 64 / 256, one / two / three query chunks per (sample, head)) against fp64 softmax attention on the
    fp16-rounded q/k/v."""
    import ctypes as C
    from gesturediffusion_amd import _lib
    lib = _lib.load()
    d = dev()
    hd = dm // H
    g = torch.Generator(device=d).manual_seed(S)
    qkv = torch.randn(B * S, 3 * dm, device=d, generator=g)
    qkv[:, :dm] *= 2.0
    ctx = torch.full((B * S, dm), float("nan"), device=d)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.gdx_attention_f16(C.c_void_p(qkv.data_ptr()), C.c_void_p(ctx.data_ptr()), B, S, H, dm, s), lib)
    r = qkv.half().double().view(B, S, 3, H, hd)
    q, k, v = (r[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    p = torch.softmax(q @ k.transpose(-1, -2) / hd ** 0.5, dim=-1)
    ref = (p @ v).permute(0, 2, 1, 3).reshape(B * S, dm)
    assert rel_err(ctx.cpu().double(), ref.cpu()) < 2e-3


@pytest.mark.parametrize("version", [1, 3, 5])
@pytest.mark.parametrize("B,S,H,dm", [(3, 197, 4, 512), (2, 201, 4, 512), (2, 61, 4, 512), (2, 65, 4, 512), (2, 129, 4, 512),
                                      (1, 256, 4, 512), (2, 241, 4, 512), (3, 1, 4, 512), (2, 16, 4, 512), (2, 197, 8, 512),
                                      (2, 81, 2, 128), (66, 197, 4, 512)])
def test_fp32_attention_vs_torch(B, S, H, dm, version):
    """The two fp32 SDPA kernels (csrc/attention.hip = version 1, the general fallback; attention3.hip = version 3; version 5 =
    attention3's persistent variant, every workgroup walking ~3 (sample, head) items) against fp64 softmax attention: the BASELINE sequence
    lengths (197, 201, 61), every 4k + 1 block count that makes attention3 share the last query block out over four
    waves (65, 129, 197), full 16 blocks, one token, head_dim 64 and 128, more workgroups than CUs."""
    import ctypes as C
    from gesturediffusion_amd import _lib
    lib = _lib.load()
    d = dev()
    hd = dm // H
    g = torch.Generator(device=d).manual_seed(S + min(version, 3))   # version 5 sees version 3's data
    qkv = torch.randn(B * S, 3 * dm, device=d, generator=g)
    qkv[:, :dm] *= 3.0                                   # peaked rows: exercises the deferred-max rescale
    ctx = torch.full((B * S, dm), float("nan"), device=d)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.gdx_attention_f32(C.c_void_p(qkv.data_ptr()), C.c_void_p(ctx.data_ptr()), B, S, H, dm, version, s), lib)
    r = qkv.double().view(B, S, 3, H, hd)
    q, k, v = (r[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    p = torch.softmax(q @ k.transpose(-1, -2) / hd ** 0.5, dim=-1)
    ref = (p @ v).permute(0, 2, 1, 3).reshape(B * S, dm)
    assert rel_err(ctx.cpu().double(), ref.cpu()) < 2e-6


@pytest.mark.parametrize("hd", [64, 128])
def test_fp32_attention3_every_block_count(hd):
    """attention3.hip at every query-block count 1..16 (sequence lengths 16 k - 15 and 16 k - 3): with / without the
    shared last block, 1..4 K/V tiles, waves with 0, 1 or 2 own blocks, masked tail of 1 and 13 keys."""
    import ctypes as C
    from gesturediffusion_amd import _lib
    lib = _lib.load()
    d = dev()
    H = 2
    dm = H * hd
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for k in range(1, 17):
        for S in (16 * k - 15, 16 * k - 3):
            B = 3
            g = torch.Generator(device=d).manual_seed(1000 * hd + S)
            qkv = torch.randn(B * S, 3 * dm, device=d, generator=g)
            qkv[:, :dm] *= 2.0
            r = qkv.double().view(B, S, 3, H, hd)
            q, kk, v = (r[:, :, i].permute(0, 2, 1, 3) for i in range(3))
            p = torch.softmax(q @ kk.transpose(-1, -2) / hd ** 0.5, dim=-1)
            ref = (p @ v).permute(0, 2, 1, 3).reshape(B * S, dm)
            outs = []
            for version in (3, 5):                        # item-resident / persistent (2 workgroups x 3 items)
                ctx = torch.full((B * S, dm), float("nan"), device=d)
                _lib.check(lib.gdx_attention_f32(C.c_void_p(qkv.data_ptr()), C.c_void_p(ctx.data_ptr()), B, S, H, dm, version, s), lib)
                assert rel_err(ctx.cpu().double(), ref.cpu()) < 2e-6, (hd, S, version)
                outs.append(ctx)
            assert torch.equal(outs[0], outs[1]), (hd, S)   # same arithmetic per item


@pytest.mark.parametrize("name,arch,J,dm", [("c1_v2", "mdm", 150, 512), ("c2_v1", "mdm_old", 263, 512),
                                            ("c5_v2", "mdm", 498, 1024)])
def test_fp16_mode_real_shapes_vs_reference_golden(name, arch, J, dm):
    """fp16 mode at BASELINE shapes (incl. config 5: d=1024, T=520) against the reference's own fp32 outputs."""
    from gesturediffusion_amd.utils.init import init_state_dict, synthetic_inputs
    g = load_golden("real_shapes.npz")
    B, T = int(g[name + ".meta"][0]), int(g[name + ".meta"][1])
    cfg = _real_cfg(arch, J, dm)
    m = build_model(arch, cfg, init_state_dict(cfg, seed=0))
    m.compute_dtype = "fp16"
    x, seedp, mfcc = synthetic_inputs(cfg, B, T, seed=10)
    d = dev()
    t = torch.from_numpy(g[name + ".t"]).to(d)
    y = {"seed": seedp.to(d), "mfcc": mfcc.to(d)}
    assert rel_err(m(x.to(d), t, y).cpu(), g[name + ".out"]) < F16_TOL
    assert rel_err(m(x.to(d), t, dict(y, uncond=True)).cpu(), g[name + ".out_uncond"]) < F16_TOL
    if name == "c1_v2":
        gen = torch.Generator().manual_seed(77)
        tape = torch.randn(11, B, J, 1, T, generator=gen).to(d)
        r = _diffusion("ddim10").ddim_sample_loop(m, (B, J, 1, T), noise_tape=tape, clip_denoised=False,
                                                   model_kwargs={"y": y})
        assert rel_err(r.cpu(), g["c1_v2.ddim10"]) < F16_TOL


@pytest.mark.parametrize("arch", ["mdm", "mdm_old"])
@pytest.mark.parametrize("name", ["p20", "p20_cfg", "ddim10_cfg", "p20_cfg_inpaint"])
def test_fp16_mode_loops_vs_reference_golden(arch, name):
    """fp16 mode through whole sampling loops (fused C++ loop) against the reference's fp32 loops, same noise tape."""
    _run_loop_case(arch, name, True, "fp16", F16_TOL)


# ---------------------------------------------------------------------------------------------------------------
# PLMS: reference gaussian_diffusion.py:995-1190
def _plms_oracle_step(tab, kind, x, x0, t, eps):
    from oracle import sampler as osamp
    ex = osamp.extract
    if kind == 0:
        return osamp.predict_eps(tab, x0, x, t)
    abp = ex(tab.alphas_cumprod_prev, t)
    if kind == 6:
        return x0 * torch.sqrt(abp) + torch.sqrt(1 - abp) * eps[0]
    ep = {1: lambda: eps[0], 2: lambda: (3 * eps[0] - eps[1]) / 2,
          3: lambda: (23 * eps[0] - 16 * eps[1] + 5 * eps[2]) / 12,
          4: lambda: (55 * eps[0] - 59 * eps[1] + 37 * eps[2] - 9 * eps[3]) / 24,
          5: lambda: (eps[0] + eps[1]) / 2}[kind]()
    pred = osamp.predict_xstart(tab, ep, x, t)
    mean = pred * torch.sqrt(abp) + torch.sqrt(1 - abp) * ep
    nz = (t != 0).float().view(-1, 1, 1, 1)
    return mean * nz + x0 * (1 - nz)


@pytest.mark.parametrize("kind", [0, 1, 2, 3, 4, 5, 6])
def test_plms_update_bit_exact(kind):
    """gdx_plms_update against the torch-CPU expression of the reference, same operands: identical bits."""
    from gesturediffusion_amd import engine as E
    from oracle import schedule as osch
    tab, _ = osch.make_tables("cosine", 1000, [10])
    df = _diffusion([10])
    d = dev()
    g = torch.Generator().manual_seed(kind)
    shape = (5, 7, 1, 13)
    x, x0 = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    eps = [torch.randn(shape, generator=g) for _ in range(4)]
    t = torch.tensor([0, 1, 5, 9, 0])
    want = _plms_oracle_step(tab, kind, x, x0, t, eps)
    coef = df.coef_table(1, d, 0.0)
    got = E.plms_update(kind, coef, t.to(d), x.to(d), x0.to(d), eps=[e.to(d) for e in eps])
    assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize("arch", ["mdm", "mdm_old"])
@pytest.mark.parametrize("name,order", [("plms10_o2", 2), ("plms10_o3", 3), ("plms10_o4_cfg", 4), ("plms10_o2_inpaint", 2),
                                        ("plms10_o2_init_skip", 2)])
def test_plms_loops_vs_reference_golden(arch, name, order):
    from gesturediffusion_amd.model.cfg_sampler import ClassifierFreeSampleModel
    g = load_golden(f"loops_{arch}_tiny.npz")
    gp = load_golden(f"plms_{arch}_tiny.npz")
    d = dev()
    m = build_model(arch, TINY, weights_from(g))
    y = {"seed": torch.from_numpy(g["seed"]).to(d), "mfcc": torch.from_numpy(g["mfcc"]).to(d)}
    model, kw = m, {}
    if "cfg" in name:
        y["scale"] = torch.from_numpy(g["scale"]).to(d)
        model = ClassifierFreeSampleModel(m)
    if "inpaint" in name:
        y["inpainting_mask"] = torch.from_numpy(g["inpainting_mask"]).to(d)
        y["inpainted_motion"] = torch.from_numpy(g["inpainted_motion"]).to(d)
    if "init" in name:
        kw.update(init_image=torch.from_numpy(g["init_image"]).to(d), skip_timesteps=3)
    x_T = torch.from_numpy(g["tape"])[0].to(d)
    df = _diffusion([10])
    r = df.plms_sample_loop(model, tuple(x_T.shape), noise=x_T.clone(), clip_denoised=False, model_kwargs={"y": y},
                            order=order, **kw)
    # the multistep weights amplify fp32 forward differences (oracle vs reference measures 1.1e-4 at order 4 + CFG)
    assert rel_err(r.cpu(), gp[name]) < (2e-3 if order == 4 else LOOP_TOL), name
    with pytest.raises(TypeError):      # order 1 subscripts old_out = None on the first step, like the reference
        df.plms_sample_loop(model, tuple(x_T.shape), noise=x_T.clone(), clip_denoised=False, model_kwargs={"y": y}, order=1)
    with pytest.raises(ValueError):
        df.plms_sample_loop(model, tuple(x_T.shape), noise=x_T.clone(), clip_denoised=False, model_kwargs={"y": y}, order=5)


def test_fp16_mode_switch_and_reshape_on_one_model():
    """The compute mode is a property of the engine, not of the weights: one model object switches fp32 -> fp16 -> fp32
    (engine re-created, weights re-packed) and is re-prepared for another (B, T) in between; the fp32 results before and
    after are identical, the fp16 ones within the fp16 tolerance of them."""
    from gesturediffusion_amd.utils.init import init_state_dict, synthetic_inputs
    cfg = dict(arch="mdm_old", njoints=53, nfeats=1, latent_dim=256, ff_size=512, num_layers=2, num_heads=4, seed_poses=10)
    m = build_model("mdm_old", cfg, init_state_dict(cfg, seed=3, perturb=True))
    d = dev()

    def run(B, T):
        x, seedp, mfcc = synthetic_inputs(cfg, B, T, seed=B + T)
        t = (torch.arange(B) * 37 + 5) % 1000
        return m(x.to(d), t.to(d), {"seed": seedp.to(d), "mfcc": mfcc.to(d)})
    a32 = run(3, 50)
    m.compute_dtype = "fp16"
    a16 = run(3, 50)
    b16 = run(5, 33)
    m.compute_dtype = "fp32"
    b32 = run(5, 33)
    again = run(3, 50)
    assert torch.equal(a32, again)
    assert rel_err(a16.cpu(), a32.cpu()) < F16_TOL and rel_err(b16.cpu(), b32.cpu()) < F16_TOL
    assert not torch.equal(a16, a32)
    with pytest.raises(ValueError):
        m.compute_dtype = "int8"
        run(3, 50)


def test_postprocess_chunk_bit_exact():
    """gdx_postprocess (inv_transform + position / rotation split, reference sample/generate.py:132-146) against the
    CPU restatement: identical bits (fp64 statistics, one rounding)."""
    from gesturediffusion_amd import engine as E
    from oracle import sampler as osamp
    g = torch.Generator().manual_seed(4)
    B, nj, T = 3, 83, 120                                   # GENEA: 83 joints x 6 = 498 features, 120-frame chunks
    x = torch.randn(B, nj * 6, 1, T, generator=g)
    rng = np.random.default_rng(0)
    mean, std = rng.normal(size=nj * 6), rng.uniform(0.1, 3.0, size=nj * 6)
    pos, rot = E.postprocess(x.to(dev()), mean, std)
    wp, wr = osamp.postprocess_chunk(x, mean, std)
    assert pos.shape == (B, nj, 3, T) and torch.equal(pos.cpu(), wp.contiguous()) and torch.equal(rot.cpu(), wr.contiguous())


@pytest.mark.parametrize("arch", ["mdm", "mdm_old"])
@pytest.mark.parametrize("tag,resp", [("full", [1000]), ("r20", [20])])
def test_training_losses_forward_half_vs_reference_golden(arch, tag, resp):
    """training_losses' forward values (reference gaussian_diffusion.py:1227-1352): q_sample with per-sample
    timesteps, native forward, masked MSE over a ragged frame mask -- against the values the reference computed."""
    g = load_golden(f"loops_{arch}_tiny.npz")
    gl = load_golden(f"losses_{arch}_tiny.npz")
    d = dev()
    m = build_model(arch, TINY, weights_from(g))
    y = {"seed": torch.from_numpy(g["seed"]).to(d), "mfcc": torch.from_numpy(g["mfcc"]).to(d),
         "mask": torch.from_numpy(gl["mask"]).to(d)}
    df = _diffusion(resp)
    terms = df.training_losses(m, torch.from_numpy(gl["x_start"]).to(d), torch.from_numpy(gl[tag + ".t"]).to(d),
                               model_kwargs={"y": y}, noise=torch.from_numpy(gl["noise"]).to(d))
    assert rel_err(terms["rot_mse"].cpu(), gl[tag + ".rot_mse"]) < 2e-5
    assert rel_err(terms["loss"].cpu(), gl[tag + ".loss"]) < 2e-5
    with pytest.raises(KeyError):
        df.training_losses(m, torch.from_numpy(gl["x_start"]).to(d), torch.from_numpy(gl[tag + ".t"]).to(d),
                           model_kwargs={"y": {k: v for k, v in y.items() if k != "mask"}})


@pytest.mark.parametrize("arch", ["mdm", "mdm_old"])
@pytest.mark.parametrize("name", ["p20_cfg_inpaint", "ddim10_eta05", "p20_const_noise"])
def test_graph_replay_matches_eager_loop(arch, name):
    """gdx_set_graph_replay: one captured step replayed as a hipGraph (device-resident step state) gives bit-identical
    results to the eager loop and matches the reference fixture (noise tape, CFG, inpainting, const_noise, DDIM eta);
    a Philox loop is compared graph vs eager as well."""
    from gesturediffusion_amd.model.cfg_sampler import ClassifierFreeSampleModel
    g = load_golden(f"loops_{arch}_tiny.npz")
    d = dev()
    m = build_model(arch, TINY, weights_from(g))
    tape = torch.from_numpy(g["tape"]).to(d)
    y = {"seed": torch.from_numpy(g["seed"]).to(d), "mfcc": torch.from_numpy(g["mfcc"]).to(d)}
    model = m
    if "cfg" in name:
        y["scale"] = torch.from_numpy(g["scale"]).to(d)
        model = ClassifierFreeSampleModel(m)
    if "inpaint" in name:
        y["inpainting_mask"] = torch.from_numpy(g["inpainting_mask"]).to(d)
        y["inpainted_motion"] = torch.from_numpy(g["inpainted_motion"]).to(d)
    kw = dict(clip_denoised=False, model_kwargs={"y": y})
    if name.startswith("p20"):
        df, fn = _diffusion([20]), "p_sample_loop"
    else:
        df, fn = _diffusion("ddim10"), "ddim_sample_loop"
    if name == "p20_const_noise":
        kw["const_noise"] = True
    if name == "ddim10_eta05":
        kw["eta"] = 0.5
    shape = tuple(tape[0].shape)
    eng = m._get_engine(d)
    eager = getattr(df, fn)(model, shape, noise_tape=tape, **kw)
    eager_px = getattr(df, fn)(model, shape, rng="philox", philox_seed=5, **kw)
    eng.set_graph_replay(True)
    try:
        replay = getattr(df, fn)(model, shape, noise_tape=tape, **kw)
        replay_px = getattr(df, fn)(model, shape, rng="philox", philox_seed=5, **kw)
    finally:
        eng.set_graph_replay(False)
    assert torch.equal(replay, eager) and torch.equal(replay_px, eager_px)
    assert rel_err(replay.cpu(), g[name]) < LOOP_TOL


def test_fp16_mode_taps_match_fp32_taps():
    """Parity taps in the fp16 mode (fp32 copies written by the fp16 GEMM / LayerNorm epilogues only when taps are kept):
    every encoder-layer activation stays within the fp16 tolerance of the fp32 path's."""
    from gesturediffusion_amd.utils.init import init_state_dict, synthetic_inputs
    cfg = dict(arch="mdm", njoints=48, nfeats=1, latent_dim=512, ff_size=1024, num_layers=3, num_heads=4, seed_poses=10)
    sd = init_state_dict(cfg, seed=1, perturb=True)
    d = dev()
    x, seedp, mfcc = synthetic_inputs(cfg, 2, 30, seed=2)
    t = torch.tensor([17, 803], device=d)
    y = {"seed": seedp.to(d), "mfcc": mfcc.to(d)}
    taps = {}
    for dt in ("fp32", "fp16"):
        m = build_model("mdm", cfg, sd)
        m.compute_dtype = dt
        eng = m._get_engine(d)
        eng.keep_taps(True)
        m(x.to(d), t, y)
        taps[dt] = [eng.tap(i, 2 * 2 * 31, 512, d)[: 2 * 31].cpu() for i in range(cfg["num_layers"] + 1)]
    for a, b in zip(taps["fp32"], taps["fp16"]):
        assert rel_err(b, a) < F16_TOL and not torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------
# cond_fn guidance: condition_mean / condition_score, reference gaussian_diffusion.py:418-494
def _cond_fn_fixture(x, t, **kwargs):
    return 0.05 * torch.sin(x) * (1.0 + t.view(-1, 1, 1, 1).float() / 1000.0)


@pytest.mark.parametrize("kind,eta", [("p", 0.0), ("ddim", 0.0), ("ddim", 0.5)])
def test_guided_update_bit_exact(kind, eta):
    """The fused update with a cond_fn gradient against the torch-CPU expression of the reference: identical bits."""
    from gesturediffusion_amd import engine as E
    from oracle import sampler as osamp
    from oracle import schedule as osch
    tab, _ = osch.make_tables("cosine", 1000, [10])
    df = _diffusion([10])
    d = dev()
    g = torch.Generator().manual_seed(11)
    shape = (5, 7, 1, 13)
    x, x0, z, gr = (torch.randn(shape, generator=g) for _ in range(4))
    t = torch.tensor([0, 1, 5, 9, 0])
    if kind == "p":
        want = osamp.p_sample_step_cond(tab, x0, x, t, z, gr)
    else:
        want = osamp.ddim_step_cond(tab, x0, x, t, z, gr, eta)
    code = 0 if kind == "p" else 1
    out = torch.empty(shape, device=d)
    E.sampler_update(code, df.coef_table(code, d, eta), x.to(d), x0.to(d), out, t=t.to(d), noise=z.to(d),
                     cond_grad=gr.to(d), cond_coef=df._cond_coef(d) if kind == "ddim" else None)
    assert torch.equal(out.cpu(), want)


@pytest.mark.parametrize("arch", ["mdm", "mdm_old"])
@pytest.mark.parametrize("name,fn,resp,eta", [("p20_guided", "p_sample_loop", [20], None), ("ddim10_guided", "ddim_sample_loop", "ddim10", 0.0),
                                              ("ddim10_eta05_guided", "ddim_sample_loop", "ddim10", 0.5)])
def test_guided_loops_vs_reference_golden(arch, name, fn, resp, eta):
    """Loops with cond_fn against the reference's (same noise tape): the user's gradient callable runs in torch on the
    device, its application to the mean / eps inside the fused update kernel."""
    g = load_golden(f"loops_{arch}_tiny.npz")
    gg = load_golden(f"guided_{arch}_tiny.npz")
    d = dev()
    m = build_model(arch, TINY, weights_from(g))
    tape = torch.from_numpy(g["tape"]).to(d)
    y = {"seed": torch.from_numpy(g["seed"]).to(d), "mfcc": torch.from_numpy(g["mfcc"]).to(d)}
    kw = dict(clip_denoised=False, model_kwargs={"y": y}, cond_fn=_cond_fn_fixture, noise_tape=tape)
    if eta is not None:
        kw["eta"] = eta
    r = getattr(_diffusion(resp), fn)(m, tuple(tape[0].shape), **kw)
    assert rel_err(r.cpu(), gg[name]) < LOOP_TOL, name


@pytest.mark.parametrize("arch", ["mdm", "mdm_old"])
def test_plms_guided_loop_vs_reference_golden(arch):
    """plms_sample_loop with cond_fn (condition_score inside get_model_output, reference :1015-1041)."""
    g = load_golden(f"loops_{arch}_tiny.npz")
    gg = load_golden(f"guided_{arch}_tiny.npz")
    d = dev()
    m = build_model(arch, TINY, weights_from(g))
    y = {"seed": torch.from_numpy(g["seed"]).to(d), "mfcc": torch.from_numpy(g["mfcc"]).to(d)}
    x_T = torch.from_numpy(g["tape"])[0].to(d)
    r = _diffusion([10]).plms_sample_loop(m, tuple(x_T.shape), noise=x_T.clone(), clip_denoised=False,
                                          model_kwargs={"y": y}, cond_fn=_cond_fn_fixture)
    assert rel_err(r.cpu(), gg["plms10_o2_guided"]) < LOOP_TOL


@pytest.mark.parametrize("n", [88200, 44100 + 17, 1000])
def test_mfcc_front_end_vs_restated_package(n):
    """gdx_mfcc against oracle/mfcc.py.  PARITY UNPINNED with respect to the reference: the oracle restates
    python_speech_features 0.6 (absent from this image, no fixtures in the reference); 120-frame chunk, a ragged chunk
    and a chunk shorter than one frame."""
    from gesturediffusion_amd.data_loaders.mfcc import MfccExtractor
    from oracle import mfcc as om
    rng = np.random.default_rng(n)
    t = np.arange(n) / 22050.0
    sig = (0.3 * np.sin(2 * np.pi * 220 * t) + 0.1 * np.sin(2 * np.pi * 1870 * t) + 0.05 * rng.normal(size=n)).astype(np.float32)
    mean, std = rng.normal(size=26), rng.uniform(0.5, 3.0, size=26)
    want = om.genea_mfcc(sig.astype(np.float64), 22050, 30, mean, std)
    ex = MfccExtractor(dev(), mfcc_mean=mean, mfcc_std=std)
    got = ex(torch.from_numpy(sig).to(dev()))
    assert tuple(got.shape) == want.shape == (ex.num_frames(n), 26)
    assert rel_err(got.cpu(), want) < 2e-4
