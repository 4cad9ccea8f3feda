"""DDIM inversion on the GPU (gdx_ddim_reverse_step, gdx_ddim_reverse_loop, ddim_reverse_sample{,_loop}, ddim_sample_loop's
init_is_state, sample.generate --invert_gt; include/gdx.h): the fused step against its op order bit for bit, the in-library loop
against the reference's golden, the step-wise protocol and the block-wise issue, inversion + re-generation against the CPU
restatement (ddim_reverse_restatement.py), and the CLI.  Need an MI355X."""
import os

import numpy as np
import pytest
import torch

import ddim_reverse_restatement as R
from conftest import rel_err
from misaligned import shifted
from oracle import schedule as osch
from test_ddim_reverse_host import ARCHS, ROUND_TRIP_TOL, tiny_case
from test_gpu_dpm import B, _tiny
from test_gpu_parity import LOOP_TOL, _diffusion, dev

pytestmark = pytest.mark.gpu
CANARY = 64                      # floats behind every output
SENTINEL = 12345.0


# ---------------------------------------------------------------------------------------------------------------- kernel
def _out(shape, d, shift=False):
    """An output tensor of `shape` (one float off 16-byte alignment if shift) with CANARY sentinel floats right behind it."""
    n = int(np.prod(shape))
    buf = torch.full((n + CANARY + 1,), SENTINEL, device=d)
    v = buf[1:] if shift else buf[:-1]
    assert v.data_ptr() % 16 == (4 if shift else 0)
    return v[:n].view(shape), v[n:n + CANARY]


def _intact(canary):
    return bool((canary == SENTINEL).all())


@pytest.mark.parametrize("variant", ["plain", "cfg", "mask", "clamp"])
@pytest.mark.parametrize("shape", [(3, 5, 7), (2, 1, 4), (2, 257, 4), (1, 13, 79)])
def test_step_kernel_bit_exact(shape, variant):
    """gdx_ddim_reverse_step == its op order in torch fp32 on the CPU (IEEE division) by torch.equal on out, pred_out and eps_out.
    J*T = 35: scalar path; 4: one vector group; 1028 = 257 groups: the second block has one live thread; 1027: scalar with a
    3-element tail.  Per-sample t (rows 0, 4 and the last, whose abar_next is 0) and step_index; out aliasing x; every operand in
    turn one float (the mask: one byte) off alignment, which takes the scalar path with the same bits; 64 sentinel floats behind each
    output stay untouched; leaving eps_out / pred_out out changes no bit of out.  CFG: every sample meets the scales 2.5, 1.0 and 0."""
    from gesturediffusion_amd import engine as E
    from gesturediffusion_amd._lib import GDX_SAMPLER_DDIM
    d = dev()
    Bn, J, T = shape
    full = (Bn, J, 1, T)
    coef = _diffusion("ddim10").coef_table(GDX_SAMPLER_DDIM, d, "reverse")
    g = torch.Generator().manual_seed(J * T + len(variant))
    rnd = lambda s=1.0: torch.randn(full, generator=g) * s   # noqa: E731
    x, oc, ou, motion = rnd(), rnd(1.5), rnd(1.5), rnd(0.5)
    mask = torch.rand(full, generator=g) < 0.3
    t_rows = torch.tensor([0, 4, 9])[:Bn]
    scales = [torch.tensor(s)[:Bn] for s in ([2.5, 1.0, 0.0], [1.0, 0.0, 2.5], [0.0, 2.5, 1.0])] if variant == "cfg" else [None]
    launches = 0
    for scale in scales:
        host = dict(ou=ou if variant == "cfg" else None, scale=scale, mask=mask if variant == "mask" else None,
                    motion=motion if variant == "mask" else None)
        clip = variant == "clamp"
        ops = {"x": x.to(d), "x0_cond": oc.to(d)}
        if variant == "cfg":
            ops.update(x0_uncond=ou.to(d), scale=scale.to(d))
        if variant == "mask":
            ops.update(inpaint_mask=mask.to(d), inpaint_motion=motion.to(d))

        def run(t_mode, alias=False, off=None, want_pred=True, want_eps=True):
            """One launch -> (out, pred, eps) on the host; `off`: the operand moved off alignment."""
            nonlocal launches
            kw = {k: (shifted(v) if k == off else v) for k, v in ops.items()}
            xin = kw.pop("x").clone()
            if off == "x":
                xin = shifted(xin)
            outs = {k: _out(full, d, off == k) for k in ("out", "pred_out", "eps_out")}
            out = xin if alias else outs["out"][0]
            E.ddim_reverse_step(coef, xin, kw.pop("x0_cond"), out, pred_out=outs["pred_out"][0] if want_pred else None,
                                eps_out=outs["eps_out"][0] if want_eps else None, clip_denoised=clip,
                                **(dict(t=t_rows.to(d)) if t_mode == "t" else dict(step_index=t_mode)), **kw)
            launches += 1
            assert all(_intact(c) for _, c in outs.values()), (t_mode, alias, off)
            if not want_pred:
                assert _intact(outs["pred_out"][0])
            if not want_eps:
                assert _intact(outs["eps_out"][0])
            return out.cpu(), outs["pred_out"][0].cpu(), outs["eps_out"][0].cpu()

        for t_mode in ("t", 5):
            idx = t_rows if t_mode == "t" else torch.full((Bn,), t_mode)
            want = R.step(coef.cpu()[idx], x, oc, host["ou"], scale, host["mask"], host["motion"], clip)
            assert all(torch.isfinite(w).all() for w in want)
            base = None
            for alias in (False, True):
                got = run(t_mode, alias)
                base = base or got
                for name, a, b in zip(("out", "pred", "eps"), got, want):
                    assert torch.equal(a, b), (name, shape, variant, t_mode, alias)
            for off in list(ops) + ["out", "pred_out", "eps_out"]:
                if off == "scale":
                    continue                                        # read per sample, never by group
                got = run(t_mode, off=off)
                for name, a, b in zip(("out", "pred", "eps"), got, want):
                    assert torch.equal(a, b), (name, shape, variant, t_mode, off)
            for want_pred, want_eps in ((False, True), (True, False), (False, False)):
                got = run(t_mode, want_pred=want_pred, want_eps=want_eps)
                assert torch.equal(got[0].view(torch.int32), base[0].view(torch.int32)), (shape, variant, t_mode, want_pred, want_eps)
    assert launches >= 2 * (2 + 5 + 3) * len(scales)


def test_step_kernel_has_the_bits_of_the_update_kernel_with_zero_noise():
    """What ddim_reverse_sample ran before: gdx_sampler_update with the reverse rows and a zero noise tensor.  Equal by torch.equal
    (which takes +0 and -0 for equal: the old path adds 0*0 last)."""
    from gesturediffusion_amd import engine as E
    from gesturediffusion_amd._lib import GDX_SAMPLER_DDIM
    d = dev()
    coef = _diffusion("ddim10").coef_table(GDX_SAMPLER_DDIM, d, "reverse")
    g = torch.Generator().manual_seed(11)
    x, oc = (torch.randn(3, 16, 1, 20, generator=g).to(d) for _ in range(2))
    t = torch.tensor([0, 3, 9], device=d)
    old, old_pred, new, new_pred = (torch.empty_like(x) for _ in range(4))
    E.sampler_update(GDX_SAMPLER_DDIM, coef, x, oc, old, t=t, noise=torch.zeros_like(x), pred_xstart=old_pred, clip_denoised=True)
    E.ddim_reverse_step(coef, x, oc, new, t=t, pred_out=new_pred, clip_denoised=True)
    assert torch.equal(new, old) and torch.equal(new_pred, old_pred)


# ------------------------------------------------------------------------------------------------------------------ loop
@pytest.mark.parametrize("arch", ARCHS)
def test_fused_loop_vs_reference_golden(arch):
    """ddim_reverse_sample_loop(until=3) from tape[0] on ddim10 against the reference's own three steps (ddim10_reverse3) at
    LOOP_TOL, fused and step by step."""
    g, m = _tiny(arch)
    d = dev()
    y = {"seed": torch.from_numpy(g["seed"]).to(d), "mfcc": torch.from_numpy(g["mfcc"]).to(d)}
    df = _diffusion("ddim10")
    x = torch.from_numpy(g["tape"])[0].to(d)
    for fused in (True, False):
        got = df.ddim_reverse_sample_loop(m, x, clip_denoised=False, model_kwargs={"y": y}, until=3, fused=fused)
        err = rel_err(got.cpu(), g["ddim10_reverse3"])
        print(f"{arch} fused={fused}: rel err vs ddim10_reverse3 {err:.3e}")
        assert err < LOOP_TOL
    assert torch.equal(x.cpu(), torch.from_numpy(g["tape"])[0])            # the caller's x_start is not written


VARIANTS = ["plain", "cfg", "inpaint", "clip", "interval", "rescale", "fp16"]
MID = (300, 700)                 # model timesteps of ddim10 are 0, 100, ..., 900: guidance on indices 3..7


def _case(name, arch):
    """(model, y, clip_denoised, x_start, inner model) of a variant on the first B samples of a tiny fixture."""
    from gesturediffusion_amd.model.cfg_sampler import ClassifierFreeSampleModel
    g, m = _tiny(arch, "fp16" if name == "fp16" else "fp32")
    d = dev()
    Tn = lambda k: torch.from_numpy(g[k])[:B].contiguous().to(d)   # noqa: E731
    y, model = {"seed": Tn("seed"), "mfcc": Tn("mfcc")}, m
    if name in ("cfg", "interval", "rescale", "fp16"):
        y["scale"] = torch.full((B,), 2.5, device=d)
        model = ClassifierFreeSampleModel(m)
    if name == "inpaint":
        y["inpainting_mask"], y["inpainted_motion"] = Tn("inpainting_mask"), Tn("inpainted_motion")
    if name == "interval":
        y["guidance_interval"] = MID
    if name == "rescale":
        y["guidance_rescale"] = 0.7
    return model, y, name == "clip", Tn("init_image"), m


@pytest.mark.parametrize("arch", ARCHS)
@pytest.mark.parametrize("name", VARIANTS)
def test_fused_loop_equals_stepwise_bit_for_bit(arch, name):
    """ddim_reverse_sample_loop(fused=True) == fused=False by torch.equal for until = 1, 9 and 10 (the last step goes to
    abar_next = 0), and the fused route pushes B samples through the denoiser on an unguided step and 2B on a guided one."""
    from gesturediffusion_amd.model.cfg_sampler import ClassifierFreeSampleModel
    model, y, clip, x0, inner = _case(name, arch)
    df = _diffusion("ddim10")
    flags = df.guided_steps(y.get("guidance_interval"))
    if name == "interval":
        assert flags == [False] * 3 + [True] * 5 + [False] * 2
    guided = isinstance(model, ClassifierFreeSampleModel)
    eng = inner._get_engine(dev())
    state = {}
    for until in (1, 9, 10):
        before = eng.forward_samples()
        fused = df.ddim_reverse_sample_loop(model, x0, clip_denoised=clip, model_kwargs={"y": y}, until=until)
        assert eng.forward_samples() - before == sum(2 * B if guided and flags[i] else B for i in range(until)), (name, until)
        step = df.ddim_reverse_sample_loop(model, x0, clip_denoised=clip, model_kwargs={"y": y}, until=until, fused=False)
        assert torch.isfinite(fused).all() and torch.equal(fused, step), (name, until)
        assert not any(torch.equal(fused, s) for s in state.values())     # each `until` is another state
        state[until] = fused
    chain = [o["sample"] for o in df.ddim_reverse_sample_loop_progressive(model, x0, clip_denoised=clip, model_kwargs={"y": y},
                                                                          until=9)]
    assert len(chain) == 9 and torch.equal(chain[0], state[1]) and torch.equal(chain[-1], state[9])
    assert torch.equal(df.ddim_reverse_sample_loop(model, x0, clip_denoised=clip, model_kwargs={"y": y}), state[9])   # the default until


@pytest.mark.parametrize("arch", ARCHS)
@pytest.mark.parametrize("name", ["plain", "interval"])
def test_blocks_of_3_4_2_equal_one_call_of_9(arch, name):
    """engine.ddim_reverse_loop issued as first_index / run_steps = 0/3, 3/4, 7/2 == one call 0/9: nothing but x is carried."""
    from gesturediffusion_amd._lib import GDX_SAMPLER_DDIM
    model, y, clip, x0, _ = _case(name, arch)
    df = _diffusion("ddim10")
    whole = df.ddim_reverse_sample_loop(model, x0, clip_denoised=clip, model_kwargs={"y": y}, until=9)
    x, eng, mode, scale, mask, motion = df._fused_setup(model, x0, {"y": y})
    coef, tmap = df.coef_table(GDX_SAMPLER_DDIM, x.device, "reverse"), df._timestep_map()
    for first, run in ((0, 3), (3, 4), (7, 2)):
        eng.ddim_reverse_loop(x, mode, coef, tmap, first, run, scale=scale, inpaint_mask=mask, inpaint_motion=motion, clip_denoised=clip)
    assert torch.equal(x, whole)


def test_library_refuses_the_guidance_refresh_and_python_refuses_first():
    from gesturediffusion_amd._lib import GDX_SAMPLER_DDIM, GdxError
    model, y, clip, x0, inner = _case("cfg", "mdm")
    df = _diffusion("ddim10")
    with pytest.raises(ValueError, match="guidance_refresh"):
        df.ddim_reverse_sample_loop(model, x0, clip_denoised=clip, model_kwargs={"y": dict(y, guidance_refresh=2)})
    x, eng, mode, scale, mask, motion = df._fused_setup(model, x0, {"y": y})
    eng.set_guidance_refresh(2)
    try:
        with pytest.raises(GdxError, match="guidance refresh"):
            eng.ddim_reverse_loop(x, mode, df.coef_table(GDX_SAMPLER_DDIM, x.device, "reverse"), df._timestep_map(), 0, 3, scale=scale)
    finally:
        eng.set_guidance_refresh(1)
    assert torch.equal(x, x0)                                              # refused before anything ran


# ------------------------------------------------------------------------------------------------- inversion + re-generation
@pytest.mark.parametrize("arch", ARCHS)
def test_inversion_and_regeneration_vs_cpu_restatement(arch):
    """Full inversion (until = 9) of tape[0] on ddim10 and ddim_sample_loop(noise=latent, eta=0) on it, clip_denoised=False (the
    un-clamped state stays finite on these weights: max|latent| ~6e2), against the restatement on the CPU.  Bounds (derivation and
    the measured spread: test_ddim_reverse_host.py): the restatement's own fp32-vs-float64 spread measured 3.86e-7 on the latent
    and 2.16e-4 on the re-generated sample; the GPU is allowed four times that, never less than LOOP_TOL: 2e-4 and 8.64e-4."""
    p, cfg, y, x, g = tiny_case(arch)
    tab, tmap = osch.make_tables("cosine", 1000, "ddim10")
    want_latent, want_sample = R.round_trip(p, cfg, tab, tmap, x, y, 9)
    _, m = _tiny(arch)
    d = dev()
    yd = {k: v.to(d) for k, v in y.items()}
    df = _diffusion("ddim10")
    latent = df.ddim_reverse_sample_loop(m, x.to(d), clip_denoised=False, model_kwargs={"y": yd}, until=9)
    sample = df.ddim_sample_loop(m, tuple(x.shape), noise=latent, eta=0.0, clip_denoised=False, model_kwargs={"y": yd})
    errs = {"latent": rel_err(latent.cpu(), want_latent), "sample": rel_err(sample.cpu(), want_sample)}
    print(f"{arch}: latent rel err {errs['latent']:.3e} (bound {ROUND_TRIP_TOL['latent']:.3e}), sample rel err "
          f"{errs['sample']:.3e} (bound {ROUND_TRIP_TOL['sample']:.3e}), max|latent| {float(latent.abs().max()):.1f}")
    assert torch.isfinite(latent).all() and torch.isfinite(sample).all()
    assert errs["latent"] <= ROUND_TRIP_TOL["latent"] and errs["sample"] <= ROUND_TRIP_TOL["sample"], errs


@pytest.mark.parametrize("arch", ARCHS)
@pytest.mark.parametrize("name", ["plain", "cfg"])
def test_init_is_state_round_trip(arch, name):
    """Invert to until = 5, re-generate with skip_timesteps = 4 and init_is_state=True: the loop starts at index 10 - 1 - 4 = 5 on
    the latent as it is, so the sample equals (torch.equal) a step-wise ddim_sample chain over the indices 5 .. 0 from that latent,
    fused or not.  Without the flag the latent is scaled by q_sample's sqrt(1 - abar) and the result differs."""
    model, y, clip, x0, _ = _case(name, arch)
    df = _diffusion("ddim10")
    kw = dict(clip_denoised=clip, model_kwargs={"y": y})
    latent = df.ddim_reverse_sample_loop(model, x0, until=5, **kw)
    keep = latent.clone()
    x = latent
    for i in range(5, -1, -1):
        x = df.ddim_sample(model, x, torch.full((B,), i, device=x.device, dtype=torch.long), **kw)["sample"]
    shape = tuple(latent.shape)
    for fused in (True, False):
        got = df.ddim_sample_loop(model, shape, noise=latent, skip_timesteps=4, init_is_state=True, fused=fused, **kw)
        assert torch.isfinite(got).all() and torch.equal(got, x), fused
    assert not torch.equal(df.ddim_sample_loop(model, shape, noise=latent, skip_timesteps=4, **kw), x)
    assert torch.equal(latent, keep)
    # skip_timesteps = 0 starts from `noise` as it is with or without the flag
    assert torch.equal(df.ddim_sample_loop(model, shape, noise=latent, init_is_state=True, **kw),
                       df.ddim_sample_loop(model, shape, noise=latent, **kw))


# --------------------------------------------------------------------------------------------------------------------- CLI
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    from genea_tree import build_tree
    from test_gpu_genea_data import FRAMES_VAL, J
    return build_tree(str(tmp_path_factory.mktemp("genea498inv")), J=J, frames_trn=[64], frames_val=FRAMES_VAL, seed=498, zero_std_at=7)


RESULT_KEYS = {"motion", "motion_rot", "num_samples", "num_chunks", "gt_motion", "gt_motion_rot", "audio", "text", "lengths", "takes"}


def _argv(tree, out, scale):
    from test_gpu_genea_data import argv_for
    argv = argv_for(tree, out, "mdm", "fp32")
    argv[argv.index("--guidance_param") + 1] = str(scale)
    return argv + ["--invert_gt"]


def test_generate_cli_invert_gt_equals_direct_calls(tree, tmp_path):
    """`sample.generate --dataset genea2023 --data_dir <tree> --sampler ddim --invert_gt` under guidance 2.5: every chunk of
    results.npy is ddim_reverse_sample_loop on the collated ground truth with the inner model (the conditional pass alone) followed
    by the guided ddim_sample_loop from that latent; results.npy keeps its keys."""
    from gesturediffusion_amd import engine as E
    from gesturediffusion_amd.data_loaders.mfcc import MfccExtractor
    from gesturediffusion_amd.data_loaders.tensors import gg_collate
    from gesturediffusion_amd.model.cfg_sampler import ClassifierFreeSampleModel
    from gesturediffusion_amd.sample import generate
    from gesturediffusion_amd.utils.init import MFCC_DIM, init_state_dict
    from gesturediffusion_amd.utils.model_util import create_model_and_diffusion
    from gesturediffusion_amd.utils.parser_util import generate_args
    from test_gpu_genea_data import CHUNKS, ITEMS, J, P, SCALE, SEED, T, TAKES, open_val
    out = str(tmp_path / "out")
    argv = _argv(tree, out, SCALE)
    assert generate.main(argv) == 0
    res = np.load(os.path.join(out, "results.npy"), allow_pickle=True).item()      # written a moment ago
    assert set(res) == RESULT_KEYS and res["motion"].shape == (TAKES, J // 6, 3, CHUNKS * T)
    d = dev()
    ds = open_val(tree)
    ex = MfccExtractor(d, sr=ds.sr, fps=ds.fps, mfcc_mean=ds.mfcc_mean, mfcc_std=ds.mfcc_std)
    args = generate_args(argv)
    args.mfcc_input = True
    inner, df = create_model_and_diffusion(args, None)
    cfg = dict(arch="mdm", njoints=J, nfeats=1, latent_dim=128, ff_size=1024, num_layers=2, num_heads=4, seed_poses=P)
    inner.load_state_dict(init_state_dict(cfg, seed=SEED), strict=False)
    model = ClassifierFreeSampleModel(inner).to(d).eval()
    prev = None
    for c, row in enumerate(ITEMS):
        where = [ds.locate(i) for i in row]
        windows = [ds.motion_window(*w) for w in where]
        audio = [ds.audio_window(*w) for w in where]
        mfcc = torch.stack([ex(torch.from_numpy(a).to(d)).t().unsqueeze(1) for a in audio]).contiguous()
        gt = gg_collate([(m, ds.text_window(*w), T, a, torch.zeros(T, MFCC_DIM), s)
                         for w, (m, s), a in zip(where, windows, audio)])[0].float().to(d)
        seed = (torch.stack([torch.from_numpy(s).t().float().unsqueeze(1) for _, s in windows]).to(d) if c == 0
                else prev[..., -P:])
        latent = df.ddim_reverse_sample_loop(inner, gt, clip_denoised=False, model_kwargs={"y": {"mfcc": mfcc, "seed": seed}})
        y = {"mfcc": mfcc, "seed": seed, "scale": torch.ones(TAKES, device=d) * SCALE}
        prev = df.ddim_sample_loop(model, (TAKES, J, 1, T), noise=latent, clip_denoised=False, model_kwargs={"y": y}, rng="philox",
                                   philox_seed=SEED + 1000 * c)
        pos, rot = E.postprocess(prev, ds.mean, ds.std)
        assert np.isfinite(res["motion"]).all()
        assert np.array_equal(res["motion"][..., c * T:(c + 1) * T], pos.cpu().numpy()), c
        assert np.array_equal(res["motion_rot"][..., c * T:(c + 1) * T], rot.cpu().numpy()), c
        drawn = df.ddim_sample_loop(model, (TAKES, J, 1, T), clip_denoised=False, model_kwargs={"y": y}, rng="philox",
                                    philox_seed=SEED + 1000 * c)
        assert not torch.equal(drawn, prev)                               # the latent did replace the drawn x_T


def test_generate_cli_invert_gt_prints_the_round_trip(tree, tmp_path, capsys):
    """With --guidance_param 1 the re-generation retraces the inversion, and the CLI prints each chunk's round-trip error."""
    from gesturediffusion_amd.sample import generate
    from test_gpu_genea_data import CHUNKS
    out = str(tmp_path / "out1")
    assert generate.main(_argv(tree, out, 1)) == 0
    text = capsys.readouterr().out
    lines = [ln for ln in text.splitlines() if "round trip max|regenerated - gt| / max|gt| = " in ln]
    assert len(lines) == CHUNKS, text
    for ln in lines:
        err = float(ln.rsplit("= ", 1)[1])
        assert np.isfinite(err) and err > 0
    res = np.load(os.path.join(out, "results.npy"), allow_pickle=True).item()      # written a moment ago
    assert set(res) == RESULT_KEYS
    argv = _argv(tree, out, 1)
    argv[argv.index("--sampler") + 1] = "p"
    with pytest.raises(SystemExit):                                       # refused before a model is built
        generate.main(argv)
