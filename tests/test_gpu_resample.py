"""RePaint resampling on the GPU (gdx_set_resample, gdx_sample_loop's walk, renoise_kernel, repaint_sample_loop, sample.generate
--edit_mode / --resample; the rule is in include/gdx.h): repeats = 1 against the plain loops, the fused loop against the hop-by-hop
twin (gdx_randn + gdx_q_sample for a forward hop) bit for bit, issue in blocks, the end of loop against the CPU restatement
(resample_restatement.py), the known region, the denoiser-call count, a side stream, the refusals and the CLI.  Need an MI355X.

Tiny models: latent_dim 64, 2 layers, 2 heads, a 20-step schedule (ddim20: model timesteps 0, 50, ..., 950).  Shape V: MDM, J = 16,
T = 20, B = 2 (320 floats per sample: the 128-bit path).  Shape S: MDM_Old, J = 5, T = 7, B = 3 (35 floats per sample: the scalar
path, and a ragged last group in every sample)."""
import numpy as np
import pytest
import torch

import resample_restatement as R
from conftest import rel_err
from misaligned import shifted
from oracle import schedule as osch
from test_gpu_parity import LOOP_TOL, _diffusion, build_model, dev

pytestmark = pytest.mark.gpu
RESP = "ddim20"
SHAPES = {"V": ("mdm", 16, 20, 2), "S": ("mdm_old", 5, 7, 3)}
PAIRS = [(2, 2), (5, 3), (7, 2)]                 # 9, 3 and 2 jump levels on 20 steps: 38, 50 and 34 denoiser calls
MID = (300, 700)                                 # guidance on 9 of the 20 schedule indices, the rest unguided
SEED = 23
_CASES = {}


def _case(name):
    """(model, config, weights, host inputs) of a shape: weights and inputs are drawn once and shared by every test."""
    if name not in _CASES:
        from gesturediffusion_amd.utils.init import init_state_dict, synthetic_inputs
        arch, J, T, B = SHAPES[name]
        cfg = dict(arch=arch, njoints=J, nfeats=1, latent_dim=64, ff_size=128, num_layers=2, num_heads=2, seed_poses=10)
        sd = init_state_dict(cfg, seed=3, perturb=True)
        x, seedp, mfcc = synthetic_inputs(cfg, B, T, seed=10)
        g = torch.Generator().manual_seed(77)
        host = dict(seed=seedp, mfcc=mfcc, mask=torch.rand(B, J, 1, T, generator=g) < 0.4,
                    motion=0.5 * torch.randn(B, J, 1, T, generator=g), init=0.5 * torch.randn(B, J, 1, T, generator=g),
                    tape=torch.randn(80, B, J, 1, T, generator=g))
        _CASES[name] = (build_model(arch, cfg, sd), cfg, sd, host)
    return _CASES[name]


def _variant(name, variant):
    """-> (model, y on the device, y on the host, keywords of repaint_sample_loop, keywords of the restatement)."""
    from gesturediffusion_amd.model.cfg_sampler import ClassifierFreeSampleModel
    model, cfg, sd, host = _case(name)
    B = host["seed"].shape[0]
    y = {"seed": host["seed"], "mfcc": host["mfcc"]}
    kw, rkw, extra = dict(clip_denoised=False), {}, {}
    if variant in ("cfg", "interval", "rescale"):
        y["scale"] = torch.full((B,), 2.5)
        model = ClassifierFreeSampleModel(model)
    if variant == "interval":
        extra["guidance_interval"] = MID
        rkw["interval"] = MID
    if variant == "rescale":
        extra["guidance_rescale"] = 0.7
        rkw["rescale"] = 0.7
    if variant == "inpaint":
        y["inpainting_mask"], y["inpainted_motion"] = host["mask"], host["motion"]
    if variant == "ddim0":
        kw.update(sampler="ddim", eta=0.0)
    if variant == "ddim05":
        kw.update(sampler="ddim", eta=0.5)
    if variant == "init_skip":
        kw.update(skip_timesteps=3)
        rkw.update(skip_timesteps=3, init_image=host["init"])
    d = dev()
    yd = dict({k: v.to(d) for k, v in y.items()}, **extra)
    if variant == "init_skip":
        kw["init_image"] = host["init"].to(d)
    return model, yd, y, kw, rkw


def _tape(name, df, jump, repeats, skip=0):
    host = _case(name)[3]
    return host["tape"][:1 + len(df.resample_plan(jump, repeats, skip_timesteps=skip))].contiguous()


# --------------------------------------------------------------------------------------------------------------- 1. off is off
@pytest.mark.parametrize("name", ["V", "S"])
@pytest.mark.parametrize("sampler", ["p", "ddim"])
def test_repeats_1_is_the_plain_loop(name, sampler):
    """repeats = 1 (any jump): torch.equal with p_sample_loop / ddim_sample_loop (eta = 0.5), under Philox noise and under a tape,
    fused and hop by hop."""
    df = _diffusion(RESP)
    model, y, _, kw, _ = _variant(name, "inpaint")
    shape = tuple(_case(name)[3]["motion"].shape)
    tape = _tape(name, df, 3, 1).to(dev())
    for noise in (dict(rng="philox", philox_seed=SEED, sample_offset=3), dict(noise_tape=tape)):
        if sampler == "p":
            want = df.p_sample_loop(model, shape, clip_denoised=False, model_kwargs={"y": y}, **noise)
        else:
            want = df.ddim_sample_loop(model, shape, clip_denoised=False, model_kwargs={"y": y}, eta=0.5, **noise)
        assert torch.isfinite(want).all()
        for fused in (True, False):
            got = df.repaint_sample_loop(model, shape, model_kwargs={"y": y}, sampler=sampler, eta=0.5, jump=3, repeats=1,
                                         fused=fused, **kw, **noise)
            assert torch.equal(got, want), (sorted(noise), fused)


# ---------------------------------------------------------------------------------------------------- 2. fused == hop by hop
@pytest.mark.parametrize("name", ["V", "S"])
@pytest.mark.parametrize("variant", ["inpaint", "cfg", "interval", "rescale", "ddim0", "ddim05", "init_skip"])
@pytest.mark.parametrize("jump,repeats", PAIRS)
def test_fused_equals_stepwise(jump, repeats, variant, name):
    """fused=True (gdx_sample_loop's walk, renoise_kernel) == fused=False (model call + gdx_sampler_update per reverse hop, gdx_randn
    or the tape + gdx_q_sample per forward hop), torch.equal, under Philox noise and under a tape; and the resampled chain differs
    from the plain one."""
    df = _diffusion(RESP)
    model, y, _, kw, _ = _variant(name, variant)
    shape = tuple(_case(name)[3]["motion"].shape)
    tape = _tape(name, df, jump, repeats, kw.get("skip_timesteps", 0)).to(dev())
    for noise in (dict(rng="philox", philox_seed=SEED, sample_offset=5), dict(noise_tape=tape)):
        outs = [df.repaint_sample_loop(model, shape, model_kwargs={"y": y}, jump=jump, repeats=repeats, fused=fused, **kw, **noise)
                for fused in (True, False)]
        assert torch.isfinite(outs[0]).all()
        assert torch.equal(outs[0], outs[1]), sorted(noise)
    plain = df.repaint_sample_loop(model, shape, model_kwargs={"y": y}, jump=jump, repeats=1, noise_tape=tape[:21 - kw.get("skip_timesteps", 0)],
                                   **kw)
    assert not torch.equal(plain, outs[0])


@pytest.mark.parametrize("jump,repeats", PAIRS)
def test_misaligned_state_and_tape_take_the_scalar_path_with_the_same_bits(jump, repeats):
    """gdx_sample_loop on a state and a tape one float off 16-byte alignment (tests/misaligned.shifted): the bits of the aligned
    run, which are those of repaint_sample_loop."""
    from gesturediffusion_amd._lib import GDX_SAMPLER_P
    df = _diffusion(RESP)
    model, y, _, kw, _ = _variant("V", "inpaint")
    shape = tuple(_case("V")[3]["motion"].shape)
    tape = _tape("V", df, jump, repeats).to(dev())
    want = df.repaint_sample_loop(model, shape, model_kwargs={"y": y}, jump=jump, repeats=repeats, noise_tape=tape, **kw)
    want_philox = df.repaint_sample_loop(model, shape, model_kwargs={"y": y}, jump=jump, repeats=repeats, rng="philox",
                                         philox_seed=SEED, noise=tape[0], **kw)
    x = tape[0].clone()
    eng, mode, scale, mask, motion = df._native_loop_setup(model, x, {"y": y})
    coef, tmap = df.coef_table(GDX_SAMPLER_P, x.device), df._timestep_map()
    eng.set_resample(jump, repeats, df.alphas_cumprod)
    try:
        for tp, ref in ((shifted(tape[1:].contiguous()), want), (None, want_philox)):
            xs = shifted(tape[0])
            assert xs.data_ptr() % 16 == 4
            eng.sample_loop(xs, GDX_SAMPLER_P, mode, coef, tmap, df.num_timesteps - 1, scale=scale, inpaint_mask=mask,
                            inpaint_motion=motion, noise_tape=tp, philox_seed=SEED)
            assert torch.equal(xs, ref), tp is None
    finally:
        eng.set_resample(1, 1)


# ------------------------------------------------------------------------------------------------------------------ 3. blocks
@pytest.mark.parametrize("name", ["V", "S"])
@pytest.mark.parametrize("sampler", ["p", "ddim"])
def test_blocks_of_3_hops_equal_one_call(name, sampler, monkeypatch):
    """(2, 2): a forward hop behind every second reverse hop from hop 18 on, so blocks of 3 hops start on a forward hop and directly
    behind one.  Blocks == one call, torch.equal, under Philox noise, a tape and torch's generator; rng="torch" == a tape drawn in
    the same order."""
    from gesturediffusion_amd.diffusion import gaussian_diffusion as gd
    df = _diffusion(RESP)
    model, y, _, kw, _ = _variant(name, "inpaint")
    kw = dict(kw, sampler=sampler, eta=0.5, jump=2, repeats=2)
    shape = tuple(_case(name)[3]["motion"].shape)
    plan = df.resample_plan(2, 2)
    starts = {k for k in range(0, len(plan), 3)}
    assert any(plan[k][0] == "f" for k in starts) and any(plan[k - 1][0] == "f" for k in starts if k)
    d = dev()
    tape = _tape(name, df, 2, 2).to(d)
    torch.manual_seed(5)
    drawn = torch.stack([torch.randn(*shape, device=d)] + [torch.empty(shape, device=d).normal_() for _ in plan])
    results = {}
    for block in (gd.NOISE_BLOCK, 3):
        monkeypatch.setattr(gd, "NOISE_BLOCK", block)
        results[block, "philox"] = df.repaint_sample_loop(model, shape, model_kwargs={"y": y}, rng="philox", philox_seed=SEED, **kw)
        results[block, "tape"] = df.repaint_sample_loop(model, shape, model_kwargs={"y": y}, noise_tape=tape, **kw)
        torch.manual_seed(5)
        results[block, "torch"] = df.repaint_sample_loop(model, shape, model_kwargs={"y": y}, rng="torch", **kw)
    assert len(plan) <= 50 and len(plan) > 3
    for noise in ("philox", "tape", "torch"):
        assert torch.equal(results[3, noise], results[50, noise]), noise
    assert torch.equal(results[3, "torch"], df.repaint_sample_loop(model, shape, model_kwargs={"y": y}, noise_tape=drawn, **kw))
    torch.manual_seed(5)
    assert torch.equal(results[3, "torch"], df.repaint_sample_loop(model, shape, model_kwargs={"y": y}, rng="torch", fused=False, **kw))


# ------------------------------------------------------------------------------------------------------------------ 4. oracle
@pytest.mark.parametrize("name", ["V", "S"])
@pytest.mark.parametrize("variant", ["inpaint", "cfg", "ddim05", "init_skip"])
def test_end_of_loop_against_the_restatement(name, variant):
    """(5, 3), 50 denoiser calls on 20 steps, the same tape: the fused loop's sample against resample_restatement.repaint_loop (the
    oracle's forward and steps, the forward hop in fp32 torch) within LOOP_TOL = 2e-4 of max|ref|, the project's stated end-of-loop
    tolerance.  Measured on an MI355X (profiles/repaint_loop.txt): 2.9e-7 .. 1.1e-6."""
    df = _diffusion(RESP)
    model, y, yh, kw, rkw = _variant(name, variant)
    _, cfg, sd, host = _case(name)
    shape = tuple(host["motion"].shape)
    skip = kw.get("skip_timesteps", 0)
    tape = _tape(name, df, 5, 3, skip)
    got = df.repaint_sample_loop(model, shape, model_kwargs={"y": y}, jump=5, repeats=3, noise_tape=tape.to(dev()), **kw)
    tab, tmap = osch.make_tables("cosine", 1000, RESP)
    want = R.repaint_loop(sd, cfg, tab, tmap, tape, yh, "ddim" if kw.get("sampler") == "ddim" else "p", 5, 3, eta=kw.get("eta", 0.0),
                          **rkw)
    err = rel_err(got.cpu(), want)
    print(f"repaint (5, 3) {name} {variant}: rel err vs restatement {err:.3e}")
    assert torch.isfinite(want).all() and err < LOOP_TOL, err


# ----------------------------------------------------------------------------------------------------------- 5. known region
@pytest.mark.parametrize("name", ["V", "S"])
@pytest.mark.parametrize("sampler", ["p", "ddim"])
def test_known_region_and_nan_outside_the_mask(name, sampler):
    """The known part of the final sample is the step kernel's own last-step expression of inpainted_motion (gdx_sampler_update at
    index 0 on x0 = the motion), bit for bit; a NaN in inpainted_motion outside the mask never reaches the output, which keeps the
    bits of the run on clean motion.  Fused and hop by hop."""
    from gesturediffusion_amd import engine as E
    from gesturediffusion_amd._lib import GDX_SAMPLER_DDIM, GDX_SAMPLER_P
    df = _diffusion(RESP)
    model, y, _, kw, _ = _variant(name, "inpaint")
    kw = dict(kw, sampler=sampler, eta=0.5, jump=5, repeats=3, rng="philox", philox_seed=SEED)
    shape = tuple(_case(name)[3]["motion"].shape)
    mask, motion = y["inpainting_mask"], y["inpainted_motion"]
    kind = GDX_SAMPLER_P if sampler == "p" else GDX_SAMPLER_DDIM
    zeros = torch.zeros(shape, device=dev())
    last = E.sampler_update(kind, df.coef_table(kind, dev(), 0.5), zeros, motion, torch.empty_like(zeros), step_index=0, noise=zeros)
    poisoned = motion.clone()
    poisoned[~mask] = float("nan")
    for fused in (True, False):
        clean = df.repaint_sample_loop(model, shape, model_kwargs={"y": y}, fused=fused, **kw)
        assert torch.equal(clean[mask], last[mask]) and torch.equal(clean[mask], motion[mask])
        got = df.repaint_sample_loop(model, shape, model_kwargs={"y": dict(y, inpainted_motion=poisoned)}, fused=fused, **kw)
        assert torch.isfinite(got).all() and torch.equal(got, clean), fused


# ------------------------------------------------------------------------------------------------------------------ 6. counts
@pytest.mark.parametrize("variant", ["inpaint", "cfg", "interval"])
@pytest.mark.parametrize("jump,repeats", PAIRS)
def test_forward_samples_rise_by_the_call_count(jump, repeats, variant):
    """gdx_forward_samples rises by calls x B, x 2 on guided hops: every reverse hop under plain guidance, the hops whose model
    timestep lies in the interval under y['guidance_interval']; a forward hop adds nothing."""
    df = _diffusion(RESP)
    model, y, _, kw, _ = _variant("V", variant)
    shape = tuple(_case("V")[3]["motion"].shape)
    B = shape[0]
    eng = _case("V")[0]._get_engine(dev())
    plan = df.resample_plan(jump, repeats)
    flags = df.guided_steps(MID if variant == "interval" else None)
    calls = [h[1] for h in plan if h[0] == "r"]
    assert len(calls) == R.calls(20, jump, repeats)
    want = sum((2 * B if variant != "inpaint" and flags[i] else B) for i in calls)
    if variant == "interval":
        assert B * len(calls) < want < 2 * B * len(calls)
    before = eng.forward_samples()
    df.repaint_sample_loop(model, shape, model_kwargs={"y": y}, jump=jump, repeats=repeats, rng="philox", philox_seed=SEED, **kw)
    assert eng.forward_samples() - before == want


# ------------------------------------------------------------------------------------------------------------- 7. side stream
def test_side_stream_has_the_bits_of_the_default_stream():
    df = _diffusion(RESP)
    model, y, _, kw, _ = _variant("V", "cfg")
    shape = tuple(_case("V")[3]["motion"].shape)
    kw = dict(kw, jump=5, repeats=3, rng="philox", philox_seed=SEED)
    want = df.repaint_sample_loop(model, shape, model_kwargs={"y": y}, **kw)
    side = torch.cuda.Stream(dev())
    side.wait_stream(torch.cuda.current_stream(dev()))
    with torch.cuda.stream(side):
        got = df.repaint_sample_loop(model, shape, model_kwargs={"y": y}, **kw)
    side.synchronize()
    assert torch.equal(got, want)


# --------------------------------------------------------------------------------------------------------------- 8. refusals
def test_refusals_while_resampling_is_on(monkeypatch):
    """With repeats > 1 the other seven loops refuse, gdx_sample_loop refuses dump_steps, const_noise, the guidance refresh, the layer
    cache and another schedule length, all before a launch (the state keeps its bits); after repaint_sample_loop's `finally`, also
    when the loop raised, plms_sample_loop runs."""
    from gesturediffusion_amd import engine as E
    from gesturediffusion_amd._lib import GDX_SAMPLER_DDIM, GDX_SAMPLER_P
    df = _diffusion(RESP)
    model, y, _, kw, _ = _variant("V", "inpaint")
    shape = tuple(_case("V")[3]["motion"].shape)
    d = dev()
    x = _case("V")[3]["tape"][0].to(d)
    keep = x.clone()
    eng, mode, scale, mask, motion = df._native_loop_setup(model, x, {"y": y})
    coef, tmap, first = df.coef_table(GDX_SAMPLER_P, d), df._timestep_map(), df.num_timesteps - 1
    hist = torch.zeros(4, *shape, device=d)
    out = torch.zeros(shape[0], df.num_timesteps, device=d)
    thr = df.parallel_threshold(0.1)
    planes = x.unsqueeze(0).repeat(2, 1, 1, 1, 1)
    eng.set_resample(2, 2, df.alphas_cumprod)
    try:
        others = {
            "gdx_plms_loop": lambda: eng.plms_loop(x, mode, 2, coef, tmap, first, hist, hist[3]),
            "gdx_dpm_loop": lambda: eng.dpm_loop(x, mode, 2, coef, tmap, first, hist),
            "gdx_dpm_sde_loop": lambda: eng.dpm_sde_loop(x, mode, 2, coef, tmap, first, hist),
            "gdx_unipc_loop": lambda: eng.unipc_loop(x, mode, 2, coef, hist[0], tmap, first, hist, hist[3]),
            "gdx_ddim_reverse_loop": lambda: eng.ddim_reverse_loop(x, mode, coef, tmap, 0, 3),
            "gdx_parallel_loop": lambda: eng.parallel_loop(planes, GDX_SAMPLER_P, mode, coef, tmap, thr, first),
            "gdx_bpd_loop": lambda: eng.bpd_loop(x, mode, coef, tmap, out, out.clone(), out.clone()),
        }
        for who, call in others.items():
            with pytest.raises(E.GdxError, match=f"{who}: resampling is on"):
                call()
        with pytest.raises(E.GdxError, match="does not support dump_steps"):
            eng.sample_loop(x, GDX_SAMPLER_P, mode, coef, tmap, first, dump=hist, dump_steps=[1, 2])
        with pytest.raises(E.GdxError, match="does not support const_noise"):
            eng.sample_loop(x, GDX_SAMPLER_P, mode, coef, tmap, first, const_noise=True)
        with pytest.raises(E.GdxError, match="neither const_noise nor dump_steps"):
            eng.sample_loop(x, GDX_SAMPLER_DDIM, mode, coef, tmap, first, const_noise=True)
        eng.set_guidance_refresh(2)
        with pytest.raises(E.GdxError, match="guidance refresh .* exclude each other"):
            eng.sample_loop(x, GDX_SAMPLER_P, mode, coef, tmap, first)
        eng.set_guidance_refresh(1)
        eng.set_layer_cache(2, 1)
        with pytest.raises(E.GdxError, match="layer cache .* exclude each other"):
            eng.sample_loop(x, GDX_SAMPLER_P, mode, coef, tmap, first)
        eng.set_layer_cache(1, 0)
        eng.set_resample(2, 2, df.alphas_cumprod[:10])
        with pytest.raises(E.GdxError, match="set for a schedule of 10 steps, the loop has 20"):
            eng.sample_loop(x, GDX_SAMPLER_P, mode, coef, tmap, first)
        eng.set_resample(2, 2, df.alphas_cumprod)
        for k_base, run_steps in ((len(df.resample_plan(2, 2)), 0), (0, len(df.resample_plan(2, 2)) + 1)):
            with pytest.raises(E.GdxError, match="bad step range"):
                eng.sample_loop(x, GDX_SAMPLER_P, mode, coef, tmap, first, k_base=k_base, run_steps=run_steps)
    finally:
        eng.set_resample(1, 1)
    torch.cuda.synchronize()
    assert torch.equal(x, keep)                               # every refusal came before a launch
    want = df.plms_sample_loop(model, shape, noise=x, clip_denoised=False, model_kwargs={"y": y})
    assert torch.isfinite(want).all()

    def broken(self, *a, **k):
        raise RuntimeError("the loop failed")
    with monkeypatch.context() as m:
        m.setattr(E.Engine, "sample_loop", broken)
        with pytest.raises(RuntimeError, match="the loop failed"):
            df.repaint_sample_loop(model, shape, model_kwargs={"y": y}, jump=2, repeats=2, noise=x, **kw)
    assert torch.equal(df.plms_sample_loop(model, shape, noise=x, clip_denoised=False, model_kwargs={"y": y}), want)


# --------------------------------------------------------------------------------------------------------------------- 9. CLI
@pytest.mark.parametrize("extra", [["--arch_version", "mdm", "--edit_mode", "in_between", "--resample", "5", "2"],
                                   ["--arch_version", "mdm_old", "--sampler", "ddim", "--resample", "10", "2", "--rng", "philox"]])
def test_generate_cli_in_between_and_resample(tmp_path, extra, capsys):
    """sample.generate --synthetic with --resample, with and without --edit_mode in_between, two chunks on 25 steps: the hop and
    call counts are printed, results.npy is finite, and under --edit_mode the kept frames of every chunk (37 features: the
    normalised poses are written) are the synthetic ground truth bit for bit while the gap is not."""
    from gesturediffusion_amd.sample import generate
    out = tmp_path / "out"
    base = ["--synthetic", "--latent_dim", "128", "--layers", "2", "--num_samples", "3", "--chunks", "2", "--synthetic_njoints", "37",
            "--num_frames", "20", "--timestep_respacing", "25", "--output_dir", str(out), "--seed", "7"]
    assert generate.main(base + extra) == 0
    text = capsys.readouterr().out
    jump, repeats = (int(v) for v in extra[extra.index("--resample") + 1:][:2])
    calls = R.calls(25, jump, repeats)
    assert f"{len(R.hops(25, jump, repeats))} hops, {calls} denoiser calls per chunk" in text
    assert ("in-betweening: frames 5..14 of 20 are generated" in text) == ("--edit_mode" in extra)
    res = np.load(out / "results.npy", allow_pickle=True).item()      # written by this test a moment ago
    assert res["motion"].shape == (3, 37, 1, 40) and np.isfinite(res["motion"]).all() and np.abs(res["motion"]).max() > 0
    if "--edit_mode" in extra:                                 # the kept frames of every chunk are the synthetic ground truth
        gt = generate.synthetic_ground_truth(7, 3, 37, 20, 2)
        for c in range(2):
            chunk = res["motion"][..., 20 * c:20 * (c + 1)]
            assert np.array_equal(chunk[..., :5], gt[c][..., :5].numpy()) and np.array_equal(chunk[..., 15:], gt[c][..., 15:].numpy())
            assert not np.array_equal(chunk[..., 5:15], gt[c][..., 5:15].numpy())
