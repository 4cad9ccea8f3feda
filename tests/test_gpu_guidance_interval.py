"""Guidance interval on the GPU (y['guidance_interval'], gdx_set_guidance_interval, gdx_forward_samples; include/gdx.h): a guided
loop limited to an interval against the composition of today's step methods bit for bit, the two ends of the range, the
step-wise forward's per-sample choice, the denoiser samples actually skipped, the CPU restatement, gdx_bpd_loop, graph replay,
workspace guards and the CLI.

Shapes: TINY (J = 16, d = 128, L = 2), B = 2 with scales (2.5, -1.0); 10-step loops on ddim10 (cosine) and, for the DPM loops,
logsnr10 (linear: ten kept timesteps).  T = 20 takes gdx_sample_loop's token-major path (T % 4 == 0, V2 needs T % 10 == 0),
T = 10 the pose-layout path; MDM_Old also runs T = 12 (token-major, no multiple of 10)."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import guidance_interval_restatement as GR
from conftest import load_golden, rel_err, weights_from
from test_dpm_host import diffusion
from test_gpu_parity import LOOP_TOL, TINY, build_model, dev

pytestmark = pytest.mark.gpu
B = 2
SCALES = (2.5, -1.0)
MID = (300, 700)         # ddim10: 900, 800 unguided, 700 .. 300 guided, 200 .. 0 unguided; logsnr10: guided at 603 and 410
EMPTY, ALL = (1, 0), (0, 999)
SHAPES = [("mdm", 20), ("mdm", 10), ("mdm_old", 20), ("mdm_old", 12), ("mdm_old", 10)]
SAMPLERS = ["p", "ddim", "plms", "dpmpp", "dpmpp_sde"]
NOISY = ("p", "dpmpp_sde")
SEED = 77
DDIM_ETA = 0.5           # so that ddim_sample_loop reads its noise


@functools.lru_cache(maxsize=None)
def _model(arch, dtype):
    m = build_model(arch, TINY, weights_from(load_golden(f"loops_{arch}_tiny.npz")))
    m.compute_dtype = dtype
    return m


@functools.lru_cache(maxsize=None)
def _inputs(T):
    """Inputs of one frame count, drawn once on the host and shared (never written) by every test."""
    g = torch.Generator().manual_seed(1000 + T)
    r = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    host = dict(seed=r(B, 16, 1, 10), mfcc=r(B, 26, 1, T), tape=r(11, B, 16, 1, T), motion=0.5 * r(B, 16, 1, T),
                mask=torch.rand(B, 16, 1, T, generator=g) < 0.3, scale=torch.tensor(SCALES), x_start=0.5 * r(B, 16, 1, T))
    return host, {k: v.to(dev()) for k, v in host.items()}


def _df(sampler):
    return diffusion("linear", "logsnr10") if sampler.startswith("dpmpp") else diffusion("cosine", "ddim10")


def _ys(T, variant="plain", interval=None):
    """(y of the guided model [with the key when an interval is given], y of the inner model: no scale, no key)."""
    _, i = _inputs(T)
    y_in = {"seed": i["seed"], "mfcc": i["mfcc"]}
    if variant == "inpaint":
        y_in.update(inpainting_mask=i["mask"], inpainted_motion=i["motion"])
    y_cfg = dict(y_in, scale=i["scale"])
    if interval is not None:
        y_cfg["guidance_interval"] = interval
    return y_cfg, y_in


def _cfg(m):
    from gesturediffusion_amd.model.cfg_sampler import ClassifierFreeSampleModel
    return ClassifierFreeSampleModel(m)


def _loop(df, sampler, model, y, T, clip=False, rng="tape", fused=True):
    """The sampler's whole-loop method on the shared inputs."""
    tape = _inputs(T)[1]["tape"]
    kw = dict(clip_denoised=clip, model_kwargs={"y": y}, fused=fused)
    if sampler in ("p", "ddim", "dpmpp_sde"):
        kw.update(dict(noise_tape=tape) if rng == "tape" else dict(rng="philox", philox_seed=SEED))
    else:
        kw["noise"] = tape[0].clone()
    shape = tuple(tape.shape[1:])
    if sampler == "p":
        return df.p_sample_loop(model, shape, **kw)
    if sampler == "ddim":
        return df.ddim_sample_loop(model, shape, eta=DDIM_ETA, **kw)
    if sampler == "plms":
        return df.plms_sample_loop(model, shape, order=2, **kw)
    if sampler == "dpmpp":
        return df.dpm_solver_sample_loop(model, shape, order=2, **kw)
    return df.dpm_solver_sde_sample_loop(model, shape, order=2, eta=1.0, **kw)


@contextlib.contextmanager
def _randn_like(z):
    """p_sample / ddim_sample draw with torch.randn_like: hand them the step's recorded noise instead."""
    orig = torch.randn_like
    torch.randn_like = lambda x, *a, **k: z
    try:
        yield
    finally:
        torch.randn_like = orig


def _hand_loop(df, sampler, m, T, variant, interval, rng="tape"):
    """The composition: today's step method per step, with the guided model on the steps the flag function marks and the inner
    model (y without scale) on the others; the same noise as the fused loop."""
    from gesturediffusion_amd import engine as E
    flags = df.guided_steps(interval)
    n, d = df.num_timesteps, dev()
    tape = _inputs(T)[1]["tape"]
    shape = tuple(tape.shape[1:])
    if rng == "tape":
        x, z = tape[0], (lambda k: tape[1 + k])
    else:
        x, z = E.randn(shape, d, SEED, 0, 0), (lambda k: E.randn(shape, d, SEED, 0, k + 1))
    y_cfg, y_in = _ys(T, variant)
    guided_model = _cfg(m)
    if sampler == "plms":
        assert flags[n - 1] == flags[n - 2], "plms_sample's first step runs both forwards on one model"
    old = None
    for k, i in enumerate(range(n - 1, -1, -1)):
        t = torch.full((B,), i, device=d, dtype=torch.long)
        model, y = (guided_model, y_cfg) if flags[i] else (m, y_in)
        kw = dict(clip_denoised=variant == "clip", model_kwargs={"y": y})
        if sampler == "p":
            with _randn_like(z(k)):
                out = df.p_sample(model, x, t, **kw)
        elif sampler == "ddim":
            with _randn_like(z(k)):
                out = df.ddim_sample(model, x, t, eta=DDIM_ETA, **kw)
        elif sampler == "plms":
            out = old = df.plms_sample(model, x, t, order=2, old_out=old, **kw)
        elif sampler == "dpmpp":
            out = old = df.dpm_solver_sample(model, x, t, order=2, old_out=old, **kw)
        else:
            out = old = df.dpm_solver_sde_sample(model, x, t, order=2, eta=1.0, old_out=old, noise=z(k), **kw)
        x = out["sample"]
    return x


# ------------------------------------------------------------------------------------------------- 1. composition, bit for bit
@pytest.mark.parametrize("arch,T", SHAPES)
@pytest.mark.parametrize("sampler", SAMPLERS)
def test_interval_loop_is_the_composition_of_todays_steps(arch, T, sampler):
    """Fused loop on the guided model with the key == the hand loop over the existing step methods, torch.equal: unguided ->
    guided -> unguided (a stale uncond half of the token-major state would show on the first guided step); plain, inpainting
    (pose-layout path), clip_denoised; Philox noise for the two noisy samplers; fp32 and fp16."""
    df = _df(sampler)
    flags = df.guided_steps(MID)
    assert not flags[-1] and not flags[0] and any(flags)
    ran = 0
    for dtype in ("fp32", "fp16"):
        m = _model(arch, dtype)
        cases = [("plain", "tape"), ("inpaint", "tape"), ("clip", "tape")] + ([("plain", "philox")] if sampler in NOISY else [])
        for variant, rng in cases:
            y_key, _ = _ys(T, variant, MID)
            fused = _loop(df, sampler, _cfg(m), y_key, T, clip=variant == "clip", rng=rng)
            hand = _hand_loop(df, sampler, m, T, variant, MID, rng)
            tag = (arch, T, sampler, dtype, variant, rng)
            assert torch.isfinite(fused).all(), tag
            assert torch.equal(fused, hand), tag
            if variant == "plain" and rng == "tape":        # and the interval does something: not the loop guided throughout
                assert not torch.equal(fused, _loop(df, sampler, _cfg(m), _ys(T)[0], T)), tag
            ran += 1
    assert ran == (8 if sampler in NOISY else 6)


# ----------------------------------------------------------------------------------------------------- 2. ends of the range
@pytest.mark.parametrize("arch,T", SHAPES)
@pytest.mark.parametrize("dtype", ["fp32", "fp16", "bf16"])
def test_ends_of_the_range(arch, T, dtype):
    """An interval over every timestep == the loop without the key; the empty interval == the same loop on the inner model."""
    m = _model(arch, dtype)
    for sampler in SAMPLERS:
        df = _df(sampler)
        y_cfg, y_in = _ys(T)
        every = _loop(df, sampler, _cfg(m), _ys(T, interval=ALL)[0], T)
        assert torch.equal(every, _loop(df, sampler, _cfg(m), y_cfg, T)), (sampler, "all")
        never = _loop(df, sampler, _cfg(m), _ys(T, interval=EMPTY)[0], T)
        assert torch.equal(never, _loop(df, sampler, m, y_in, T)), (sampler, "empty")
        assert torch.isfinite(every).all() and torch.isfinite(never).all() and not torch.equal(every, never)


# ------------------------------------------------------------------------------------------------------ 3. step-wise forward
@pytest.mark.parametrize("arch,T", SHAPES)
@pytest.mark.parametrize("dtype", ["fp32", "fp16", "bf16"])
def test_stepwise_forward_selects_per_sample(arch, T, dtype):
    """Per-sample timesteps on both sides of the interval, t = (100, 600) under (300, 700): row 0 is the inner model's
    conditional output, row 1 today's blend.  Then with the bounds on the timesteps themselves (inclusive), an empty interval
    and a handle that must not keep the interval of the call before."""
    m = _model(arch, dtype)
    d = dev()
    x = _inputs(T)[1]["tape"][3]
    t = torch.tensor([100, 600], device=d)
    y_cfg, y_in = _ys(T)
    cond = m(x, t, y=y_in)
    blend = _cfg(m)(x, t, y=y_cfg)
    assert not torch.equal(cond[1], blend[1])
    got = _cfg(m)(x, t, y=dict(y_cfg, guidance_interval=MID))
    assert torch.equal(got[0], cond[0]), "unguided row: the conditional output itself"
    assert torch.equal(got[1], blend[1]), "guided row: today's blend"
    got = _cfg(m)(x, t, y=dict(y_cfg, guidance_interval=(100, 100)))
    assert torch.equal(got[0], blend[0]) and torch.equal(got[1], cond[1])
    got = _cfg(m)(x, t, y=dict(y_cfg, guidance_interval=(101, 599)))
    assert torch.equal(got, cond)
    assert torch.equal(_cfg(m)(x, t, y=dict(y_cfg, guidance_interval=EMPTY)), cond)
    assert torch.equal(_cfg(m)(x, t, y=y_cfg), blend), "key absent after a call with one: every timestep again"


@pytest.mark.parametrize("arch,T", SHAPES)
def test_stepwise_loop_equals_fused(arch, T):
    """The loop of test 1 with fused=False (the guided model called step by step with the key) == the fused one."""
    m = _model(arch, "fp32")
    for sampler in SAMPLERS:
        df = _df(sampler)
        y_key, _ = _ys(T, "plain", MID)
        fused = _loop(df, sampler, _cfg(m), y_key, T)
        assert torch.equal(fused, _loop(df, sampler, _cfg(m), y_key, T, fused=False)), sampler


def test_refusals_of_the_key():
    """A key on a model that runs no guidance, and anything but two ints, raise ValueError -- in the loops and step-wise."""
    m = _model("mdm", "fp32")
    d = dev()
    T = 20
    df = _df("p")
    y_cfg, y_in = _ys(T)
    x = _inputs(T)[1]["tape"][0]
    t = torch.tensor([100, 600], device=d)
    for sampler in SAMPLERS:
        with pytest.raises(ValueError, match="ClassifierFreeSampleModel"):
            _loop(_df(sampler), sampler, m, dict(y_in, guidance_interval=MID), T)
    with pytest.raises(ValueError, match="ClassifierFreeSampleModel"):
        m(x, t, y=dict(y_in, guidance_interval=MID))
    with pytest.raises(ValueError, match="ClassifierFreeSampleModel"):
        df.calc_bpd_loop(m, x, model_kwargs={"y": dict(y_in, guidance_interval=MID)})
    for bad in ((300,), (300.0, 700), torch.tensor([300, 700], device=d), torch.tensor([300, 700])):
        with pytest.raises(ValueError, match="guidance_interval"):
            _loop(df, "p", _cfg(m), dict(y_cfg, guidance_interval=bad), T)
        with pytest.raises(ValueError, match="guidance_interval"):
            _cfg(m)(x, t, y=dict(y_cfg, guidance_interval=bad))


# --------------------------------------------------------------------------------------------------- 4. work actually skipped
def _interval_with(df, G):
    tmap = df.timestep_map
    iv = {0: EMPTY, 4: (tmap[3], tmap[6]), 10: ALL}[G]
    assert sum(df.guided_steps(iv)) == G and df.num_timesteps == 10
    return iv


@pytest.mark.parametrize("arch,T", [("mdm", 20), ("mdm", 10), ("mdm_old", 12)])
@pytest.mark.parametrize("sampler", SAMPLERS)
def test_unguided_steps_skip_the_unconditional_pass(arch, T, sampler):
    """gdx_forward_samples around a fused 10-step loop with G guided steps advances by B * (10 - G) + 2 * B * G; PLMS's extra
    first-step forward (index 8) counts by its own timestep."""
    m = _model(arch, "fp32")
    df = _df(sampler)
    eng = m._get_engine(dev())
    for G in (0, 4, 10):
        iv = _interval_with(df, G)
        flags = df.guided_steps(iv)
        want = B * (10 - G) + 2 * B * G
        if sampler == "plms":
            want += 2 * B if flags[8] else B
        before = eng.forward_samples()
        r = _loop(df, sampler, _cfg(m), _ys(T, interval=iv)[0], T)
        assert eng is m._get_engine(dev())
        assert eng.forward_samples() - before == want, (G, eng.forward_samples() - before, want)
        assert torch.isfinite(r).all()
    # the loop without the key pays for guidance on every step, the inner model on none
    before = eng.forward_samples()
    _loop(df, sampler, _cfg(m), _ys(T)[0], T)
    assert eng.forward_samples() - before == 2 * B * (11 if sampler == "plms" else 10)
    before = eng.forward_samples()
    _loop(df, sampler, m, _ys(T)[1], T)
    assert eng.forward_samples() - before == B * (11 if sampler == "plms" else 10)


# ------------------------------------------------------------------------------------------------------ 5. against the oracle
@functools.lru_cache(maxsize=None)
def _oracle(arch, T, sampler):
    host, _ = _inputs(T)
    p = weights_from(load_golden(f"loops_{arch}_tiny.npz"))
    cfg = dict(TINY, arch=arch)
    y = {"seed": host["seed"], "mfcc": host["mfcc"], "scale": host["scale"]}
    if sampler == "dpmpp":
        tmap = diffusion("linear", "logsnr10").timestep_map
        return torch.from_numpy(GR.dpm_loop(p, cfg, MID, "linear", tmap, host["tape"][0], y, 2))
    return GR.sample_loop(p, cfg, MID, "cosine", "ddim10", host["tape"], y, sampler, eta=DDIM_ETA if sampler == "ddim" else 0.0)


@pytest.mark.parametrize("arch,T", [("mdm", 20), ("mdm", 10), ("mdm_old", 12), ("mdm_old", 10)])
@pytest.mark.parametrize("sampler", ["p", "ddim", "dpmpp"])
def test_interval_loop_vs_cpu_restatement(arch, T, sampler):
    """The loop of test 1 against the CPU restatement (oracle forwards, oracle loops / the fp64 DPM recurrence): fp32 within the
    suite's LOOP_TOL, fp16 / bf16 within numerics.stated_tolerance for the largest guidance factor of the scales used."""
    from gesturediffusion_amd.numerics import guidance_factor, stated_tolerance
    want = _oracle(arch, T, sampler)
    worst = max(SCALES, key=guidance_factor)
    for dtype in ("fp32", "fp16", "bf16"):
        tol = LOOP_TOL if dtype == "fp32" else stated_tolerance(dtype, worst)
        got = _loop(_df(sampler), sampler, _cfg(_model(arch, dtype)), _ys(T, interval=MID)[0], T)
        err = rel_err(got.cpu(), want)
        print(f"{arch} T={T} {sampler} {dtype}: rel err vs the restatement {err:.3e} (tolerance {tol:.1e})")
        assert err < tol, (dtype, err)


# ------------------------------------------------------------------------------------------------------------ 6. gdx_bpd_loop
def test_bpd_loop_equals_the_stepwise_terms():
    """calc_bpd_loop on the guided model with the mid interval: gdx_bpd_loop (per-step mode on the host) == the step-wise
    _vb_terms_bpd route (double batch, per-sample choice in the blend kernel), bit for bit."""
    m = _model("mdm", "fp32")
    df = _df("p")
    T = 20
    _, i = _inputs(T)
    y_key, _ = _ys(T, interval=MID)
    kw = dict(clip_denoised=True, model_kwargs={"y": y_key}, noise_tape=i["tape"][:10].contiguous())
    eng = m._get_engine(dev())
    before = eng.forward_samples()
    fused = df.calc_bpd_loop(_cfg(m), i["x_start"], **kw)
    assert eng.forward_samples() - before == B * 5 + 2 * B * 5
    step = df.calc_bpd_loop(_cfg(m), i["x_start"], fused=False, **kw)
    for k in ("total_bpd", "prior_bpd", "vb", "xstart_mse", "mse"):
        assert torch.isfinite(fused[k]).all() and torch.equal(fused[k], step[k]), k
    plain = df.calc_bpd_loop(_cfg(m), i["x_start"], **dict(kw, model_kwargs={"y": _ys(T)[0]}))
    assert not torch.equal(plain["vb"], fused["vb"])


# ------------------------------------------------------------------------------------------------------------ 7. graph replay
@pytest.mark.parametrize("arch", ["mdm", "mdm_old"])
def test_graph_replay_with_an_interval_equals_eager(arch):
    """Graph replay on: a call whose steps change mode runs eagerly, one whose steps share a mode (every timestep / none)
    replays its captured step; all three equal the eager results, and the counter counts replayed steps like eager ones."""
    m = _model(arch, "fp32")
    eng = m._get_engine(dev())
    T = 20
    for sampler in ("p", "ddim"):
        df = _df(sampler)
        eager = {iv: _loop(df, sampler, _cfg(m), _ys(T, interval=iv)[0], T) for iv in (MID, ALL, EMPTY)}
        eng.set_graph_replay(True)
        try:
            for iv, G in ((MID, 5), (ALL, 10), (EMPTY, 0)):
                before = eng.forward_samples()
                r = _loop(df, sampler, _cfg(m), _ys(T, interval=iv)[0], T)
                assert torch.equal(r, eager[iv]), (sampler, iv)
                assert eng.forward_samples() - before == B * (10 - G) + 2 * B * G, (sampler, iv)
        finally:
            eng.set_graph_replay(False)


# -------------------------------------------------------------------------------------------------------- 8. workspace guards
@pytest.mark.parametrize("arch,T", [("mdm", 20), ("mdm", 10), ("mdm_old", 12)])
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_interval_loop_leaves_the_workspace_guards_intact(arch, T, dtype):
    m = _model(arch, dtype)
    d = dev()
    eng = m._get_engine(d)
    eng.set_guards(True)
    try:
        for sampler in SAMPLERS:
            r = _loop(_df(sampler), sampler, _cfg(m), _ys(T, interval=MID)[0], T)
            bad, zone = eng.check_guards(d)
            assert bad == 0, f"{sampler}: {bad} canary bytes overwritten, first in workspace allocation #{zone}"
            assert torch.isfinite(r).all()
    finally:
        eng.set_guards(False)


# --------------------------------------------------------------------------------------------------------------------- 9. CLI
def test_generate_cli_with_an_interval_equals_a_direct_call(tmp_path, capsys):
    """`sample.generate --synthetic --guidance_interval 300 700 --sampler dpmpp --timestep_respacing logsnr10 --chunks 2` at a
    small width: both chunks equal a direct sample_chunks call on the inputs the CLI builds from its seed, and the printed
    count of guided steps is the flag function's."""
    import re
    from gesturediffusion_amd.sample import generate
    from gesturediffusion_amd.utils.init import MFCC_DIM, init_state_dict
    from gesturediffusion_amd.utils.model_util import create_model_and_diffusion
    from gesturediffusion_amd.utils.parser_util import generate_args
    out = tmp_path / "out"
    argv = ["--synthetic", "--guidance_interval", "300", "700", "--sampler", "dpmpp", "--timestep_respacing", "logsnr10",
            "--chunks", "2", "--latent_dim", "128", "--layers", "2", "--num_samples", "3", "--synthetic_njoints", "37",
            "--output_dir", str(out), "--seed", "7", "--arch_version", "mdm", "--num_frames", "20", "--rng", "philox"]
    assert generate.main(argv) == 0
    printed = capsys.readouterr().out
    res = np.load(out / "results.npy", allow_pickle=True).item()      # written by this test a moment ago
    assert res["motion"].shape == (3, 37, 1, 40) and np.isfinite(res["motion"]).all()
    d = dev()
    args = generate_args(argv)
    args.mfcc_input = True
    model, df = create_model_and_diffusion(args, None)
    flags = df.guided_steps((300, 700))
    said = re.search(r"guidance on (\d+) of (\d+) steps", printed)
    assert said and (int(said.group(1)), int(said.group(2))) == (sum(flags), len(flags)) and 0 < sum(flags) < len(flags)
    cfg = dict(arch="mdm", njoints=37, nfeats=1, latent_dim=128, ff_size=1024, num_layers=2, num_heads=4, seed_poses=args.seed_poses)
    model.load_state_dict(init_state_dict(cfg, seed=7), strict=False)
    model = _cfg(model).to(d).eval()
    gen = torch.Generator().manual_seed(7)
    seedp = torch.randn(3, 37, 1, args.seed_poses, generator=gen).to(d)
    mfcc = lambda chunk: torch.randn(3, MFCC_DIM, 1, 20, generator=gen).to(d)   # noqa: E731
    kw = dict(guidance_param=args.guidance_param, sampler="dpmpp", rng="philox", philox_seed=7, dpm_order=2)
    want = generate.sample_chunks(model, df, seedp, mfcc, 2, 20, args.seed_poses, guidance_interval=(300, 700), **kw)
    assert np.array_equal(res["motion"], torch.cat(want, dim=3).cpu().numpy())
    gen.manual_seed(7)
    torch.randn(3, 37, 1, args.seed_poses, generator=gen)
    plain = generate.sample_chunks(model, df, seedp, mfcc, 2, 20, args.seed_poses, **kw)
    assert not np.array_equal(res["motion"], torch.cat(plain, dim=3).cpu().numpy())
