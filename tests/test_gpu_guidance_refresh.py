"""Guidance refresh on the GPU (y['guidance_refresh'], gdx_set_guidance_refresh, gdx_cfg_delta; include/gdx.h): the stand-alone
pass against torch.sub, no key / every = 1 against today's loops, the fused loops against a hand loop built from today's pieces
bit for bit, the denoiser samples actually skipped, block-wise issue and its refusal, the CPU restatement, graph replay,
workspace guards, the refusals of everything without memory, and the CLI.

Loops: the TINY model, inputs, samplers and schedules of test_gpu_guidance_interval.py (B = 2, scales (2.5, -1.0), 10 steps).
T = 20 takes gdx_sample_loop's token-major path without the key, so the switch to the pose-layout path is exercised."""
import functools
import math

import numpy as np
import pytest
import torch

import guidance_refresh_restatement as FR
from conftest import load_golden, rel_err, weights_from
from misaligned import shifted
from test_dpm_host import diffusion
from test_gpu_guidance_interval import (DDIM_ETA, MID, NOISY, SAMPLERS, SCALES, SEED, SHAPES, _cfg, _df, _inputs, _loop, _model,
                                        _randn_like, _ys)
from test_gpu_parity import LOOP_TOL, TINY, dev

pytestmark = pytest.mark.gpu
B = 2
PHI = 0.7
COUNTS = (1, 3, 4, 16 * 20 * 2, 4099)
SENTINEL = math.nan


def _key(y, every=2, **more):
    return dict(y, guidance_refresh=every, **more)


def _plan(df, every, sampler, interval=None):
    """The rule from the restatement's counter (not the package's guidance_plan) on the diffusion's per-index flags."""
    return FR.plan(df.guided_steps(interval), every, plms=sampler == "plms")


# ------------------------------------------------------------------------------------------------ 1. gdx_cfg_delta against torch
@pytest.mark.parametrize("misaligned", [False, True])
@pytest.mark.parametrize("count", COUNTS)
def test_cfg_delta_against_torch(count, misaligned):
    """out = a - b == torch.sub bit for bit on aligned operands (the 128-bit path when count % 4 == 0) and on views one float off
    alignment (the scalar path and its tail); NaN sentinels in front of and behind the output survive; out may be b itself; a
    count shorter than the tensors leaves the rest alone."""
    from gesturediffusion_amd import engine as E
    d = dev()
    g = torch.Generator().manual_seed(count)
    a_h, b_h = torch.randn(count, generator=g), torch.randn(count, generator=g) * 3
    a_h[0], b_h[-1] = math.inf, -0.0                           # special values go through like any other
    place = shifted if misaligned else (lambda t: t)
    a, b = place(a_h.to(d)), place(b_h.to(d))
    assert (a.data_ptr() % 16 != 0) == misaligned and (b.data_ptr() % 16 != 0) == misaligned
    want = torch.sub(a, b)
    lead = 4 + int(misaligned)                                 # aligned: 16 bytes of sentinels in front, misaligned: 20
    buf = torch.full((lead + count + 64,), SENTINEL, device=d)
    out = buf[lead:lead + count]
    assert (out.data_ptr() % 16 != 0) == misaligned
    got = E.cfg_delta(a, b, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(out, want), (count, misaligned)
    assert bool(torch.isnan(buf[:lead]).all()) and bool(torch.isnan(buf[lead + count:]).all()), (count, misaligned)
    # in place on b (the reuse call's u' = c - d lands where d's operand was read)
    b2 = place(b_h.to(d))
    E.cfg_delta(a, b2, out=b2)
    assert torch.equal(b2, want), (count, misaligned)
    # a fresh output without `out`
    assert torch.equal(E.cfg_delta(a, b), want)
    # count below the tensors' length: elements past it keep their sentinel
    if count > 1:
        buf.fill_(SENTINEL)
        E.cfg_delta(a, b, out=out, count=count - 1)
        assert torch.equal(out[:count - 1], want[:count - 1]) and bool(torch.isnan(buf[lead + count - 1:]).all())


def test_cfg_delta_mixed_alignment_takes_the_scalar_path():
    """One misaligned operand out of three is enough for the scalar path; the result is the same."""
    from gesturediffusion_amd import engine as E
    d = dev()
    g = torch.Generator().manual_seed(5)
    a, b = torch.randn(640, generator=g).to(d), torch.randn(640, generator=g).to(d)
    want = torch.sub(a, b)
    for which in range(3):
        ops = [a.clone(), b.clone(), torch.full((640,), SENTINEL, device=d)]
        ops[which] = shifted(ops[which])
        E.cfg_delta(ops[0], ops[1], out=ops[2])
        assert torch.equal(ops[2], want), which


# ------------------------------------------------------------------------------------ 2. no key and every = 1 change nothing
@pytest.mark.parametrize("arch,T", [("mdm", 20), ("mdm", 10), ("mdm_old", 12)])
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_every_one_is_todays_loop(arch, T, dtype):
    """every = 1 == no key, bit for bit and with the same gdx_forward_samples, for the five samplers; and a call without the
    key after one with every = 2 on the same engine is today's loop again (a handle that kept its setting would show here)."""
    m = _model(arch, dtype)
    eng = m._get_engine(dev())
    y0 = _ys(T)[0]
    for sampler in SAMPLERS:
        df = _df(sampler)
        before = eng.forward_samples()
        today = _loop(df, sampler, _cfg(m), y0, T)
        ran = eng.forward_samples() - before
        assert ran == 2 * B * (11 if sampler == "plms" else 10)
        before = eng.forward_samples()
        assert torch.equal(_loop(df, sampler, _cfg(m), _key(y0, 1), T), today), sampler
        assert eng.forward_samples() - before == ran, sampler
        assert not torch.equal(_loop(df, sampler, _cfg(m), _key(y0, 2), T), today), sampler
        before = eng.forward_samples()
        assert torch.equal(_loop(df, sampler, _cfg(m), y0, T), today), (sampler, "a handle kept its setting")
        assert eng.forward_samples() - before == ran, sampler


# ------------------------------------------------------------------------------------------------- 3. composition, bit for bit
class _HandModel:
    """The guided model of the hand loop, from today's pieces: the inner model's conditional forward; on a refresh its
    unconditional forward and d = torch.sub(c, u); on a reuse u' = torch.sub(c, d); then the blend u + s (c - u) -- the existing
    gdx_cfg_rescale entry, which at phi = 0 is the blend itself (f = 1 exactly) and at phi > 0 the rescale the fused loop runs.
    The step methods of today (p_sample, ddim_sample, plms_sample, dpm_solver_sample, dpm_solver_sde_sample) call it once per
    denoiser call, in execution order, and do inpainting, clip_denoised, the noise and the history as ever."""

    def __init__(self, m, plan, phi=0.0):
        self.m, self.calls, self.phi, self.d, self.seen = m, iter(plan), phi, None, []

    def __call__(self, x, t, y=None):
        what = next(self.calls)
        self.seen.append(what)
        y_in = {k: v for k, v in y.items() if k not in ("scale", "guidance_interval", "guidance_refresh", "guidance_rescale")}
        c = self.m(x, t, y=y_in)
        if what == "off":
            return c
        if what == "refresh":
            u = self.m(x, t, y=dict(y_in, uncond=True))
            self.d = torch.sub(c, u)
        else:
            u = torch.sub(c, self.d)
        eng = self.m._get_engine(x.device)
        return eng.cfg_rescale(c, u, y["scale"].reshape(-1).contiguous(), self.phi)[0]


def _hand_loop(df, sampler, m, T, variant, plan, rng="tape", phi=0.0):
    from gesturediffusion_amd import engine as E
    n, d = df.num_timesteps, dev()
    tape = _inputs(T)[1]["tape"]
    shape = tuple(tape.shape[1:])
    if rng == "tape":
        x, z = tape[0], (lambda k: tape[1 + k])
    else:
        x, z = E.randn(shape, d, SEED, 0, 0), (lambda k: E.randn(shape, d, SEED, 0, k + 1))
    model = _HandModel(m, plan, phi)
    kw = dict(clip_denoised=variant == "clip", model_kwargs={"y": _ys(T, variant)[0]})
    old = None
    for k, i in enumerate(range(n - 1, -1, -1)):
        t = torch.full((B,), i, device=d, dtype=torch.long)
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
    assert model.seen == list(plan) and next(model.calls, None) is None
    return x


@pytest.mark.parametrize("arch,T", SHAPES)
@pytest.mark.parametrize("sampler", SAMPLERS)
def test_refresh_loop_is_the_composition_of_todays_pieces(arch, T, sampler):
    """Fused loop with every in {2, 3} == the hand loop, torch.equal: plain, inpainting, clip_denoised; tape and Philox noise for
    the noisy samplers; fp32 and fp16; one case with the interval (300, 700) and one with guidance_rescale = 0.7.  The plain
    case differs from the every = 1 loop."""
    df = _df(sampler)
    ran = 0
    for dtype in ("fp32", "fp16"):
        m = _model(arch, dtype)
        today = _loop(df, sampler, _cfg(m), _ys(T)[0], T)
        cases = [("plain", "tape"), ("inpaint", "tape"), ("clip", "tape")] + ([("plain", "philox")] if sampler in NOISY else [])
        for every in (2, 3):
            for variant, rng in cases:
                fused = _loop(df, sampler, _cfg(m), _key(_ys(T, variant)[0], every), T, clip=variant == "clip", rng=rng)
                hand = _hand_loop(df, sampler, m, T, variant, _plan(df, every, sampler), rng)
                tag = (arch, T, sampler, dtype, every, variant, rng)
                assert torch.isfinite(fused).all(), tag
                assert torch.equal(fused, hand), tag
                if variant == "plain" and rng == "tape":
                    assert not torch.equal(fused, today), tag
                ran += 1
        # with the guidance interval: only the guided calls are counted
        plan = _plan(df, 2, sampler, MID)
        assert "off" in plan and "reuse" in plan
        fused = _loop(df, sampler, _cfg(m), _key(_ys(T, "plain", MID)[0], 2), T)
        assert torch.equal(fused, _hand_loop(df, sampler, m, T, "plain", plan)), (arch, T, sampler, dtype, "interval")
        # with the guidance rescale: the unchanged rescale on (c, u')
        fused = _loop(df, sampler, _cfg(m), _key(_ys(T)[0], 2, guidance_rescale=PHI), T)
        hand = _hand_loop(df, sampler, m, T, "plain", _plan(df, 2, sampler), phi=PHI)
        assert torch.equal(fused, hand), (arch, T, sampler, dtype, "rescale")
        assert not torch.equal(fused, _loop(df, sampler, _cfg(m), _key(_ys(T)[0], 2), T))
        ran += 2
    assert ran == 2 * ((8 if sampler in NOISY else 6) + 2)


# ------------------------------------------------------------------------------------------------- 4. passes actually skipped
@pytest.mark.parametrize("arch,T", [("mdm", 20), ("mdm", 10), ("mdm_old", 12)])
@pytest.mark.parametrize("sampler", SAMPLERS)
def test_reuse_calls_skip_the_unconditional_pass(arch, T, sampler):
    """gdx_forward_samples around a fused 10-step loop advances by the sum over guidance_plan of 2B (refresh) or B (reuse, off),
    for every in {2, 4}, without and with the interval; PLMS makes 11 calls."""
    m = _model(arch, "fp32")
    df = _df(sampler)
    eng = m._get_engine(dev())
    for every in (2, 4):
        for interval in (None, MID):
            plan = df.guidance_plan(interval, every, plms=sampler == "plms")
            assert plan == _plan(df, every, sampler, interval) and len(plan) == (11 if sampler == "plms" else 10)
            want = sum(2 * B if what == "refresh" else B for what in plan)
            assert plan.count("reuse") > 0 and want < 2 * B * len(plan)
            before = eng.forward_samples()
            r = _loop(df, sampler, _cfg(m), _key(_ys(T, interval=interval)[0], every), T)
            got = eng.forward_samples() - before
            assert got == want, (every, interval, got, want)
            assert torch.isfinite(r).all()


# ------------------------------------------------------------------------------------------------------- 5. block-wise issue
def _engine_loop(df, sampler, m, T, every, blocks):
    """The sampler's in-library loop at the engine level, issued as blocks [(first executed step, steps or 0 = the rest), ...]
    after one loop setup; Philox noise for "p"."""
    from gesturediffusion_amd._lib import GDX_SAMPLER_DDIM, GDX_SAMPLER_P
    d = dev()
    tape = _inputs(T)[1]["tape"]
    x, eng, mode, scale, mask, motion = df._fused_setup(_cfg(m), tape[0], {"y": _key(_ys(T)[0], every)})
    tmap, n = df._timestep_map(), df.num_timesteps
    hist = torch.zeros((2, *x.shape), device=d, dtype=torch.float32)   # zeros: a loop entered midway reads finite history
    scratch = torch.zeros_like(x)
    for k, nb in blocks:
        kw = dict(scale=scale, run_steps=nb, k_base=k)
        if sampler == "p":
            eng.sample_loop(x, GDX_SAMPLER_P, mode, df.coef_table(GDX_SAMPLER_P, d, 0.0), tmap, n - 1 - k, philox_seed=SEED, **kw)
        elif sampler == "plms":
            eng.plms_loop(x, mode, 2, df.coef_table(GDX_SAMPLER_DDIM, d, 0.0), tmap, n - 1 - k, hist, scratch, **kw)
        else:
            eng.dpm_loop(x, mode, 2, df.dpm_coef_table(d), tmap, n - 1 - k, hist, **kw)
    return x, eng


@pytest.mark.parametrize("arch,T", [("mdm", 20), ("mdm_old", 12)])
@pytest.mark.parametrize("sampler", ["dpmpp", "plms", "p"])
def test_blocks_give_the_bits_of_one_call(arch, T, sampler):
    """run_steps = 3, then the rest with k_base = 3 == one call, every in {2, 3}: the second block starts with a reuse
    (every = 2: calls 9 R, 8 U, 7 R | 6 U; PLMS: 9 R, 8 U, 8 R, 7 U | 6 R) or inside a run of reuses (every = 3)."""
    m = _model(arch, "fp32")
    df = _df(sampler)
    today, _ = _engine_loop(df, sampler, m, T, 1, [(0, 0)])
    for every in (2, 3):
        one, _ = _engine_loop(df, sampler, m, T, every, [(0, 0)])
        assert not torch.equal(one, today), (sampler, every)
        two, _ = _engine_loop(df, sampler, m, T, every, [(0, 3), (3, 0)])
        three, _ = _engine_loop(df, sampler, m, T, every, [(0, 3), (3, 4), (7, 3)])
        assert torch.isfinite(one).all()
        assert torch.equal(one, two) and torch.equal(one, three), (sampler, every)
        if sampler != "p":                                      # x_T is the tape's entry 0: the fused method gives the same
            assert torch.equal(one, _loop(df, sampler, _cfg(m), _key(_ys(T)[0], every), T)), (sampler, every)


@pytest.mark.parametrize("sampler", ["dpmpp", "plms", "p"])
def test_a_block_that_starts_with_a_reuse_needs_the_stored_difference(sampler):
    """After a fresh loop setup a block whose first guided call is a reuse is refused: the message says what a block-wise call
    must continue, nothing ran (the sample counter stands, the state keeps its bits), and the handle works afterwards."""
    from gesturediffusion_amd.engine import GdxError
    m = _model("mdm", "fp32")
    df = _df(sampler)
    T = 20
    eng = m._get_engine(dev())
    whole, _ = _engine_loop(df, sampler, m, T, 2, [(0, 0)])            # leaves a stored difference: the next setup must clear it
    before = eng.forward_samples()
    x0 = _inputs(T)[1]["tape"][0].clone()
    with pytest.raises(GdxError, match="must continue the loop that stored the difference"):
        _engine_loop(df, sampler, m, T, 2, [(2 if sampler == "plms" else 3, 0)])      # call n = 3 (PLMS: 9, 8, 8 | 7)
    assert eng.forward_samples() == before
    assert torch.equal(_inputs(T)[1]["tape"][0], x0)
    again, _ = _engine_loop(df, sampler, m, T, 2, [(0, 0)])
    assert torch.equal(again, whole)
    # a block that starts on a refresh needs nothing stored (every = 2: executed step 2 / PLMS 3 is call n = 2 / 4)
    part, _ = _engine_loop(df, sampler, m, T, 2, [(3 if sampler == "plms" else 2, 0)])
    assert torch.isfinite(part).all()


# ------------------------------------------------------------------------------------------- 6. against the CPU restatement
@functools.lru_cache(maxsize=None)
def _oracle(arch, T, sampler, every):
    """The restatement's final sample for every = 1, 2 or None (the unguided loop), computed once and shared."""
    host, _ = _inputs(T)
    p = weights_from(load_golden(f"loops_{arch}_tiny.npz"))
    cfg = dict(TINY, arch=arch)
    y = {"seed": host["seed"], "mfcc": host["mfcc"], "scale": host["scale"]}
    if sampler == "dpmpp":
        tmap = diffusion("linear", "logsnr10").timestep_map
        out, calls = FR.dpm_loop(p, cfg, every, "linear", tmap, host["tape"][0], y, 2)
        out = torch.from_numpy(out)
    else:
        out, calls = FR.sample_loop(p, cfg, every, "cosine", "ddim10", host["tape"], y, sampler,
                                    eta=DDIM_ETA if sampler == "ddim" else 0.0)
    assert calls == (["off"] * 10 if every is None else FR.plan([True] * 10, every))
    return out


@pytest.mark.parametrize("arch,T", [("mdm", 20), ("mdm", 10), ("mdm_old", 12), ("mdm_old", 10)])
@pytest.mark.parametrize("sampler", ["p", "ddim", "dpmpp"])
def test_refresh_loop_vs_cpu_restatement(arch, T, sampler):
    """every = 2 against the CPU restatement (oracle forwards, oracle loops / the fp64 DPM recurrence, its own counter): fp32
    within the suite's LOOP_TOL, fp16 / bf16 within numerics.stated_tolerance for the worse scale.  And on the restatement
    alone: the deviation of every = 2 from every = 1 is below half the deviation of the unguided loop from every = 1 -- a wrong
    sign or a stale difference would not be."""
    from gesturediffusion_amd.numerics import guidance_factor, stated_tolerance
    want, full, none = (_oracle(arch, T, sampler, e).double() for e in (2, 1, None))
    top = float(full.abs().max())
    dev2, dev0 = float((want - full).abs().max()) / top, float((none - full).abs().max()) / top
    print(f"{arch} T={T} {sampler}: restatement deviation from every=1: every=2 {dev2:.3e}, unguided {dev0:.3e}")
    assert dev2 < 0.5 * dev0, (dev2, dev0)
    worst = max(SCALES, key=guidance_factor)
    for dtype in ("fp32", "fp16", "bf16"):
        tol = LOOP_TOL if dtype == "fp32" else stated_tolerance(dtype, worst)
        got = _loop(_df(sampler), sampler, _cfg(_model(arch, dtype)), _key(_ys(T)[0], 2), T)
        err = rel_err(got.cpu(), _oracle(arch, T, sampler, 2))
        print(f"{arch} T={T} {sampler} {dtype}: rel err vs the restatement {err:.3e} (tolerance {tol:.1e})")
        assert err < tol, (dtype, err)


# ------------------------------------------------------------------------------------------------------------ 7. graph replay
@pytest.mark.parametrize("arch", ["mdm", "mdm_old"])
def test_graph_replay_with_a_refresh_equals_eager(arch):
    """Graph replay on with every = 2: such a call runs eagerly, so the result and the sample count are the eager ones; and a
    loop without the key afterwards replays its graph and is today's loop."""
    m = _model(arch, "fp32")
    eng = m._get_engine(dev())
    T = 20
    for sampler in ("p", "ddim"):
        df = _df(sampler)
        y2, y0 = _key(_ys(T)[0], 2), _ys(T)[0]
        before = eng.forward_samples()
        eager = _loop(df, sampler, _cfg(m), y2, T)
        ran = eng.forward_samples() - before
        today = _loop(df, sampler, _cfg(m), y0, T)
        eng.set_graph_replay(True)
        try:
            before = eng.forward_samples()
            assert torch.equal(_loop(df, sampler, _cfg(m), y2, T), eager), sampler
            assert eng.forward_samples() - before == ran == 5 * 2 * B + 5 * B, sampler
            assert torch.equal(_loop(df, sampler, _cfg(m), y0, T), today), sampler
        finally:
            eng.set_graph_replay(False)


# -------------------------------------------------------------------------------------------------------- 8. workspace guards
@pytest.mark.parametrize("arch,T", [("mdm", 20), ("mdm", 10), ("mdm_old", 12)])
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_refresh_loop_leaves_the_workspace_guards_intact(arch, T, dtype):
    """gdx_set_guards re-prepares the workspace, so the difference buffer is allocated afresh -- with its own canary zone -- by
    the first loop below; no canary byte changes, and the results are those without guards."""
    m = _model(arch, dtype)
    d = dev()
    eng = m._get_engine(d)
    before = eng.forward_samples()
    plain = {s: _loop(_df(s), s, _cfg(m), _key(_ys(T)[0], 2), T) for s in SAMPLERS}
    assert eng.forward_samples() - before == 4 * (5 * 2 * B + 5 * B) + (6 * 2 * B + 5 * B)       # the key is at work: reuses ran
    eng.set_guards(True)
    try:
        for sampler in SAMPLERS:
            for y in (_key(_ys(T)[0], 2), _key(_ys(T, interval=MID)[0], 2, guidance_rescale=PHI)):
                r = _loop(_df(sampler), sampler, _cfg(m), y, T)
                bad, zone = eng.check_guards(d)
                assert bad == 0, f"{sampler}: {bad} canary bytes overwritten, first in workspace allocation #{zone}"
                assert torch.isfinite(r).all()
                if "guidance_rescale" not in y:
                    assert torch.equal(r, plain[sampler]), sampler
    finally:
        eng.set_guards(False)


# ------------------------------------------------------------------------------------------- 9. refusals on the GPU path
def test_paths_without_memory_refuse_on_the_gpu():
    """The guided model's step-wise forward, fused=False and calc_bpd_loop raise ValueError with k = 2; with k = 1 they pass and
    keep the bits of the call without the key."""
    m = _model("mdm", "fp32")
    d = dev()
    T = 20
    _, i = _inputs(T)
    x = i["tape"][3]
    t = torch.tensor([100, 600], device=d)
    y0 = _ys(T)[0]
    with pytest.raises(ValueError, match="in-library loop"):
        _cfg(m)(x, t, y=_key(y0, 2))
    assert torch.equal(_cfg(m)(x, t, y=_key(y0, 1)), _cfg(m)(x, t, y=y0))
    for sampler in SAMPLERS:
        df = _df(sampler)
        with pytest.raises(ValueError, match="in-library loop"):
            _loop(df, sampler, _cfg(m), _key(y0, 2), T, fused=False)
        assert torch.equal(_loop(df, sampler, _cfg(m), _key(y0, 1), T, fused=False), _loop(df, sampler, _cfg(m), y0, T, fused=False))
    df = _df("p")
    kw = dict(clip_denoised=True, noise_tape=i["tape"][:10].contiguous())
    for fused in (True, False):
        with pytest.raises(ValueError, match="in-library loop"):
            df.calc_bpd_loop(_cfg(m), i["x_start"], model_kwargs={"y": _key(y0, 2)}, fused=fused, **kw)
    one = df.calc_bpd_loop(_cfg(m), i["x_start"], model_kwargs={"y": _key(y0, 1)}, **kw)
    none = df.calc_bpd_loop(_cfg(m), i["x_start"], model_kwargs={"y": y0}, **kw)
    for k in ("total_bpd", "prior_bpd", "vb", "xstart_mse", "mse"):
        assert torch.equal(one[k], none[k]), k
    # the key on a model that runs no guidance, and a malformed key, in the fused loops
    for sampler in SAMPLERS:
        with pytest.raises(ValueError, match="ClassifierFreeSampleModel"):
            _loop(_df(sampler), sampler, m, dict(_ys(T)[1], guidance_refresh=2), T)
        for bad in (0, 2.0, True, torch.tensor(2)):
            with pytest.raises(ValueError, match="guidance_refresh"):
                _loop(_df(sampler), sampler, _cfg(m), _key(y0, bad), T)


# -------------------------------------------------------------------------------------------------------------------- 10. CLI
def test_generate_cli_with_a_refresh_equals_a_direct_call(tmp_path, capsys):
    """`sample.generate --synthetic --guidance_refresh 2 --sampler dpmpp --timestep_respacing logsnr10 --chunks 2` at a small
    width: both chunks equal a direct sample_chunks call on the inputs the CLI builds from its seed (each chunk its own loop),
    the plan line is printed with the plan's counts, and the result is not the one without the flag."""
    import re
    from gesturediffusion_amd.sample import generate
    from gesturediffusion_amd.utils.init import MFCC_DIM, init_state_dict
    from gesturediffusion_amd.utils.model_util import create_model_and_diffusion
    from gesturediffusion_amd.utils.parser_util import generate_args
    out = tmp_path / "out"
    argv = ["--synthetic", "--guidance_refresh", "2", "--sampler", "dpmpp", "--timestep_respacing", "logsnr10",
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
    said = re.search(r"### unconditional pass on (\d+) of (\d+) guided calls", printed)
    plan = FR.plan(df.guided_steps(None), 2)                 # the CLI's schedule keeps n timesteps: n calls, all guided
    n_ref, n_calls = plan.count("refresh"), len(plan)
    assert n_calls == df.num_timesteps >= 8 and n_ref == (n_calls + 1) // 2 and plan == df.guidance_plan(None, 2)
    assert said and (int(said.group(1)), int(said.group(2))) == (n_ref, n_calls)
    cfg = dict(arch="mdm", njoints=37, nfeats=1, latent_dim=128, ff_size=1024, num_layers=2, num_heads=4, seed_poses=args.seed_poses)
    model.load_state_dict(init_state_dict(cfg, seed=7), strict=False)
    model = _cfg(model).to(d).eval()
    gen = torch.Generator().manual_seed(7)
    seedp = torch.randn(3, 37, 1, args.seed_poses, generator=gen).to(d)
    mfcc = lambda chunk: torch.randn(3, MFCC_DIM, 1, 20, generator=gen).to(d)   # noqa: E731
    kw = dict(guidance_param=args.guidance_param, sampler="dpmpp", rng="philox", philox_seed=7, dpm_order=2)
    eng = model.model._get_engine(d)
    before = eng.forward_samples()
    want = generate.sample_chunks(model, df, seedp, mfcc, 2, 20, args.seed_poses, guidance_refresh=2, **kw)
    assert eng.forward_samples() - before == 2 * (n_ref * 6 + (n_calls - n_ref) * 3)     # per chunk: refreshes run 2 * 3 samples
    assert np.array_equal(res["motion"], torch.cat(want, dim=3).cpu().numpy())
    gen.manual_seed(7)
    torch.randn(3, 37, 1, args.seed_poses, generator=gen)
    plain = generate.sample_chunks(model, df, seedp, mfcc, 2, 20, args.seed_poses, **kw)
    assert not np.array_equal(res["motion"], torch.cat(plain, dim=3).cpu().numpy())
