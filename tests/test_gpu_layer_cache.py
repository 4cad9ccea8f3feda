"""Layer cache on the GPU (y['layer_cache'], gdx_set_layer_cache, gdx_layer_delta, gdx_forward_layer_samples, tap L + 1;
include/gdx.h): the stand-alone pass against torch, no key / every = 1 against today's loops, full and partial calls through the
taps bit for bit, the encoder layers actually skipped, the same bits along every route, the CPU restatement, workspace guards,
every feature with late workspace on a handle prepared for another shape and back, and the CLI.

Loops: the TINY model (L = 2, so keep = 1; golden weights), inputs, samplers and schedules of test_gpu_guidance_interval.py
(B = 2, scales (2.5, -1.0), 10 steps), plus UniPC on the DPM schedule, and a 4-layer variant of TINY (keep in {1, 2, 3})
initialised by utils/init.py under a fixed seed.  T = 20 takes gdx_sample_loop's token-major path, T = 10 / 12 the others."""
import functools
import math
import re

import numpy as np
import pytest
import torch

import layer_cache_restatement as LR
from conftest import load_golden, rel_err, weights_from
from test_dpm_host import diffusion
from test_gpu_guidance_interval import DDIM_ETA, MID, SAMPLERS, SCALES, SEED, _cfg, _df, _inputs, _loop, _model, _ys
from test_gpu_parity import LOOP_TOL, TINY, build_model, dev

pytestmark = pytest.mark.gpu
B = 2
TINY4 = dict(TINY, num_layers=4)
LOOPS = SAMPLERS + ["unipc"]
SHAPES3 = [("mdm", 20), ("mdm", 10), ("mdm_old", 12), ("mdm_old", 10)]
PAIRS = {"fp32": (torch.float32, torch.float32), "fp16": (torch.float16, torch.float16), "bf16": (torch.float32, torch.bfloat16)}
GDX_COND = 0


@functools.lru_cache(maxsize=None)
def _weights4(arch):
    from gesturediffusion_amd.utils.init import init_state_dict
    return init_state_dict(dict(TINY4, arch=arch), seed=4, perturb=True)


@functools.lru_cache(maxsize=None)
def _model4(arch, dtype):
    m = build_model(arch, TINY4, _weights4(arch))
    m.compute_dtype = dtype
    return m


def _key(y, every=2, keep=1, **more):
    return dict(y, layer_cache=(every, keep), **more)


def _run(sampler, model, y, T, **kw):
    """The sampler's whole-loop method on the shared inputs (test_gpu_guidance_interval._loop, plus UniPC)."""
    if sampler != "unipc":
        return _loop(_df(sampler), sampler, model, y, T, **kw)
    tape = _inputs(T)[1]["tape"]
    return _df("dpmpp").unipc_sample_loop(model, tuple(tape.shape[1:]), order=2, noise=tape[0].clone(), clip_denoised=False,
                                          model_kwargs={"y": y}, fused=kw.get("fused", True))


def _dfx(sampler):
    return _df("dpmpp" if sampler == "unipc" else sampler)


def _want_layers(df, sampler, every, keep, L, guided=True, interval=None, refresh=1):
    """(samples x layers, full calls, calls) of a loop from the restatement's own counter."""
    modes = LR.modes_of(df.guided_steps(interval), refresh, guided, plms=sampler == "plms")
    plan = LR.plan(modes, every)
    width = {LR.CFG: 2 * B, LR.COND: B}
    return sum(width[c] * (L if what == "full" else keep) for c, what in zip(modes, plan)), plan.count("full"), len(plan)


# ---------------------------------------------------------------------------------------------- 1. gdx_layer_delta against torch
@pytest.mark.parametrize("pairing", ["fp32", "fp16", "bf16"])
def test_layer_delta_against_torch(pairing):
    """store == torch.sub on the remapped rows, apply == (in + delta) rounded to the operand's type, bit for bit, for batch in
    {1, 3}, frames in {1, 10, 33}, width in {32, 128, 192} (33 x 192 x 3 / 8 octets: more than one block).  NaN sentinels in
    front of and behind the written operand survive, and so do NaNs in the token-0 rows of `in`, which never reach the output."""
    from gesturediffusion_amd import engine as E
    d = dev()
    ti, to = PAIRS[pairing]
    pad = 64
    for batch in (1, 3):
        for frames in (1, 10, 33):
            for width in (32, 128, 192):
                tag = (pairing, batch, frames, width)
                g = torch.Generator().manual_seed(batch * 10000 + frames * 100 + width)
                inp = (torch.randn(batch, frames + 1, width, generator=g) * 2).to(ti).to(d)
                inp[:, 0, :] = math.nan
                inp_bits = inp.clone()
                outc_h = torch.randn(batch, frames, width, generator=g).to(to)
                n = batch * frames * width
                # store
                buf = torch.full((pad + n + pad,), math.nan, device=d, dtype=torch.float32)
                delta = buf[pad:pad + n].view(batch, frames, width)
                outc = outc_h.to(d)
                E.Engine.layer_delta(0, inp, outc, delta)
                want = torch.sub(outc.float(), inp[:, 1:].float())
                assert torch.equal(delta, want) and torch.isfinite(delta).all(), tag
                assert bool(torch.isnan(buf[:pad]).all()) and bool(torch.isnan(buf[pad + n:]).all()), tag
                assert torch.equal(outc.cpu(), outc_h), tag                                     # the read operand is untouched
                # apply
                obuf = torch.full((pad + n + pad,), math.nan, device=d, dtype=to)
                out2 = obuf[pad:pad + n].view(batch, frames, width)
                dl = want.clone()
                E.Engine.layer_delta(1, inp, out2, dl)
                want2 = (inp[:, 1:].float() + want).to(to)
                assert torch.equal(out2, want2) and torch.isfinite(out2.float()).all(), tag
                assert bool(torch.isnan(obuf[:pad]).all()) and bool(torch.isnan(obuf[pad + n:]).all()), tag
                assert torch.equal(dl, want), tag
                assert torch.equal(inp.view(torch.int32 if ti == torch.float32 else torch.int16),
                                   inp_bits.view(torch.int32 if ti == torch.float32 else torch.int16)), tag


def test_layer_delta_refusals():
    """Every refusal of the stand-alone entry, on real device operands: nothing is written."""
    from gesturediffusion_amd import engine as E
    from gesturediffusion_amd.engine import GdxError
    d = dev()
    mk = lambda dt, *s: torch.zeros(*s, device=d, dtype=dt)      # noqa: E731
    f32, f16, bf16 = torch.float32, torch.float16, torch.bfloat16
    sent = torch.full((2, 10, 128), math.nan, device=d)
    for ti, to in ((f16, f32), (f32, f16), (f16, bf16), (bf16, bf16), (bf16, f32)):
        with pytest.raises(GdxError, match=r"\(fp32, fp32\), \(fp16, fp16\) or \(fp32, bf16\)"):
            E.layer_delta(0, mk(ti, 2, 11, 128), mk(to, 2, 10, 128), sent)
    for op in (-1, 2):
        with pytest.raises(GdxError, match="op must be 0"):
            E.layer_delta(op, mk(f32, 2, 11, 128), mk(f32, 2, 10, 128), sent)
    for width in (48, 16, 100):
        with pytest.raises(GdxError, match="multiple of 32"):
            E.layer_delta(0, mk(f32, 2, 11, width), mk(f32, 2, 10, width), sent)
    flat = torch.zeros(2 * 11 * 128 + 8, device=d)
    off = flat[1:1 + 2 * 11 * 128].view(2, 11, 128)                                    # one float off alignment
    with pytest.raises(GdxError, match="16-byte aligned"):
        E.layer_delta(0, off, mk(f32, 2, 10, 128), sent)
    with pytest.raises(GdxError, match="16-byte aligned"):
        E.layer_delta(1, mk(f32, 2, 11, 128), off[:, :10], sent)
    with pytest.raises(GdxError, match="must be positive"):
        E.layer_delta(0, mk(f32, 2, 1, 128), mk(f32, 2, 0, 128), sent)
    assert bool(torch.isnan(sent).all())


# ------------------------------------------------------------------------------------------------------ 2. off is today's loop
@pytest.mark.parametrize("arch,T", [("mdm", 20), ("mdm", 10), ("mdm_old", 12)])
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_every_one_is_todays_loop(arch, T, dtype):
    """No key == (1, anything), bit for bit, with gdx_forward_samples and gdx_forward_layer_samples advancing alike (every call
    runs L layers); and a call without the key after one with (2, 1) on the same engine is today's loop again."""
    m = _model(arch, dtype)
    eng = m._get_engine(dev())
    L = TINY["num_layers"]
    y0 = _ys(T)[0]
    for sampler in LOOPS:
        s0, l0 = eng.forward_samples(), eng.forward_layer_samples()
        today = _run(sampler, _cfg(m), y0, T)
        ran, layers = eng.forward_samples() - s0, eng.forward_layer_samples() - l0
        assert ran == 2 * B * (11 if sampler == "plms" else 10) and layers == ran * L
        for keep in (1, 0, 99):
            s0, l0 = eng.forward_samples(), eng.forward_layer_samples()
            assert torch.equal(_run(sampler, _cfg(m), _key(y0, 1, keep), T), today), (sampler, keep)
            assert (eng.forward_samples() - s0, eng.forward_layer_samples() - l0) == (ran, layers), (sampler, keep)
        s0, l0 = eng.forward_samples(), eng.forward_layer_samples()
        cached = _run(sampler, _cfg(m), _key(y0, 2, 1), T)
        assert torch.isfinite(cached).all() and not torch.equal(cached, today), sampler
        assert eng.forward_samples() - s0 == ran and eng.forward_layer_samples() - l0 < layers, sampler
        s0, l0 = eng.forward_samples(), eng.forward_layer_samples()
        assert torch.equal(_run(sampler, _cfg(m), y0, T), today), (sampler, "a handle kept its setting")
        assert (eng.forward_samples() - s0, eng.forward_layer_samples() - l0) == (ran, layers), sampler


# ------------------------------------------------------------------------------------- 3. composition, bit for bit, through the taps
def _dpm_steps(df, model, T, y, steps):
    """gdx_dpm_loop on the shared x_T, one call per executed step in `steps` after one loop setup -> (x, engine)."""
    d = dev()
    x, eng, mode, scale, mask, motion = df._fused_setup(model, _inputs(T)[1]["tape"][0], {"y": y})
    hist = torch.zeros((2, *x.shape), device=d, dtype=torch.float32)
    n = df.num_timesteps
    for k in steps:
        eng.dpm_loop(x, mode, 2, df.dpm_coef_table(d), df._timestep_map(), n - 1 - k, hist, scale=scale, run_steps=1, k_base=k)
        yield x, eng


@pytest.mark.parametrize("arch,T", [("mdm", 20), ("mdm_old", 12)])
@pytest.mark.parametrize("dtype", ["fp32", "fp16", "bf16"])
def test_full_and_partial_calls_through_the_taps(arch, T, dtype):
    """keep_taps on, gdx_dpm_loop one step at a time, every = 2, keep in {1, 2, 3} on the 4-layer model, GDX_COND (the inner
    model) and GDX_CFG (both halves).  After the full call tap(L+1) == tap(L) on the compact rows (rounded to the 16-bit type in
    the 16-bit modes) and the sample equals the same call without the key; after the partial call
    tap(L+1) == fl32(s(tap'(keep))[rows] + delta), delta = fl32(tap(L+1) - s(tap(keep))[rows]) from the full call, s the
    identity where the stream is fp32 and a round trip through fp16 in the fp16 mode, rounded likewise.  A partial call launches
    keep layers, leaves taps keep+1 .. L stale, and moves the sample off the uncached one."""
    d = dev()
    m = _model4(arch, dtype)
    L, S, width = 4, T + 1, TINY4["latent_dim"]
    half = {"fp32": None, "fp16": torch.float16, "bf16": torch.bfloat16}[dtype]
    r = (lambda t: t) if half is None else (lambda t: t.to(half).float())               # the operand's rounding
    s = (lambda t: t.half().float()) if dtype == "fp16" else (lambda t: t)               # the stream as the cache reads it
    df = _df("dpmpp")
    eng = m._get_engine(d)
    eng.keep_taps(True)
    try:
        for guided in (False, True):
            model, y0 = (_cfg(m), _ys(T)[0]) if guided else (m, _ys(T)[1])
            Beff = 2 * B if guided else B
            stream = lambda which: eng.tap(which, Beff * S, width, d).view(Beff, S, width)[:, 1:]      # noqa: E731
            operand = lambda: eng.tap(L + 1, Beff * T, width, d).view(Beff, T, width)                   # noqa: E731
            ref = [x.clone() for x, _ in _dpm_steps(df, model, T, y0, (0, 1))]
            for keep in (1, 2, 3):
                tag = (arch, dtype, guided, keep)
                steps = _dpm_steps(df, model, T, _key(y0, 2, keep), (0, 1))
                l0 = eng.forward_layer_samples()
                x, _ = next(steps)                                                      # m = 0: full
                assert eng.forward_layer_samples() - l0 == Beff * L, tag
                assert torch.equal(x, ref[0]), tag
                last, xc, inner = stream(L), operand(), stream(keep)
                assert torch.isfinite(xc).all() and torch.equal(xc, r(last)), tag
                delta = torch.sub(xc, s(inner))
                l0 = eng.forward_layer_samples()
                x, _ = next(steps)                                                      # m = 1: partial
                assert eng.forward_layer_samples() - l0 == Beff * keep, tag
                inner2, xc2 = stream(keep), operand()
                assert not torch.equal(inner2, inner), tag
                assert torch.equal(xc2, r(s(inner2) + delta)), tag
                assert torch.equal(stream(L), last), (tag, "tap L is stale after a partial call")
                assert torch.isfinite(x).all() and not torch.equal(x, ref[1]), tag
                assert next(steps, None) is None
    finally:
        eng.keep_taps(False)


# ----------------------------------------------------------------------------------------------------- 4. skipped work is skipped
@pytest.mark.parametrize("arch,T", [("mdm", 20), ("mdm", 10), ("mdm_old", 12)])
@pytest.mark.parametrize("sampler", LOOPS)
def test_partial_calls_skip_the_deep_layers(arch, T, sampler):
    """Over whole loops gdx_forward_layer_samples rises by sum_full Beff L + sum_partial Beff keep per the restatement's plan and
    gdx_forward_samples as without the key: plain, with the interval (300, 700) (the width changes mid-loop) and with
    guidance_refresh = 2; every in {2, 3}; TINY (keep = 1) and the 4-layer model (keep = 2); the unguided model too."""
    df = _dfx(sampler)
    for m, L, keep in ((_model(arch, "fp32"), 2, 1), (_model4(arch, "fp32"), 4, 2)):
        eng = m._get_engine(dev())
        for every in (2, 3):
            for guided, interval, refresh in ((True, None, 1), (True, MID, 1), (True, None, 2), (True, MID, 2), (False, None, 1)):
                tag = (sampler, L, every, guided, interval, refresh)
                y = _ys(T, interval=interval)[0] if guided else _ys(T)[1]
                if refresh > 1:
                    y = dict(y, guidance_refresh=refresh)
                model = _cfg(m) if guided else m
                s0 = eng.forward_samples()
                _run(sampler, model, y, T)
                plain = eng.forward_samples() - s0
                want, n_full, n_calls = _want_layers(df, sampler, every, keep, L, guided, interval, refresh)
                assert n_calls == (11 if sampler == "plms" else 10) and 0 < n_full < n_calls
                s0, l0 = eng.forward_samples(), eng.forward_layer_samples()
                out = _run(sampler, model, _key(y, every, keep), T)
                got = (eng.forward_samples() - s0, eng.forward_layer_samples() - l0)
                assert got == (plain, want), (tag, got, plain, want)
                assert want < plain * L and torch.isfinite(out).all(), tag
                assert df.layer_cache_plan((every, keep), interval, refresh, guided=guided,
                                           plms=sampler == "plms").count("full") == n_full, tag


# ------------------------------------------------------------------------------------------------ 5. same bits along every route
def _engine_loop(df, sampler, m, T, lc, blocks, **keys):
    """The sampler's in-library loop at the engine level, issued as blocks [(first executed step, steps or 0 = the rest), ...]
    after one loop setup; Philox noise for "p"; keys: further entries of y."""
    from gesturediffusion_amd._lib import GDX_SAMPLER_DDIM, GDX_SAMPLER_P
    d = dev()
    tape = _inputs(T)[1]["tape"]
    x, eng, mode, scale, mask, motion = df._fused_setup(_cfg(m), tape[0], {"y": _key(_ys(T)[0], *lc, **keys)})
    tmap, n = df._timestep_map(), df.num_timesteps
    hist = torch.zeros((3, *x.shape), device=d, dtype=torch.float32)   # zeros: a loop entered midway reads finite history
    scratch, base = torch.zeros_like(x), torch.zeros_like(x)
    for k, nb in blocks:
        kw = dict(scale=scale, run_steps=nb, k_base=k)
        if sampler == "p":
            eng.sample_loop(x, GDX_SAMPLER_P, mode, df.coef_table(GDX_SAMPLER_P, d, 0.0), tmap, n - 1 - k, philox_seed=SEED, **kw)
        elif sampler == "plms":
            eng.plms_loop(x, mode, 2, df.coef_table(GDX_SAMPLER_DDIM, d, 0.0), tmap, n - 1 - k, hist, scratch, **kw)
        elif sampler == "unipc":
            coef, coef_c = df.unipc_coef_tables(d)
            eng.unipc_loop(x, mode, 2, coef, coef_c, tmap, n - 1 - k, hist, base, **kw)
        else:
            eng.dpm_loop(x, mode, 2, df.dpm_coef_table(d), tmap, n - 1 - k, hist, **kw)
    return x, eng


@pytest.mark.parametrize("arch,T", [("mdm", 20), ("mdm_old", 12)])
@pytest.mark.parametrize("sampler", ["dpmpp", "plms", "p", "unipc"])
def test_blocks_give_the_bits_of_one_call(arch, T, sampler):
    """run_steps = 3, then the rest with k_base = 3 == one call == three blocks, for (2, 1) and (3, 1): the later blocks start
    with a partial call ((2, 1): calls F P F | P; PLMS: F P F P | F) or inside a run of partial calls.  And (3, 1) under the
    interval (300, 700) with guidance_refresh = 2, where the three numberings meet: the second block starts on a reuse."""
    m = _model(arch, "fp32")
    df = _dfx(sampler)
    today, _ = _engine_loop(df, sampler, m, T, (1, 0), [(0, 0)])
    for lc, keys in (((2, 1), {}), ((3, 1), {}), ((3, 1), dict(guidance_interval=MID, guidance_refresh=2))):
        one, _ = _engine_loop(df, sampler, m, T, lc, [(0, 0)], **keys)
        assert torch.isfinite(one).all() and not torch.equal(one, today), (sampler, lc, keys)
        two, _ = _engine_loop(df, sampler, m, T, lc, [(0, 3), (3, 0)], **keys)
        three, _ = _engine_loop(df, sampler, m, T, lc, [(0, 3), (3, 4), (7, 3)], **keys)
        assert torch.equal(one, two) and torch.equal(one, three), (sampler, lc, keys)
        if sampler != "p":                                      # x_T is the tape's entry 0: the fused method gives the same
            assert torch.equal(one, _run(sampler, _cfg(m), _key(_ys(T)[0], *lc, **keys), T)), (sampler, lc, keys)


@pytest.mark.parametrize("arch", ["mdm", "mdm_old"])
def test_torch_noise_blocks_give_the_bits_of_one_call(arch, monkeypatch):
    """rng="torch": the loop is issued in blocks of pre-drawn noise; blocks of 3 steps give the bits of one block of 10."""
    from gesturediffusion_amd.diffusion import gaussian_diffusion as gd
    m = _model(arch, "fp32")
    T = 20
    shape = tuple(_inputs(T)[1]["tape"].shape[1:])
    for sampler, df in (("p", _df("p")), ("dpmpp_sde", _df("dpmpp_sde"))):
        loop = df.p_sample_loop if sampler == "p" else functools.partial(df.dpm_solver_sde_sample_loop, order=2, eta=1.0)
        outs = []
        for block in (50, 3):
            monkeypatch.setattr(gd, "NOISE_BLOCK", block)
            torch.manual_seed(SEED)
            outs.append(loop(_cfg(m), shape, clip_denoised=False, model_kwargs={"y": _key(_ys(T)[0], 2, 1)}, rng="torch"))
        monkeypatch.undo()
        assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1]), sampler


@pytest.mark.parametrize("sampler", ["dpmpp", "plms", "p", "unipc"])
def test_a_block_that_starts_with_a_partial_call_needs_the_stored_change(sampler):
    """After a fresh loop setup a block whose first call is partial is refused: the message names the loop and says what a
    block-wise call must continue, nothing ran (the counters stand), and the handle works afterwards."""
    from gesturediffusion_amd.engine import GdxError
    m = _model("mdm", "fp32")
    df = _dfx(sampler)
    T = 20
    eng = m._get_engine(dev())
    whole, _ = _engine_loop(df, sampler, m, T, (2, 1), [(0, 0)])       # leaves a stored change: the next setup must clear it
    before = (eng.forward_samples(), eng.forward_layer_samples())
    entry = {"dpmpp": "gdx_dpm_loop", "plms": "gdx_plms_loop", "p": "gdx_sample_loop", "unipc": "gdx_unipc_loop"}[sampler]
    with pytest.raises(GdxError, match=entry + ".*must continue the loop that stored the change"):
        _engine_loop(df, sampler, m, T, (2, 1), [(2 if sampler == "plms" else 3, 0)])     # call m = 3 (PLMS: 9, 8, 8 | 7)
    assert (eng.forward_samples(), eng.forward_layer_samples()) == before
    again, _ = _engine_loop(df, sampler, m, T, (2, 1), [(0, 0)])
    assert torch.equal(again, whole)
    # a block that starts on a full call needs nothing stored (executed step 2 / PLMS 3 is call m = 2 / 4)
    part, _ = _engine_loop(df, sampler, m, T, (2, 1), [(3 if sampler == "plms" else 2, 0)])
    assert torch.isfinite(part).all()


@pytest.mark.parametrize("arch", ["mdm", "mdm_old"])
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_token_major_and_pose_layout_paths_give_the_same_bits(arch, dtype):
    """T = 20 without inpainting takes gdx_sample_loop's token-major path; with the taps kept the same loop takes the
    pose-layout path.  Same bits, same layer count, for the ancestral and the DDIM loop, unguided model included."""
    m = _model(arch, dtype)
    eng = m._get_engine(dev())
    T = 20
    for sampler in ("p", "ddim"):
        for model, y in ((_cfg(m), _ys(T, interval=MID)[0]), (m, _ys(T)[1])):
            l0 = eng.forward_layer_samples()
            fast = _run(sampler, model, _key(y, 2, 1), T)
            layers = eng.forward_layer_samples() - l0
            eng.keep_taps(True)
            try:
                l0 = eng.forward_layer_samples()
                slow = _run(sampler, model, _key(y, 2, 1), T)
                assert eng.forward_layer_samples() - l0 == layers
            finally:
                eng.keep_taps(False)
            assert torch.isfinite(fast).all() and torch.equal(fast, slow), (sampler, model is m)
            assert not torch.equal(fast, _run(sampler, model, y, T)), sampler


@pytest.mark.parametrize("arch", ["mdm", "mdm_old"])
def test_graph_replay_with_the_cache_equals_eager(arch):
    """Graph replay on with (2, 1): such a call runs eagerly, so the result and the counters are the eager ones; and a loop
    without the key afterwards replays its graph and is today's loop."""
    m = _model(arch, "fp32")
    eng = m._get_engine(dev())
    T = 10                                                             # the pose-layout path, where graph replay applies
    for sampler in ("p", "ddim"):
        y2, y0 = _key(_ys(T)[0], 2, 1), _ys(T)[0]
        l0 = eng.forward_layer_samples()
        eager = _run(sampler, _cfg(m), y2, T)
        layers = eng.forward_layer_samples() - l0
        today = _run(sampler, _cfg(m), y0, T)
        eng.set_graph_replay(True)
        try:
            l0 = eng.forward_layer_samples()
            assert torch.equal(_run(sampler, _cfg(m), y2, T), eager), sampler
            assert eng.forward_layer_samples() - l0 == layers == 5 * 2 * B * 2 + 5 * 2 * B * 1, sampler
            assert torch.equal(_run(sampler, _cfg(m), y0, T), today), sampler
        finally:
            eng.set_graph_replay(False)


def test_paths_without_memory_refuse_on_the_gpu():
    """The step-wise forwards, fused=False, calc_bpd_loop and the inversion raise ValueError with (2, 1); with (1, 1) they pass
    and keep the bits of the call without the key; a malformed key is a ValueError in the fused loops."""
    m = _model("mdm", "fp32")
    d = dev()
    T = 20
    _, i = _inputs(T)
    x = i["tape"][3]
    t = torch.tensor([100, 600], device=d)
    y0, y_in = _ys(T)
    for model, y in ((_cfg(m), y0), (m, y_in), (_model("mdm_old", "fp32"), y_in)):
        with pytest.raises(ValueError, match="in-library loop"):
            model(x, t, y=_key(y, 2, 1))
        assert torch.equal(model(x, t, y=_key(y, 1, 1)), model(x, t, y=y))
    for sampler in LOOPS:
        with pytest.raises(ValueError, match="in-library loop"):
            _run(sampler, _cfg(m), _key(y0, 2, 1), T, fused=False)
        assert torch.equal(_run(sampler, _cfg(m), _key(y0, 1, 1), T, fused=False), _run(sampler, _cfg(m), y0, T, fused=False))
        for bad in ((2, 2), (2, 0), (0, 1), (2.0, 1), (True, 1), 2, torch.tensor([2, 1])):
            with pytest.raises(ValueError, match="layer_cache"):
                _run(sampler, _cfg(m), dict(y0, layer_cache=bad), T)
    df = _df("p")
    kw = dict(clip_denoised=True, noise_tape=i["tape"][:10].contiguous())
    for fused in (True, False):
        with pytest.raises(ValueError, match="in-library loop"):
            df.calc_bpd_loop(_cfg(m), i["x_start"], model_kwargs={"y": _key(y0, 2, 1)}, fused=fused, **kw)
        with pytest.raises(ValueError, match="in-library loop"):
            _df("ddim").ddim_reverse_sample_loop(m, i["x_start"], clip_denoised=False, model_kwargs={"y": _key(y_in, 2, 1)}, fused=fused)
    one = df.calc_bpd_loop(_cfg(m), i["x_start"], model_kwargs={"y": _key(y0, 1, 1)}, **kw)
    none = df.calc_bpd_loop(_cfg(m), i["x_start"], model_kwargs={"y": y0}, **kw)
    for k in ("total_bpd", "prior_bpd", "vb", "xstart_mse", "mse"):
        assert torch.equal(one[k], none[k]), k
    # a handle that a cached loop left with every = 2: gdx_bpd_loop and the inversion keep every call full
    eng = m._get_engine(d)
    _run("ddim", _cfg(m), _key(y0, 2, 1), T)
    eng.set_layer_cache(2, 1)
    l0, s0 = eng.forward_layer_samples(), eng.forward_samples()
    eng.set_condition(i["seed"], i["mfcc"], cache=False)
    x2 = i["x_start"].clone()
    eng.ddim_reverse_loop(x2, GDX_COND, _df("ddim").coef_table(1, d, "reverse"), _df("ddim")._timestep_map(), 0, 4)
    assert eng.forward_layer_samples() - l0 == (eng.forward_samples() - s0) * TINY["num_layers"] == 4 * B * TINY["num_layers"]
    eng.set_layer_cache(1, 0)


# ------------------------------------------------------------------------------------------- 6. against the CPU restatement
@functools.lru_cache(maxsize=None)
def _oracle(arch, T, sampler, every, keep, layers):
    """The restatement's final sample of the guided loop, computed once and shared."""
    host, _ = _inputs(T)
    p = weights_from(load_golden(f"loops_{arch}_tiny.npz")) if layers == 2 else _weights4(arch)
    cfg = dict(TINY if layers == 2 else TINY4, arch=arch)
    y = {"seed": host["seed"], "mfcc": host["mfcc"], "scale": host["scale"]}
    if sampler == "dpmpp":
        tmap = diffusion("linear", "logsnr10").timestep_map
        out, fn = LR.dpm_loop(p, cfg, every, keep, "linear", tmap, host["tape"][0], y, 2)
    else:
        out, fn = LR.sample_loop(p, cfg, every, keep, "cosine", "ddim10", host["tape"], y, sampler,
                                 eta=DDIM_ETA if sampler == "ddim" else 0.0)
    assert fn.calls == LR.plan([LR.CFG] * 10, every)
    return out


@pytest.mark.parametrize("arch,T", SHAPES3)
@pytest.mark.parametrize("sampler", ["p", "ddim", "dpmpp"])
def test_cached_loop_vs_cpu_restatement(arch, T, sampler):
    """(2, 1) on TINY and (2, 2) on the 4-layer model against the CPU restatement (oracle forwards with their per-layer taps,
    oracle loops / the fp64 DPM recurrence, its own counter): fp32 within the suite's LOOP_TOL, fp16 / bf16 within
    numerics.stated_tolerance for the worse scale; where a case exceeds that, within twice the distance of the SAME loop without
    the key from its own restatement (measured here, on the GPU, never from the cached loop).  And on the restatement alone: the
    cached loop is not the uncached one.

    Measured on the MI355X, relative to max|restatement| (worst case over the shapes and samplers of this test; the distance
    of the loop without the key in brackets):
      TINY (2, 1):     fp32 1.68e-06 [1.39e-06]   fp16 1.98e-03 [1.97e-03]   bf16 9.53e-03 [1.00e-02]
      4-layer (2, 2):  fp32 2.47e-06 [1.86e-06]   fp16 2.78e-03 [2.45e-03]   bf16 1.21e-02 [1.01e-02]
    Every case lies within the project's own tolerance (2e-4, 8e-2, 8e-2); the twice-the-uncached allowance was never needed."""
    from gesturediffusion_amd.numerics import guidance_factor, stated_tolerance
    worst = max(SCALES, key=guidance_factor)
    for layers, keep, build in ((2, 1, _model), (4, 2, _model4)):
        want, plain = _oracle(arch, T, sampler, 2, keep, layers), _oracle(arch, T, sampler, 1, keep, layers)
        assert not torch.equal(want, plain)
        for dtype in ("fp32", "fp16", "bf16"):
            tol = LOOP_TOL if dtype == "fp32" else stated_tolerance(dtype, worst)
            m = build(arch, dtype)
            base = rel_err(_run(sampler, _cfg(m), _ys(T)[0], T).cpu(), plain)
            err = rel_err(_run(sampler, _cfg(m), _key(_ys(T)[0], 2, keep), T).cpu(), want)
            print(f"LAYERCACHE {arch} T={T} {sampler} L={layers} {dtype}: rel err vs the restatement {err:.3e} "
                  f"(without the key {base:.3e}, tolerance {tol:.1e})")
            assert err < max(tol, 2 * base), (layers, dtype, err, base, tol)


# -------------------------------------------------------------------------------------------------------- 7. workspace guards
@pytest.mark.parametrize("arch,T", SHAPES3)
@pytest.mark.parametrize("dtype", ["fp32", "fp16", "bf16"])
def test_cached_loops_leave_the_workspace_guards_intact(arch, T, dtype):
    """gdx_set_guards re-prepares the workspace, so the change and the kept stream are allocated afresh -- each with its own
    canary zone -- by the first loop below; no canary byte changes, and the results are those without guards."""
    d = dev()
    for m, keep in ((_model(arch, dtype), 1), (_model4(arch, dtype), 3)):
        eng = m._get_engine(d)
        ys = (_key(_ys(T)[0], 2, keep), _key(_ys(T, interval=MID)[0], 3, keep, guidance_refresh=2))
        plain = {(s, j): _run(s, _cfg(m), y, T) for s in LOOPS for j, y in enumerate(ys)}
        eng.set_guards(True)
        try:
            for sampler in LOOPS:
                for j, y in enumerate(ys):
                    r = _run(sampler, _cfg(m), y, T)
                    bad, zone = eng.check_guards(d)
                    assert bad == 0, f"{sampler}: {bad} canary bytes overwritten, first in workspace allocation #{zone}"
                    assert torch.equal(r, plain[sampler, j]), (sampler, j)
        finally:
            eng.set_guards(False)


# ---------------------------------------------------------------------- 7b. a handle prepared for another shape and back again
def _bpd(model, y, T):
    r = _df("p").calc_bpd_loop(model, _inputs(T)[1]["x_start"], clip_denoised=True, model_kwargs={"y": y}, rng="philox", philox_seed=SEED)
    return torch.stack([r[k] for k in ("vb", "xstart_mse", "mse")])


def _parallel(model, y, T):
    tape = _inputs(T)[1]["tape"]
    return _df("p").parallel_sample_loop(model, tuple(tape.shape[1:]), clip_denoised=False, model_kwargs={"y": y}, window=4,
                                         tolerance=0.0, noise_tape=tape)


# the features whose workspace the handle acquires after gdx_prepare: (the run, its keys in y)
LATE = {"step_tables": (functools.partial(_run, "ddim"), {}),
        "bpd_loop": (_bpd, {}),
        "parallel_loop": (_parallel, {}),
        "guidance_rescale": (functools.partial(_run, "ddim"), dict(guidance_rescale=0.7)),
        "guidance_refresh": (functools.partial(_run, "ddim"), dict(guidance_refresh=2)),
        "layer_cache": (functools.partial(_run, "ddim"), dict(layer_cache=(2, 1)))}


@pytest.mark.parametrize("feature", list(LATE))
def test_a_handle_prepared_for_another_shape_and_back_repeats_its_result(feature):
    """Each feature that owns late workspace (the step tables of a plain gdx_sample_loop, gdx_bpd_loop with Philox noise,
    gdx_parallel_loop at tolerance 0, the guidance rescale, the guidance refresh, the layer cache), guided, on a handle of its own:
    run it, prepare the handle for another (B, T) -- which frees the workspace and with it every late buffer --, run it again (the
    loop prepares the handle back and conditions it again): the bits of the first run, and those of a fresh handle."""
    run, keys = LATE[feature]
    arch, T = "mdm", 20
    y = dict(_ys(T)[0], **keys)

    def fresh():
        m = build_model(arch, TINY, weights_from(load_golden(f"loops_{arch}_tiny.npz")))
        m.compute_dtype = "fp32"
        return m
    m = fresh()
    first = run(_cfg(m), y, T)
    eng = m._get_engine(dev())
    shape = eng.shape
    eng.prepare(3, 30)
    assert shape in ((B, T), (4 * B, T)) and eng.shape == (3, 30)
    again = run(_cfg(m), y, T)
    assert eng.shape == shape
    other = run(_cfg(fresh()), y, T)
    assert torch.isfinite(first).all()
    assert torch.equal(again, first), feature
    assert torch.equal(other, first), feature


# --------------------------------------------------------------------------------------------------------------------- 8. CLI
def test_generate_cli_with_the_cache_equals_a_direct_call(tmp_path, capsys):
    """`sample.generate --synthetic --layer_cache 2 1 --sampler dpmpp --timestep_respacing logsnr10 --chunks 2` at a small
    width: both chunks equal a direct sample_chunks call on the inputs the CLI builds from its seed (each chunk its own loop,
    starting with a full call), the plan line is printed with the plan's counts, the result is not the one without the flag,
    and --invert_gt with the flag is an error."""
    from gesturediffusion_amd.sample import generate
    from gesturediffusion_amd.utils.init import MFCC_DIM, init_state_dict
    from gesturediffusion_amd.utils.model_util import create_model_and_diffusion
    from gesturediffusion_amd.utils.parser_util import generate_args
    out = tmp_path / "out"
    argv = ["--synthetic", "--layer_cache", "2", "1", "--sampler", "dpmpp", "--timestep_respacing", "logsnr10",
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
    said = re.search(r"layer cache: (\d+) full, (\d+) partial calls; (\d+) of (\d+) layers on a partial call", printed)
    plan = LR.plan([LR.CFG] * df.num_timesteps, 2)
    n_full, n_calls = plan.count("full"), len(plan)
    assert n_calls >= 8 and n_full == (n_calls + 1) // 2
    assert said and tuple(int(v) for v in said.groups()) == (n_full, n_calls - n_full, 1, 2)
    cfg = dict(arch="mdm", njoints=37, nfeats=1, latent_dim=128, ff_size=1024, num_layers=2, num_heads=4, seed_poses=args.seed_poses)
    model.load_state_dict(init_state_dict(cfg, seed=7), strict=False)
    model = _cfg(model).to(d).eval()
    gen = torch.Generator().manual_seed(7)
    seedp = torch.randn(3, 37, 1, args.seed_poses, generator=gen).to(d)
    mfcc = lambda chunk: torch.randn(3, MFCC_DIM, 1, 20, generator=gen).to(d)   # noqa: E731
    kw = dict(guidance_param=args.guidance_param, sampler="dpmpp", rng="philox", philox_seed=7, dpm_order=2)
    eng = model.model._get_engine(d)
    l0 = eng.forward_layer_samples()
    want = generate.sample_chunks(model, df, seedp, mfcc, 2, 20, args.seed_poses, layer_cache=(2, 1), **kw)
    assert eng.forward_layer_samples() - l0 == 2 * 6 * (n_full * 2 + (n_calls - n_full) * 1)      # per chunk, 2 * 3 samples a call
    assert np.array_equal(res["motion"], torch.cat(want, dim=3).cpu().numpy())
    gen.manual_seed(7)
    torch.randn(3, 37, 1, args.seed_poses, generator=gen)
    plain = generate.sample_chunks(model, df, seedp, mfcc, 2, 20, args.seed_poses, **kw)
    assert not np.array_equal(res["motion"], torch.cat(plain, dim=3).cpu().numpy())
    with pytest.raises(SystemExit):
        generate.main(["--dataset", "genea2023", "--data_dir", str(tmp_path), "--sampler", "ddim", "--invert_gt", "--layer_cache", "2", "1"])
    assert "--invert_gt runs no layer cache" in capsys.readouterr().err
