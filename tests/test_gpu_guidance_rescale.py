"""Guidance rescale on the GPU (y['guidance_rescale'], gdx_set_guidance_rescale, gdx_cfg_rescale; include/gdx.h): the stand-alone
operation against the fp64 restatement on the shapes where its kernels change path, batch independence and the edge cases, the
fused loops against the step-wise protocol bit for bit, phi = 0 / an absent key against today's loops, the denoiser samples
counted, the CPU restatement of whole loops, calc_bpd_loop, graph replay, workspace guards, the CLI and the refusals.

Loops: the TINY model, inputs, samplers and schedules of test_gpu_guidance_interval.py (B = 2, scales (2.5, -1.0), 10 steps);
phi = 0.7 unless stated."""
import functools
import math

import numpy as np
import pytest
import torch

import guidance_rescale_restatement as RR
from conftest import load_golden, rel_err, weights_from
from misaligned import shifted
from test_dpm_host import diffusion
from test_gpu_guidance_interval import (ALL, DDIM_ETA, EMPTY, MID, NOISY, SAMPLERS, SCALES, SHAPES, _cfg, _df, _inputs, _loop,
                                        _model, _ys)
from test_gpu_parity import LOOP_TOL, TINY, dev

pytestmark = pytest.mark.gpu
PHI = 0.7
KERNEL_SHAPES = [(3, 5, 3),         # N = 15: scalar path, one partial group
                 (1, 16, 256),      # N = 4096: exactly one chunk
                 (2, 16, 257),      # N = 4112: two chunks, vector path, ragged last chunk
                 (2, 17, 241)]      # N = 4097: scalar path, one-element last chunk
KERNEL_SCALES = (2.5, -1.0, 0.3)
SENTINEL = -12345.0


def _eng():
    return _model("mdm", "fp32")._get_engine(dev())


def _key(y, phi=PHI):
    return dict(y, guidance_rescale=phi)


def _ulps(a, b):
    """Largest distance in fp32 units in the last place between two tensors of positive floats."""
    return int((a.cpu().view(torch.int32).long() - b.cpu().view(torch.int32).long()).abs().max())


def _std64(v):
    return v.detach().cpu().double().reshape(v.shape[0], -1).std(dim=1)


# ------------------------------------------------------------------------------------------------------- 1. kernel against fp64
@functools.lru_cache(maxsize=None)
def _kernel_case(shape, offset):
    """(c, u, scale) on the host and {phi: (out, factor)} of the restatement, computed once per shape and data set."""
    Bk, J, T = shape
    g = torch.Generator().manual_seed(100 * J + T + int(offset))
    c = torch.randn(Bk, J, 1, T, generator=g) + offset
    u = torch.randn(Bk, J, 1, T, generator=g) + offset
    s = torch.tensor([KERNEL_SCALES[b % 3] for b in range(Bk)])
    return c, u, s, {phi: RR.rescale(c, u, s, phi) for phi in (0.0, 0.7, 1.0)}


def _blend_times(c, u, s, f):
    """(u + s (c - u)) * f in fp32 torch on the device: separate kernels, every operation rounded by itself."""
    return (u + s.view(-1, 1, 1, 1) * (c - u)) * f.view(-1, 1, 1, 1)


@pytest.mark.parametrize("misaligned", [False, True])
@pytest.mark.parametrize("shape", KERNEL_SHAPES)
def test_kernel_against_fp64(shape, misaligned):
    d = dev()
    eng = _eng()
    place = shifted if misaligned else (lambda t: t)
    for offset in (0.0, 50.0):              # randn, and randn + 50: the data an fp32 accumulation of the sums fails on
        c_h, u_h, s_h, want = _kernel_case(shape, offset)
        c, u, s = place(c_h.to(d)), place(u_h.to(d)), s_h.to(d)
        assert (c.data_ptr() % 16 != 0) == misaligned
        n = c.numel()
        for phi in (0.0, 0.7, 1.0):
            tag = (shape, misaligned, offset, phi)
            # an output 64 floats longer than the tensor: the tail must survive
            buf = torch.full((n + 64 + int(misaligned),), SENTINEL, device=d)
            out = buf[int(misaligned):int(misaligned) + n].view(c.shape)
            got, f = eng.cfg_rescale(c, u, s, phi, out=out)
            assert got.data_ptr() == out.data_ptr()
            assert bool((buf[int(misaligned) + n:] == SENTINEL).all()) and bool((buf[:int(misaligned)] == SENTINEL).all()), tag
            print(f"{tag}: factor {f.cpu().tolist()} restatement {want[phi][1].tolist()}")
            assert _ulps(f, want[phi][1]) <= 1, tag
            assert torch.equal(out, _blend_times(c, u, s, f)), tag
            if phi == 0.0:
                assert torch.equal(f, torch.ones_like(f)) and torch.equal(out, u + s.view(-1, 1, 1, 1) * (c - u)), tag
            if phi == 1.0 and offset == 0.0:
                ratio = _std64(out) / _std64(c)
                print(f"{tag}: std(out)/std(c) - 1 = {(ratio - 1).tolist()}")
                assert float((ratio - 1).abs().max()) < 1e-6, tag
            # in place on the conditional operand: the same bits
            c2 = place(c_h.to(d))
            got2, f2 = eng.cfg_rescale(c2, u, s, phi, out=c2)
            assert torch.equal(c2, out) and torch.equal(f2, f), tag


# ------------------------------------------------------------------------------------- 2. batch independence and edge cases
def test_a_sample_does_not_depend_on_its_batch():
    d = dev()
    eng = _eng()
    for offset in (0.0, 50.0):
        g = torch.Generator().manual_seed(9)
        c = (torch.randn(3, 17, 1, 241, generator=g) + offset).to(d)
        u = (torch.randn(3, 17, 1, 241, generator=g) + offset).to(d)
        s = torch.tensor(KERNEL_SCALES, device=d)
        out, f = eng.cfg_rescale(c, u, s, PHI)
        alone, fa = eng.cfg_rescale(c[1:2].contiguous(), u[1:2].contiguous(), s[1:2].contiguous(), PHI)
        assert torch.equal(out[1:2], alone) and torch.equal(f[1:2], fa)


def test_timesteps_select_per_sample():
    d = dev()
    eng = _eng()
    g = torch.Generator().manual_seed(10)
    c, u = torch.randn(2, 17, 1, 241, generator=g).to(d), torch.randn(2, 17, 1, 241, generator=g).to(d)
    s = torch.tensor(SCALES, device=d)
    every, fe = eng.cfg_rescale(c, u, s, PHI)
    out, f = eng.cfg_rescale(c, u, s, PHI, t=torch.tensor([100, 600], device=d), interval=MID)
    assert torch.equal(out[0], c[0]) and float(f[0]) == 1.0
    assert torch.equal(out[1], every[1]) and torch.equal(f[1], fe[1]) and float(f[1]) != 1.0
    out, f = eng.cfg_rescale(c, u, s, PHI, t=torch.tensor([300, 700], device=d), interval=MID)        # inclusive bounds
    assert torch.equal(out, every) and torch.equal(f, fe)
    out, f = eng.cfg_rescale(c, u, s, PHI, t=torch.tensor([299, 701], device=d), interval=MID)
    assert torch.equal(out, c) and torch.equal(f, torch.ones_like(f))


def test_constant_output_and_nan():
    d = dev()
    eng = _eng()
    s = torch.tensor(SCALES, device=d)
    k = torch.full((2, 17, 1, 241), 3.25, device=d)
    out, f = eng.cfg_rescale(k, k.clone(), s, PHI)
    assert torch.equal(f, torch.ones_like(f)) and torch.equal(out, k)            # g = u + s * 0
    g = torch.Generator().manual_seed(11)
    c, u = torch.randn(2, 17, 1, 241, generator=g).to(d), torch.randn(2, 17, 1, 241, generator=g).to(d)
    clean, fc = eng.cfg_rescale(c, u, s, PHI)
    for where, value in ((c, math.nan), (u, math.inf)):
        bad = where.clone()
        bad[1, 16, 0, 240] = value                                              # the last element: the one-element chunk
        out, f = eng.cfg_rescale(bad if where is c else c, bad if where is u else u, s, PHI)
        assert torch.equal(out[0], clean[0]) and torch.equal(f[0], fc[0]), value
        assert math.isnan(float(f[1])) and bool(torch.isnan(out[1]).all()), value


# --------------------------------------------------------------------------- 3. fused loop equals the step-wise protocol
@pytest.mark.parametrize("arch,T", SHAPES)
@pytest.mark.parametrize("sampler", SAMPLERS)
def test_fused_loop_equals_stepwise(arch, T, sampler):
    """torch.equal(fused, fused=False) with the key: plain, inpainting, clip_denoised, Philox noise for the noisy samplers, each
    without and with the mid guidance interval, fp32 and fp16; finite, and not the loop without the key."""
    df = _df(sampler)
    ran = 0
    for dtype in ("fp32", "fp16"):
        m = _model(arch, dtype)
        cases = [("plain", "tape"), ("inpaint", "tape"), ("clip", "tape")] + ([("plain", "philox")] if sampler in NOISY else [])
        for interval in (None, MID):
            for variant, rng in cases:
                y = _key(_ys(T, variant, interval)[0])
                kw = dict(clip=variant == "clip", rng=rng)
                fused = _loop(df, sampler, _cfg(m), y, T, **kw)
                step = _loop(df, sampler, _cfg(m), y, T, fused=False, **kw)
                tag = (arch, T, sampler, dtype, variant, rng, interval)
                assert torch.isfinite(fused).all(), tag
                assert torch.equal(fused, step), tag
                assert not torch.equal(fused, _loop(df, sampler, _cfg(m), _ys(T, variant, interval)[0], T, **kw)), tag
                ran += 1
    assert ran == (16 if sampler in NOISY else 12)


# -------------------------------------------------------------------------------------------------------- 4. off means off
@pytest.mark.parametrize("T", [20, 10])           # 20: gdx_sample_loop's token-major path, 10: the pose-layout path
@pytest.mark.parametrize("dtype", ["fp32", "fp16", "bf16"])
def test_off_means_off(T, dtype):
    """phi = 0 (int or float) and an absent key give the same bits; so does a call without the key after one with phi = 0.7 on
    the same engine -- a handle that kept its phi would show here -- in the loops and in the step-wise forward."""
    m = _model("mdm", dtype)
    d = dev()
    x = _inputs(T)[1]["tape"][3]
    t = torch.tensor([100, 600], device=d)
    y0 = _ys(T)[0]
    for sampler in SAMPLERS:
        df = _df(sampler)
        today = _loop(df, sampler, _cfg(m), y0, T)
        for zero in (0, 0.0):
            assert torch.equal(_loop(df, sampler, _cfg(m), _key(y0, zero), T), today), (sampler, zero)
        on = _loop(df, sampler, _cfg(m), _key(y0), T)
        assert not torch.equal(on, today), sampler
        assert torch.equal(_loop(df, sampler, _cfg(m), y0, T), today), (sampler, "a handle kept its phi")
    today = _cfg(m)(x, t, y=y0)
    assert torch.equal(_cfg(m)(x, t, y=_key(y0, 0)), today) and torch.equal(_cfg(m)(x, t, y=_key(y0, 0.0)), today)
    assert not torch.equal(_cfg(m)(x, t, y=_key(y0)), today)
    assert torch.equal(_cfg(m)(x, t, y=y0), today), "step-wise: a handle kept its phi"


def test_stepwise_forward_is_the_standalone_operation():
    """ClassifierFreeSampleModel.forward with the key == gdx_cfg_rescale on the two forwards of the inner model, with and
    without an interval across the batch."""
    m = _model("mdm", "fp32")
    d = dev()
    T = 20
    x = _inputs(T)[1]["tape"][3]
    t = torch.tensor([100, 600], device=d)
    y_cfg, y_in = _ys(T)
    c, u = m(x, t, y=y_in), m(x, t, y=dict(y_in, uncond=True))
    s = _inputs(T)[1]["scale"]
    eng = m._get_engine(d)
    assert torch.equal(_cfg(m)(x, t, y=_key(y_cfg)), eng.cfg_rescale(c, u, s, PHI)[0])
    got = _cfg(m)(x, t, y=_key(dict(y_cfg, guidance_interval=MID)))
    assert torch.equal(got, eng.cfg_rescale(c, u, s, PHI, t=t, interval=MID)[0]) and torch.equal(got[0], c[0])


# ------------------------------------------------------------------------------------------------------------ 5. work done
@pytest.mark.parametrize("arch,T", [("mdm", 20), ("mdm", 10), ("mdm_old", 12)])
def test_a_guided_step_still_runs_two_passes(arch, T):
    m = _model(arch, "fp32")
    eng = m._get_engine(dev())
    for sampler in SAMPLERS:
        df = _df(sampler)
        for interval in (None, MID):
            y = _ys(T, interval=interval)[0]
            before = eng.forward_samples()
            _loop(df, sampler, _cfg(m), y, T)
            plain = eng.forward_samples() - before
            before = eng.forward_samples()
            _loop(df, sampler, _cfg(m), _key(y), T)
            assert eng.forward_samples() - before == plain > 0, (sampler, interval)


# ------------------------------------------------------------------------------------------------------ 6. CPU restatement
@functools.lru_cache(maxsize=None)
def _oracle(arch, T, sampler, interval):
    host, _ = _inputs(T)
    p = weights_from(load_golden(f"loops_{arch}_tiny.npz"))
    cfg = dict(TINY, arch=arch)
    y = {"seed": host["seed"], "mfcc": host["mfcc"], "scale": host["scale"]}
    if sampler == "dpmpp":
        tmap = diffusion("linear", "logsnr10").timestep_map
        return RR.dpm_loop(p, cfg, PHI, interval, "linear", tmap, host["tape"][0], y, 2)
    return RR.sample_loop(p, cfg, PHI, interval, "cosine", "ddim10", host["tape"], y, sampler,
                          eta=DDIM_ETA if sampler == "ddim" else 0.0)


@pytest.mark.parametrize("interval", [None, MID])
@pytest.mark.parametrize("arch,T", [("mdm", 20), ("mdm", 10), ("mdm_old", 12)])
@pytest.mark.parametrize("sampler", ["p", "ddim", "dpmpp"])
def test_rescaled_loop_vs_cpu_restatement(arch, T, sampler, interval):
    """The fused loop with the key against the CPU restatement (oracle forwards, fp64 statistics, oracle loops / the fp64 DPM
    recurrence): fp32 within the suite's LOOP_TOL, fp16 / bf16 within numerics.stated_tolerance for the largest guidance factor of
    the scales used, times the largest rescale factor where one exceeds 1.  On the V2 model every factor the restatement computes
    is <= 1 (0.58 .. 0.77: guidance widens the output, the rescale shrinks the guided prediction and its error with it), so the
    tolerances of the unrescaled loop hold as they are.  On MDM_Old with these weights std(g) ~ std(c) and the restatement's
    factors reach 1.0084: the guided prediction's error is multiplied by f, hence the 16-bit tolerance too."""
    from gesturediffusion_amd.numerics import guidance_factor, stated_tolerance
    want, factors = _oracle(arch, T, sampler, interval)
    print(f"{arch} T={T} {sampler} {interval}: factors of the restatement in [{min(factors):.4f}, {max(factors):.4f}]")
    assert factors and min(factors) > 0
    if arch == "mdm":
        assert max(factors) <= 1.0, max(factors)
    amp = max(1.0, max(factors))
    worst = max(SCALES, key=guidance_factor)
    for dtype in ("fp32", "fp16", "bf16"):
        tol = LOOP_TOL if dtype == "fp32" else stated_tolerance(dtype, worst) * amp
        got = _loop(_df(sampler), sampler, _cfg(_model(arch, dtype)), _key(_ys(T, interval=interval)[0]), T)
        err = rel_err(got.cpu(), want)
        print(f"{arch} T={T} {sampler} {interval} {dtype}: rel err vs the restatement {err:.3e} (tolerance {tol:.1e})")
        assert err < tol, (dtype, err)


# ------------------------------------------------------------------------------------------------------------ 7. gdx_bpd_loop
def test_bpd_loop_equals_the_stepwise_terms():
    m = _model("mdm", "fp32")
    df = _df("p")
    T = 20
    _, i = _inputs(T)
    y = _key(_ys(T, interval=MID)[0])
    kw = dict(clip_denoised=True, model_kwargs={"y": y}, noise_tape=i["tape"][:10].contiguous())
    fused = df.calc_bpd_loop(_cfg(m), i["x_start"], **kw)
    step = df.calc_bpd_loop(_cfg(m), i["x_start"], fused=False, **kw)
    for k in ("total_bpd", "prior_bpd", "vb", "xstart_mse", "mse"):
        assert torch.isfinite(fused[k]).all() and torch.equal(fused[k], step[k]), k
    plain = df.calc_bpd_loop(_cfg(m), i["x_start"], **dict(kw, model_kwargs={"y": _ys(T, interval=MID)[0]}))
    assert not torch.equal(plain["vb"], fused["vb"])


# ------------------------------------------------------------------------------------------------------------ 8. graph replay
@pytest.mark.parametrize("arch", ["mdm", "mdm_old"])
def test_graph_replay_with_the_rescale_equals_eager(arch):
    """Graph replay on: a call whose guided steps are rescaled replays a step that holds the three launches (every timestep),
    runs eagerly (mid interval) or replays a step without them (empty interval); all equal the eager results."""
    m = _model(arch, "fp32")
    eng = m._get_engine(dev())
    T = 20
    for sampler in ("p", "ddim"):
        df = _df(sampler)
        ys = {iv: _key(_ys(T, interval=iv)[0]) for iv in (MID, ALL, EMPTY)}
        eager = {iv: _loop(df, sampler, _cfg(m), ys[iv], T) for iv in ys}
        assert not torch.equal(eager[ALL], eager[EMPTY]) and not torch.equal(eager[ALL], eager[MID])
        eng.set_graph_replay(True)
        try:
            for iv in ys:
                assert torch.equal(_loop(df, sampler, _cfg(m), ys[iv], T), eager[iv]), (sampler, iv)
        finally:
            eng.set_graph_replay(False)


# -------------------------------------------------------------------------------------------------------- 9. workspace guards
@pytest.mark.parametrize("arch,T", [("mdm", 20), ("mdm", 10), ("mdm_old", 12)])
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_rescaled_loop_leaves_the_workspace_guards_intact(arch, T, dtype):
    m = _model(arch, dtype)
    d = dev()
    eng = m._get_engine(d)
    eng.set_guards(True)
    try:
        for sampler in SAMPLERS:
            r = _loop(_df(sampler), sampler, _cfg(m), _key(_ys(T, interval=MID)[0]), T)
            bad, zone = eng.check_guards(d)
            assert bad == 0, f"{sampler}: {bad} canary bytes overwritten, first in workspace allocation #{zone}"
            assert torch.isfinite(r).all()
    finally:
        eng.set_guards(False)


# -------------------------------------------------------------------------------------------------------------------- 10. CLI
def test_generate_cli_with_the_rescale_equals_a_direct_call(tmp_path, capsys):
    """`sample.generate --synthetic --guidance_rescale 0.7 --sampler dpmpp --timestep_respacing logsnr10 --chunks 2` at a small
    width: both chunks equal a direct sample_chunks call on the inputs the CLI builds from its seed, the rescale line is
    printed, and the result is not the one without the flag."""
    from gesturediffusion_amd.sample import generate
    from gesturediffusion_amd.utils.init import MFCC_DIM, init_state_dict
    from gesturediffusion_amd.utils.model_util import create_model_and_diffusion
    from gesturediffusion_amd.utils.parser_util import generate_args
    out = tmp_path / "out"
    argv = ["--synthetic", "--guidance_rescale", "0.7", "--sampler", "dpmpp", "--timestep_respacing", "logsnr10",
            "--chunks", "2", "--latent_dim", "128", "--layers", "2", "--num_samples", "3", "--synthetic_njoints", "37",
            "--output_dir", str(out), "--seed", "7", "--arch_version", "mdm", "--num_frames", "20", "--rng", "philox"]
    assert generate.main(argv) == 0
    printed = capsys.readouterr().out
    assert "### guidance rescale 0.70" in printed
    res = np.load(out / "results.npy", allow_pickle=True).item()      # written by this test a moment ago
    assert res["motion"].shape == (3, 37, 1, 40) and np.isfinite(res["motion"]).all()
    d = dev()
    args = generate_args(argv)
    args.mfcc_input = True
    model, df = create_model_and_diffusion(args, None)
    cfg = dict(arch="mdm", njoints=37, nfeats=1, latent_dim=128, ff_size=1024, num_layers=2, num_heads=4, seed_poses=args.seed_poses)
    model.load_state_dict(init_state_dict(cfg, seed=7), strict=False)
    model = _cfg(model).to(d).eval()
    gen = torch.Generator().manual_seed(7)
    seedp = torch.randn(3, 37, 1, args.seed_poses, generator=gen).to(d)
    mfcc = lambda chunk: torch.randn(3, MFCC_DIM, 1, 20, generator=gen).to(d)   # noqa: E731
    kw = dict(guidance_param=args.guidance_param, sampler="dpmpp", rng="philox", philox_seed=7, dpm_order=2)
    want = generate.sample_chunks(model, df, seedp, mfcc, 2, 20, args.seed_poses, guidance_rescale=0.7, **kw)
    assert np.array_equal(res["motion"], torch.cat(want, dim=3).cpu().numpy())
    gen.manual_seed(7)
    torch.randn(3, 37, 1, args.seed_poses, generator=gen)
    plain = generate.sample_chunks(model, df, seedp, mfcc, 2, 20, args.seed_poses, **kw)
    assert not np.array_equal(res["motion"], torch.cat(plain, dim=3).cpu().numpy())


# -------------------------------------------------------------------------------------------------------------- 11. refusals
def test_refusals_of_the_key():
    """The key on a model that runs no guidance, and anything but a finite number in [0, 1], raise ValueError -- in every loop,
    step-wise and in calc_bpd_loop; the handle refuses a phi outside [0, 1] and keeps the one it had."""
    from gesturediffusion_amd.engine import GdxError
    m = _model("mdm", "fp32")
    d = dev()
    T = 20
    df = _df("p")
    y_cfg, y_in = _ys(T)
    x = _inputs(T)[1]["tape"][0]
    t = torch.tensor([100, 600], device=d)
    for sampler in SAMPLERS:
        with pytest.raises(ValueError, match="ClassifierFreeSampleModel"):
            _loop(_df(sampler), sampler, m, _key(y_in), T)
    with pytest.raises(ValueError, match="ClassifierFreeSampleModel"):
        m(x, t, y=_key(y_in))
    with pytest.raises(ValueError, match="ClassifierFreeSampleModel"):
        df.calc_bpd_loop(m, x, model_kwargs={"y": _key(y_in)})
    for bad in (True, -0.1, 1.5, math.nan, "0.7", torch.tensor(0.7, device=d), torch.tensor(0.7)):
        with pytest.raises(ValueError, match="guidance_rescale"):
            _loop(df, "p", _cfg(m), _key(y_cfg, bad), T)
        with pytest.raises(ValueError, match="guidance_rescale"):
            _cfg(m)(x, t, y=_key(y_cfg, bad))
        with pytest.raises(ValueError, match="guidance_rescale"):
            df.calc_bpd_loop(_cfg(m), x, model_kwargs={"y": _key(y_cfg, bad)})
    eng = m._get_engine(d)
    today = _cfg(m)(x, t, y=y_cfg)
    eng.set_guidance_rescale(PHI)
    for bad in (-0.1, 1.5, math.nan):
        with pytest.raises(GdxError, match=r"phi must lie in \[0, 1\]"):
            eng.set_guidance_rescale(bad)
    for ok in (0.0, 1.0, 0):
        eng.set_guidance_rescale(ok)
    assert torch.equal(_cfg(m)(x, t, y=y_cfg), today)
