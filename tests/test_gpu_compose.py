"""Per-condition guidance for use_text models on the GPU (y['guidance_drop'] / y['text_scale'] / y['guidance_order'],
gdx_set_guidance_compose; include/gdx.h): the conditioning rows of every row group, guided forwards of every mode against the
formula on four plain forwards bit for bit, the 16-bit modes, the samples counted, the seven in-library loops against their
step-wise twins and the reference's fixture, the rescale, the refusals, workspace guards, a side stream, and no state left behind.

Shapes: the cases of tests/golden/forward_text_compose.npz (J = 16, d = 128, one layer, B = 3, T = 20: J*T % 4 == 0, the 128-bit
path) and compose_restatement.scalar_case (J = 37, T = 30, B = 2: J*T % 4 == 2, the scalar path with a two-element tail).
Need an MI355X."""
import functools

import numpy as np
import pytest
import torch

import compose_restatement as cr
import text_restatement as tr
from conftest import load_golden, rel_err
from gesturediffusion_amd import numerics
from gesturediffusion_amd._lib import GDX_CFG, GDX_SAMPLER_DDIM, GDX_SAMPLER_P, GdxError
from gesturediffusion_amd.model.cfg_sampler import ClassifierFreeSampleModel
from test_gpu_parity import dev
from test_gpu_text import diffusion, on_dev

pytestmark = pytest.mark.gpu
T64, T40, SCALAR = "mdm_128_t64", "mdm_128_t40", "scalar"
MID = (300, 700)                      # of t = [7, 993, 500] only the last sample is guided
SEED_SCALE, TEXT_SCALE = (1.5, 2.5, 0.75), (3.0, -1.0, 2.25)


@functools.lru_cache(maxsize=None)
def golden():
    return load_golden("forward_text_compose.npz")


@functools.lru_cache(maxsize=None)
def case(name):
    """(cfg, weights, x, t, y) on the host; shared, read only."""
    return cr.scalar_case() if name == SCALAR else cr.case(golden(), name)


def model_of(name, dtype="fp32"):
    cfg, sd = case(name)[:2]
    m = tr.build_text_model(cfg, sd).to(dev())
    m.compute_dtype = dtype
    return m


def inputs(name):
    cfg, sd, x, t, y = case(name)
    return x.to(dev()), t.to(dev()), on_dev(y)


def keys_of(mode, yd, B):
    """y of the guided model for a compose mode, with two different scale vectors."""
    scale = torch.tensor(SEED_SCALE[:B], device=dev())
    y = dict(yd, scale=scale)
    if mode in (cr.TEXT, cr.SEED):
        y["guidance_drop"] = "text" if mode == cr.TEXT else "seed"
    if mode >= cr.SEED_TEXT:
        y["text_scale"] = torch.tensor(TEXT_SCALE[:B], device=dev())
        y["guidance_order"] = "seed_text" if mode == cr.SEED_TEXT else "text_seed"
    return y


def plain_passes(m, x, t, yd, tags="FSXU"):
    """The four conditioning states as plain GDX_COND forwards of the inner model with the dropped inputs zeroed."""
    return {tag: m(x, t, cr.dropped(yd, tag)).clone() for tag in tags}


def formula(mode, p, y):
    """gdx.h's rule in torch's separate ops on the device (every difference, product and sum its own kernel)."""
    return cr.compose(mode, p, y["scale"], y.get("text_scale"))


# ----------------------------------------------------------------------------------------------------------------- 1. rows
@pytest.mark.parametrize("name", [T40, T64])
def test_rows_of_every_group(name):
    """Token 0 of every row group of a guided forward (tap 0; RoPE at position 0 is the identity) against the fp64 rows with the
    matching input zeroed, at test_gpu_text's tolerance for the same quantity; after a switch to mode 1, GDX_UNCOND still gives U."""
    cfg, sd, xh, th_, yh = case(name)
    x, t, yd = inputs(name)
    B, S, d = x.shape[0], x.shape[3] + 1, cfg["latent_dim"]
    m = model_of(name)
    eng = m._get_engine(dev())
    eng.keep_taps(True)
    want = {tag: tr.token0_rows(sd, cfg, th_, cr.dropped(yh, tag)["seed"], cr.dropped(yh, tag)["text_embed"])[0] for tag in "FSXU"}
    assert torch.equal(want["U"], tr.token0_rows(sd, cfg, th_, yh["seed"], yh["text_embed"], uncond=True)[0])
    for mode, groups in cr.GROUPS.items():
        ClassifierFreeSampleModel(m)(x, t, keys_of(mode, yd, B))
        G = len(groups)
        tap = eng.tap(0, G * B * S, d, dev()).view(G, B, S, d)[:, :, 0].cpu().double()
        for gi, tag in enumerate(groups):
            err = float((tap[gi] - want[tag]).abs().max() / want[tag].abs().max())
            print(f"[compose-measure] token 0 {name} mode {mode} group {gi} = {tag}: max err / max|row| {err:.2e}")
            assert err < 1e-5, (mode, tag)
        if mode != cr.JOINT:
            assert not torch.equal(tap[0], tap[1])
    # mode 1 keeps S in group 1; the all-dropped rows are still what GDX_UNCOND reads
    ClassifierFreeSampleModel(m)(x, t, keys_of(cr.TEXT, yd, B))
    eng.forward(x, t, mode=1)                                                 # GDX_UNCOND on the handle as mode 1 left it
    un = eng.tap(0, B * S, d, dev()).view(B, S, d)[:, 0].cpu().double()
    assert float((un - want["U"]).abs().max() / want["U"].abs().max()) < 1e-5
    assert float((un - want["S"]).abs().max() / want["S"].abs().max()) > 1e-3
    eng.keep_taps(False)


# ------------------------------------------------------------------------------------------------------- 2. forwards, fp32
@pytest.mark.parametrize("name", [T40, T64, SCALAR])
def test_forwards_are_the_formula_on_four_plain_forwards(name):
    """gdx_forward under GDX_CFG in every mode is torch.equal to the rule evaluated with torch's separate ops on four plain
    GDX_COND forwards with zeroed inputs (rows are batch-invariant in fp32); with the mid interval only the last sample is
    composed, the others are F."""
    x, t, yd = inputs(name)
    B = x.shape[0]
    m = model_of(name)
    p = plain_passes(m, x, t, yd)
    g = ClassifierFreeSampleModel(m)
    outs = {}
    for mode in cr.GROUPS:
        y = keys_of(mode, yd, B)
        got = g(x, t, y)
        want = formula(mode, p, y)
        diff = float((got - want).abs().max())
        print(f"[compose-measure] forward {name} mode {mode}: max |got - formula| {diff:.3e}")
        assert torch.equal(got, want), (mode, diff)
        outs[mode] = got.clone()
        if B == 3:
            lim = g(x, t, dict(y, guidance_interval=MID))
            assert torch.equal(lim[:2], p["F"][:2]) and torch.equal(lim[2], want[2]), mode
    assert len({tuple(o.flatten()[:64].tolist()) for o in outs.values()}) == 5       # five rules, five results
    if name == T64:
        gold = golden()
        for tag in "FSXU":
            assert rel_err(p[tag].cpu(), gold[f"{name}.{tag}"]) < numerics.FORWARD_TOL["fp32"], tag


# ------------------------------------------------------------------------------------------------------ 3. forwards, 16-bit
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("name", [T64, SCALAR])
def test_forwards_16_bit(name, dtype):
    """Every mode in fp16 / bf16 against the fp32 result, within numerics.py's bound for a blend with |s| replaced by
    |s0| + |s1| (the 3-pass rule is (1 - s0) U + (s0 - s1) M + s1 F: three forwards with independent errors)."""
    x, t, yd = inputs(name)
    B = x.shape[0]
    g32, g16 = ClassifierFreeSampleModel(model_of(name)), ClassifierFreeSampleModel(model_of(name, dtype))
    for mode in cr.GROUPS:
        y = keys_of(mode, yd, B)
        s = y["scale"].abs() + (y["text_scale"].abs() if "text_scale" in y else 0)
        tol = numerics.stated_tolerance(dtype, float(s.max()), loop=False)
        want = g32(x, t, y)
        err = rel_err(g16(x, t, y).cpu(), want.cpu())
        print(f"[compose-measure] forward {name} mode {mode} {dtype}: rel err {err:.2e} (bound {tol:.2e})")
        assert err < tol, (mode, err)


# --------------------------------------------------------------------------------------------------------- 4. sample counter
def test_samples_counted():
    x, t, yd = inputs(T40)
    B = x.shape[0]
    m = model_of(T40)
    g = ClassifierFreeSampleModel(m)
    eng = m._get_engine(dev())
    for mode, groups in cr.GROUPS.items():
        before = eng.forward_samples()
        g(x, t, keys_of(mode, yd, B))
        assert eng.forward_samples() - before == len(groups) * B, mode
    df = diffusion(tr.RESPACING)
    flags = df.guided_steps(MID)
    assert 0 < sum(flags) < len(flags)
    for mode, groups in cr.GROUPS.items():
        before = eng.forward_samples()
        df.p_sample_loop(g, tuple(x.shape), clip_denoised=False, progress=False, rng="philox", philox_seed=3,
                         model_kwargs={"y": dict(keys_of(mode, yd, B), guidance_interval=MID)})
        want = sum(len(groups) * B if f else B for f in flags)                 # a step outside the interval: B, neither contrast pass
        assert eng.forward_samples() - before == want, mode


# ------------------------------------------------------------------------------------------------------------------ 5. loops
def _loops(df, dfd, g, x, y, fused):
    """The seven in-library loops on the guided model g, each as (name, result tensors)."""
    shape = tuple(x.shape)
    kw = dict(clip_denoised=False, progress=False, model_kwargs={"y": y}, fused=fused)
    yield "p", [df.p_sample_loop(g, shape, rng="philox", philox_seed=5, **kw)]
    yield "ddim", [df.ddim_sample_loop(g, shape, noise=x.clone(), eta=0.0, rng="philox", philox_seed=5, **kw)]
    yield "plms", [df.plms_sample_loop(g, shape, noise=x.clone(), order=2, **kw)]
    yield "dpmpp", [dfd.dpm_solver_sample_loop(g, shape, noise=x.clone(), order=2, **kw)]
    yield "dpmpp_sde", [dfd.dpm_solver_sde_sample_loop(g, shape, noise=x.clone(), order=2, eta=1.0, rng="philox", philox_seed=5, **kw)]
    yield "unipc", [dfd.unipc_sample_loop(g, shape, noise=x.clone(), order=2, **kw)]
    yield "ddim_reverse", [df.ddim_reverse_sample_loop(g, 0.5 * x, clip_denoised=False, model_kwargs={"y": y}, fused=fused)]
    r = df.calc_bpd_loop(g, 0.5 * x, clip_denoised=True, model_kwargs={"y": y}, rng="philox", philox_seed=5, fused=fused)
    yield "bpd", [r[k] for k in ("total_bpd", "prior_bpd", "vb", "xstart_mse", "mse")]


@pytest.mark.parametrize("name", [T40, SCALAR])
def test_fused_loops_equal_their_stepwise_twins(name):
    """Each of the seven fused loops in mode 3 equals its step-by-step Python twin (fused=False) bit for bit; p_sample_loop also in
    mode 4 and mode 1, without and with a guidance interval; the progressive generator ends on the fused loop's bits."""
    x, t, yd = inputs(name)
    B = x.shape[0]
    g = ClassifierFreeSampleModel(model_of(name))
    df, dfd = diffusion("ddim10"), diffusion("logsnr10")
    y = keys_of(cr.SEED_TEXT, yd, B)
    fused = {k: [v.clone() for v in r] for k, r in _loops(df, dfd, g, x, y, True)}
    step = {k: [v.clone() for v in r] for k, r in _loops(df, dfd, g, x, y, False)}
    assert len(fused) == 8                                                  # gdx_sample_loop serves p and ddim
    for k in fused:
        for a, b in zip(fused[k], step[k]):
            assert bool(torch.isfinite(a).all()) and torch.equal(a, b), k
    y_joint = dict(yd, scale=y["scale"])
    joint = df.p_sample_loop(g, tuple(x.shape), clip_denoised=False, progress=False, rng="philox", philox_seed=5, model_kwargs={"y": y_joint})
    assert not torch.equal(joint, fused["p"][0])
    for mode in (cr.TEXT_SEED, cr.TEXT):
        for interval in (None, MID):
            ym = keys_of(mode, yd, B)
            if interval is not None:
                ym["guidance_interval"] = interval
            runs = [df.p_sample_loop(g, tuple(x.shape), clip_denoised=False, progress=False, rng="philox", philox_seed=5,
                                     model_kwargs={"y": ym}, fused=f).clone() for f in (True, False)]
            assert torch.equal(runs[0], runs[1]) and not torch.equal(runs[0], joint), (mode, interval)
    # the progressive generator (deterministic at eta = 0): its last state is the fused loop's
    last = None
    for last in df.ddim_sample_loop_progressive(g, tuple(x.shape), noise=x.clone(), clip_denoised=False, model_kwargs={"y": y}, eta=0.0):
        pass
    assert torch.equal(last["sample"], fused["ddim"][0])


@pytest.mark.parametrize("order", ["seed_text", "text_seed"])
def test_p_loop_vs_reference_fixture(order):
    """p_sample_loop on [20] steps with the recorded tape and the fixture's two scale vectors against the reference's own loop
    around the composed model, within 2e-5 (fp32)."""
    gold = golden()
    x, t, yd = inputs(T64)
    g = ClassifierFreeSampleModel(model_of(T64))
    tape = torch.from_numpy(gold[f"{T64}.{order}_p20.tape"]).to(dev())
    y = dict(yd, scale=torch.from_numpy(gold[T64 + ".seed_scale"]).to(dev()), text_scale=torch.from_numpy(gold[T64 + ".text_scale"]).to(dev()),
             guidance_order=order)
    r = diffusion(tr.RESPACING).p_sample_loop(g, tuple(x.shape), noise_tape=tape, clip_denoised=False, model_kwargs={"y": y}, progress=False)
    err = rel_err(r.cpu(), gold[f"{T64}.{order}_p20.out"])
    print(f"[compose-measure] guided p20 loop {order}: rel err {err:.2e}")
    assert err < 2e-5


@pytest.mark.parametrize("name", [T40, SCALAR])
def test_block_wise_issue_gives_the_bits_of_one_call(name):
    x, t, yd = inputs(name)
    B = x.shape[0]
    g = ClassifierFreeSampleModel(model_of(name))
    df = diffusion(tr.RESPACING)
    n = df.num_timesteps
    y = dict(keys_of(cr.SEED_TEXT, yd, B), guidance_interval=MID)
    gen = torch.Generator().manual_seed(11)
    tape = torch.randn(n + 1, *x.shape, generator=gen).to(dev())
    whole = df.p_sample_loop(g, tuple(x.shape), noise_tape=tape, clip_denoised=False, model_kwargs={"y": y}, progress=False)
    state = tape[0].clone()
    eng, mode, scale, mask, motion = df._native_loop_setup(g, state, {"y": y})
    assert mode == GDX_CFG and tuple(scale.shape) == (2, B)
    coef, tmap = df.coef_table(GDX_SAMPLER_P, dev(), 0.0), df._timestep_map()
    k = 0
    for nb in (3, 1, 9, n - 13):
        eng.sample_loop(state, GDX_SAMPLER_P, mode, coef, tmap, n - 1 - k, scale=scale, noise_tape=tape[1 + k:], run_steps=nb, k_base=k)
        k += nb
    assert torch.equal(state, whole)


# ---------------------------------------------------------------------------------------------------------------- 6. rescale
@pytest.mark.parametrize("name", [T40, SCALAR])
def test_rescale_in_mode_3(name):
    """phi = 0.7 in mode 3: out = fl32(g * f) with c = F, g the composed prediction and f within one fp32 ulp of an fp64
    evaluation of phi * std(F) / std(g) + (1 - phi), per sample; the fused loop with the key equals its step-wise twin."""
    phi = 0.7
    x, t, yd = inputs(name)
    B = x.shape[0]
    m = model_of(name)
    g = ClassifierFreeSampleModel(m)
    y = keys_of(cr.SEED_TEXT, yd, B)
    comp = g(x, t, y).clone()
    F = m(x, t, yd).clone()
    out = g(x, t, dict(y, guidance_rescale=phi))
    c64, g64 = F.double().reshape(B, -1), comp.double().reshape(B, -1)
    f64 = phi * c64.std(dim=1, unbiased=False) / g64.std(dim=1, unbiased=False) + (1 - phi)
    f32 = f64.float()
    for b in range(B):
        cands = [f32[b], torch.nextafter(f32[b], f32[b] + 1), torch.nextafter(f32[b], f32[b] - 1)]
        hits = [bool(torch.equal(out[b], comp[b] * c)) for c in cands]
        print(f"[compose-measure] rescale {name} sample {b}: f64 {float(f64[b]):.9f}, matches (f, f+ulp, f-ulp) {hits}")
        assert any(hits), b
    assert not torch.equal(out, comp)
    lim = g(x, t, dict(y, guidance_rescale=phi, guidance_interval=MID))
    if B == 3:
        assert torch.equal(lim[:2], F[:2]) and torch.equal(lim[2], out[2])
    df = diffusion("ddim10")
    runs = [df.p_sample_loop(g, tuple(x.shape), clip_denoised=False, progress=False, rng="philox", philox_seed=5,
                             model_kwargs={"y": dict(y, guidance_rescale=phi)}, fused=f).clone() for f in (True, False)]
    assert torch.equal(runs[0], runs[1])


# -------------------------------------------------------------------------------------------------------------- 7. refusals
def test_refusals_on_the_device():
    """Refresh, layer cache and the parallel loop are refused in mode 3 with nothing launched; the y keys raise ValueError in
    every loop; the setter refuses what it must and leaves the handle as it was."""
    x, t, yd = inputs(T64)
    B = x.shape[0]
    m = model_of(T64)
    g = ClassifierFreeSampleModel(m)
    df = diffusion(tr.RESPACING)
    n = df.num_timesteps
    y = keys_of(cr.SEED_TEXT, yd, B)
    state = x.clone()
    eng, mode, scale, mask, motion = df._native_loop_setup(g, state, {"y": y})
    coef, tmap = df.coef_table(GDX_SAMPLER_P, dev(), 0.0), df._timestep_map()
    before = eng.forward_samples()
    hist, scratch = torch.zeros(2, *x.shape, device=dev()), torch.zeros_like(x)
    eng.set_guidance_refresh(2)
    for call in (lambda: eng.sample_loop(state, GDX_SAMPLER_P, mode, coef, tmap, n - 1, scale=scale, philox_seed=1),
                 lambda: eng.plms_loop(state, mode, 2, df.coef_table(GDX_SAMPLER_DDIM, dev(), 0.0), tmap, n - 1, hist, scratch, scale=scale)):
        with pytest.raises(GdxError, match=r"guidance refresh .*3-pass guidance compose mode"):
            call()
    eng.set_guidance_refresh(1)
    planes = torch.zeros(3, B, *x.shape[1:], device=dev())
    with pytest.raises(GdxError, match="3-pass guidance compose mode .* not supported by the parallel loop"):
        eng.parallel_loop(planes, GDX_SAMPLER_P, mode, coef, tmap, np.zeros(n), n - 1, scale=scale)
    assert eng.forward_samples() == before and torch.equal(state, x)
    # through y: ValueError in front of any launch
    for extra, says in ((dict(guidance_refresh=2), "guidance_refresh"), (dict(guidance_drop="text"), "exclude each other")):
        with pytest.raises(ValueError, match=says):
            df.p_sample_loop(g, tuple(x.shape), model_kwargs={"y": dict(y, **extra)}, progress=False)
    with pytest.raises(ValueError, match="parallel_sample_loop"):
        df.parallel_sample_loop(g, tuple(x.shape), model_kwargs={"y": y}, window=2)
    with pytest.raises(ValueError, match="ClassifierFreeSampleModel"):
        df.p_sample_loop(m, tuple(x.shape), model_kwargs={"y": {k: v for k, v in y.items() if k != "scale"}}, progress=False)
    with pytest.raises(ValueError, match="text_scale"):
        g(x, t, dict(y, text_scale=y["text_scale"][:2]))
    assert eng.forward_samples() == before
    # the setter: an unknown mode leaves the handle in mode 3, conditioned as it was
    want = g(x, t, y).clone()
    assert eng.lib.gdx_set_guidance_compose(eng.handle, 5) != 0 and b"unknown mode" in eng.lib.gdx_last_error()
    assert torch.equal(g(x, t, y), want)
    from test_gpu_parity import TINY, build_model
    from conftest import weights_from
    plain = build_model("mdm", TINY, weights_from(load_golden("loops_mdm_tiny.npz")))
    pe = plain._get_engine(dev())
    with pytest.raises(GdxError, match="nothing to compose"):
        pe.set_guidance_compose(1)
    with pytest.raises(ValueError, match="use_text"):
        ClassifierFreeSampleModel(plain)(torch.zeros(2, 16, 1, 20, device=dev()), torch.zeros(2, device=dev(), dtype=torch.long),
                                         {"seed": torch.zeros(2, 16, 1, 10, device=dev()), "mfcc": torch.zeros(2, 26, 1, 20, device=dev()),
                                          "scale": torch.ones(2, device=dev()), "guidance_drop": "text"})


def test_layer_cache_is_refused_in_mode_3():
    """A two-layer text handle (keep = 1 exists): the layer cache under a 3-pass mode is refused by the loop before its first
    launch, and accepted again in mode 1."""
    from gesturediffusion_amd.utils.init import init_state_dict, synthetic_inputs
    cfg = tr.text_cfg(40, 32, layers=2)
    m = tr.build_text_model(cfg, init_state_dict(cfg, seed=4, perturb=True)).to(dev())
    g = ClassifierFreeSampleModel(m)
    x, seedp, mfcc, text = (v.to(dev()) for v in synthetic_inputs(cfg, 2, 20, seed=6))
    yd = {"seed": seedp, "mfcc": mfcc, "text_embed": text}
    df = diffusion(tr.RESPACING)
    n = df.num_timesteps
    state = x.clone()
    eng, mode, scale, mask, motion = df._native_loop_setup(g, state, {"y": keys_of(cr.TEXT_SEED, yd, 2)})
    coef, tmap = df.coef_table(GDX_SAMPLER_P, dev(), 0.0), df._timestep_map()
    before = eng.forward_samples()
    eng.set_layer_cache(2, 1)
    with pytest.raises(GdxError, match=r"layer cache .*3-pass guidance compose mode"):
        eng.sample_loop(state, GDX_SAMPLER_P, mode, coef, tmap, n - 1, scale=scale, philox_seed=1)
    assert eng.forward_samples() == before and torch.equal(state, x)
    with pytest.raises(ValueError, match="layer_cache"):
        df.p_sample_loop(g, tuple(x.shape), model_kwargs={"y": dict(keys_of(cr.TEXT_SEED, yd, 2), layer_cache=(2, 1))}, progress=False)
    kw = dict(clip_denoised=False, progress=False, rng="philox", philox_seed=2)
    y1 = dict(keys_of(cr.TEXT, yd, 2), layer_cache=(2, 1), guidance_refresh=2)
    cached = df.p_sample_loop(g, tuple(x.shape), model_kwargs={"y": y1}, **kw)
    assert bool(torch.isfinite(cached).all())


# ----------------------------------------------------------------------------------------------------------------- 8. guards
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("name", [T40, SCALAR])
def test_guards_stay_intact(name, dtype):
    x, t, yd = inputs(name)
    B = x.shape[0]
    m = model_of(name, dtype)
    g = ClassifierFreeSampleModel(m)
    eng = m._get_engine(dev())
    eng.set_guards(True)
    try:
        for mode in (cr.SEED_TEXT, cr.JOINT, cr.TEXT_SEED, cr.TEXT):         # 3 groups, back to 2, 3 again: the workspace re-prepared
            y = keys_of(mode, yd, B)
            out = g(x, t, dict(y, guidance_rescale=0.5))
            bad, zone = eng.check_guards(dev())
            assert bad == 0 and bool(torch.isfinite(out).all()), f"forward mode {mode}: {bad} canary bytes, first in allocation #{zone}"
            r = diffusion("ddim10").p_sample_loop(g, tuple(x.shape), clip_denoised=False, progress=False, rng="philox", philox_seed=5,
                                                  model_kwargs={"y": y})
            bad, zone = eng.check_guards(dev())
            assert bad == 0 and bool(torch.isfinite(r).all()), f"loop mode {mode}: {bad} canary bytes, first in allocation #{zone}"
    finally:
        eng.set_guards(False)


# ----------------------------------------------------------------------------------------------------------------- 9. stream
def test_side_stream_gives_the_default_streams_bits():
    """A mode-3 forward and gdx_sample_loop on a non-default stream, on a handle whose every allocation happens there."""
    x, t, yd = inputs(T40)
    B = x.shape[0]
    y = keys_of(cr.SEED_TEXT, yd, B)
    df = diffusion("ddim10")
    kw = dict(clip_denoised=False, progress=False, rng="philox", philox_seed=5, model_kwargs={"y": y})
    g = ClassifierFreeSampleModel(model_of(T40))
    want = (g(x, t, y).clone(), df.p_sample_loop(g, tuple(x.shape), **kw).clone())
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev())
    assert side.cuda_stream != 0
    g2 = ClassifierFreeSampleModel(model_of(T40))
    with torch.cuda.stream(side):
        got = (g2(x, t, y).clone(), df.p_sample_loop(g2, tuple(x.shape), **kw).clone())
    side.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- 10. no leak
def test_no_mode_is_left_behind():
    """After mode 3 and back to JOINT (absent keys), a guided forward and loop equal a fresh handle's bit for bit; so does a plain
    forward, cond and uncond."""
    x, t, yd = inputs(T40)
    B = x.shape[0]
    y0 = dict(yd, scale=torch.tensor(SEED_SCALE[:B], device=dev()))
    df = diffusion("ddim10")
    kw = dict(clip_denoised=False, progress=False, rng="philox", philox_seed=5)
    fresh_m = model_of(T40)
    fresh = ClassifierFreeSampleModel(fresh_m)
    want = (fresh(x, t, y0).clone(), df.p_sample_loop(fresh, tuple(x.shape), model_kwargs={"y": y0}, **kw).clone(),
            fresh_m(x, t, yd).clone(), fresh_m(x, t, dict(yd, uncond=True)).clone())
    m = model_of(T40)
    g = ClassifierFreeSampleModel(m)
    for mode in (cr.SEED_TEXT, cr.TEXT, cr.TEXT_SEED):
        g(x, t, keys_of(mode, yd, B))
        df.p_sample_loop(g, tuple(x.shape), model_kwargs={"y": keys_of(mode, yd, B)}, **kw)
        got = (g(x, t, y0), df.p_sample_loop(g, tuple(x.shape), model_kwargs={"y": y0}, **kw))
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), mode
        g(x, t, keys_of(mode, yd, B))
        assert torch.equal(m(x, t, yd), want[2]) and torch.equal(m(x, t, dict(yd, uncond=True)), want[3]), mode
    assert torch.equal(g(x, t, dict(y0, guidance_drop="both")), want[0])
