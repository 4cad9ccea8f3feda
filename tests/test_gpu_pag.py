"""Perturbed-attention guidance on the GPU (y['pag_scale'] / y['pag_layers'], gdx_set_attention_guidance, gdx_attention_identity;
include/gdx.h): the copy kernel, every encoder layer of every row group through the taps, guided forwards and loops against the
fixture the reference's own classes wrote (tests/golden/forward_pag.npz), the empty mask, every in-library loop against its
step-wise and block-wise twins, the features of a two-group guided call under GDX_PAG_ONLY, the refusals, and a model trained
without condition dropout.

Shapes: the cases of the fixture (J = 16, d = 128, 4 heads, ff 192, 2 or 3 layers, B = 3, T = 20); the kernel at rows 1 / 63 / 257
(one partial block, one block, more than one) and d 128 / 384 / 768.  Need an MI355X."""
import functools

import numpy as np
import pytest
import torch

import pag_restatement as pr
from conftest import load_golden, rel_err
from gesturediffusion_amd import _lib, numerics
from gesturediffusion_amd import engine as E
from gesturediffusion_amd._lib import GDX_CFG, GDX_SAMPLER_P, GdxError
from gesturediffusion_amd.diffusion.gaussian_diffusion import GaussianDiffusion
from gesturediffusion_amd.model.cfg_sampler import ClassifierFreeSampleModel
from gesturediffusion_amd.model.pag_sampler import PerturbedAttentionSampleModel
from test_gpu_parity import build_model, dev
from test_gpu_text import diffusion, on_dev

pytestmark = pytest.mark.gpu
DTYPES = ("fp32", "fp16", "bf16")
V2, V3, OLD = "v2_l2_m1", "v2_l3_m02", "old_l2_m0"
ONLY_W, CFG_S, CFG_W = (3.0, 0.5, 1.25), (1.5, 2.5, 0.75), (3.0, -1.0, 2.25)      # the fixture's loops use the same
MID = (300, 700)                      # of t = [7, 993, 500] only the last sample is guided


@functools.lru_cache(maxsize=None)
def golden():
    return load_golden("forward_pag.npz")


@functools.lru_cache(maxsize=None)
def case(name):
    """(cfg, weights, x, t, y, layers) on the host; shared, read only."""
    return pr.case(golden(), name)


def model_of(name, dtype="fp32", cond_mask_prob=0.1):
    cfg, sd = case(name)[:2]
    m = build_model(cfg["arch"], cfg, sd, cond_mask_prob=cond_mask_prob)
    m.compute_dtype = dtype
    return m


def inputs(name):
    cfg, sd, x, t, y, layers = case(name)
    return x.to(dev()), t.to(dev()), on_dev(y), layers


def wrap(kind, m):
    return PerturbedAttentionSampleModel(m) if kind == pr.ONLY else ClassifierFreeSampleModel(m)


def keys_of(kind, yd, layers):
    """y of the wrapper of `kind`, with different scales per sample."""
    if kind == pr.ONLY:
        return dict(yd, pag_scale=torch.tensor(ONLY_W, device=dev()), pag_layers=layers)
    return dict(yd, scale=torch.tensor(CFG_S, device=dev()), pag_scale=torch.tensor(CFG_W, device=dev()), pag_layers=layers)


def factor_of(kind):
    """The rule's triangle factor at the worst sample of keys_of's scales."""
    if kind == pr.ONLY:
        return max(numerics.pag_factor(w) for w in ONLY_W)
    return max(numerics.pag_factor(w, s) for s, w in zip(CFG_S, CFG_W))


def reference_of(kind, name):
    """The rule in float64 on the reference's own F, P, U."""
    g = golden()
    p = {k: torch.from_numpy(g[f"{name}.{k}"]).double() for k in "FPU"}
    if kind == pr.ONLY:
        return pr.compose_only(p, 1.0 + torch.tensor(ONLY_W, dtype=torch.float64))
    return pr.compose_cfg(p, torch.tensor(CFG_S, dtype=torch.float64), torch.tensor(CFG_W, dtype=torch.float64))


# --------------------------------------------------------------------------------------------------------------- 1. kernel
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_attention_identity_copies_v_and_nothing_else(dtype):
    """ctx == the V third bit for bit at every (rows, d); Q and K hold a value that is nowhere in V, and the canary behind ctx
    stays.  fp16 and bf16 run the same 2-byte instance."""
    ints = {4: torch.int32, 2: torch.int16}[torch.empty(0, dtype=dtype).element_size()]
    gen = torch.Generator().manual_seed(3)
    for rows in (1, 63, 257):
        for d in (128, 384, 768):
            qkv = torch.full((rows, 3 * d), 1234.0, dtype=dtype)
            v = torch.randn(rows, d, generator=gen).to(dtype)
            assert not bool((v == 1234.0).any())
            qkv[:, 2 * d:] = v
            buf = torch.full((rows * d + 64,), -777.0, dtype=dtype, device=dev())
            ctx = buf[:rows * d].view(rows, d)
            E.attention_identity(qkv.to(dev()), ctx)
            assert torch.equal(ctx.view(ints).cpu(), v.view(ints)), (rows, d)
            assert bool((buf[rows * d:] == -777.0).all()), (rows, d)
    qkv, ctx = torch.zeros(4, 3 * 128 + 1, dtype=dtype, device=dev()), torch.zeros(4, 128, dtype=dtype, device=dev())
    with pytest.raises(GdxError, match="16-byte aligned"):
        E.attention_identity(qkv.flatten()[1:1 + 4 * 384].view(4, 384), ctx)


# ----------------------------------------------------------------------------------------------------------------- 2. taps
def _taps(eng, groups, B, S, d, L):
    return [eng.tap(l, groups * B * S, d, dev()).view(groups, B, S, d).clone() for l in range(L + 1)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", [pr.ONLY, pr.CFG])
@pytest.mark.parametrize("name", [V3, OLD])
def test_every_layer_of_every_group(name, kind, dtype):
    """Tap l of group P against the float64 restatement of layer l - 1 alone (identity attention where masked) applied to the
    handle's own tap l - 1, within numerics.FORWARD_TOL; group F's taps are a GDX_COND forward's and group U's a GDX_UNCOND
    forward's bit for bit: samples do not depend on their batch position, and only P's rows are perturbed."""
    cfg, sd, xh, th_, yh, layers = case(name)
    x, t, yd, _ = inputs(name)
    B, S, d, L, H = x.shape[0], x.shape[3] + 1, cfg["latent_dim"], cfg["num_layers"], cfg["num_heads"]
    m = model_of(name, dtype)
    eng = m._get_engine(dev())
    eng.keep_taps(True)
    G = 2 if kind == pr.ONLY else 3
    wrap(kind, m)(x, t, keys_of(kind, yd, layers))
    taps = _taps(eng, G, B, S, d, L)
    p64 = {k: v.double() for k, v in sd.items()}
    for l in range(1, L + 1):
        src = taps[l - 1][1].cpu().double().permute(1, 0, 2)                      # [S, B, d]
        with torch.no_grad():
            want = pr.layer(p64, l - 1, src, H, (l - 1) in layers).permute(1, 0, 2)
            plain = pr.layer(p64, l - 1, src, H, False).permute(1, 0, 2)
        err = rel_err(taps[l][1].cpu(), want)
        print(f"[pag-measure] {name} kind {kind} {dtype} layer {l - 1} group P: rel err {err:.2e}")
        assert err < numerics.FORWARD_TOL[dtype], (l, err)
        if (l - 1) in layers:                                                     # the perturbation is no rounding error
            assert rel_err(plain, want) > 10 * numerics.FORWARD_TOL[dtype]
    m(x, t, yd)                                                                   # GDX_COND on the same handle
    cond = _taps(eng, 1, B, S, d, L)
    for l in range(L + 1):
        assert torch.equal(taps[l][0], cond[l][0]), ("F", l)
    assert torch.equal(taps[0][1], taps[0][0])                                    # P's conditioning rows are F's
    if kind == pr.CFG:
        m(x, t, dict(yd, uncond=True))
        un = _taps(eng, 1, B, S, d, L)
        for l in range(L + 1):
            assert torch.equal(taps[l][2], un[l][0]), ("U", l)
    eng.keep_taps(False)


# ------------------------------------------------------------------------------------------------------------- 3. forwards
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", [pr.ONLY, pr.CFG])
@pytest.mark.parametrize("name", sorted(pr.CASES))
def test_forwards_vs_reference_fixture(name, kind, dtype):
    """Both wrappers' forward against the rule on the reference's own passes, within the mode's stated tolerance times the
    rule's triangle factor; with the mid interval only the last sample is guided, the others are F."""
    x, t, yd, layers = inputs(name)
    m = model_of(name, dtype)
    g = wrap(kind, m)
    y = keys_of(kind, yd, layers)
    got = g(x, t, y).clone()
    tol = numerics.stated_tolerance(dtype, None, loop=False) * factor_of(kind)
    err = rel_err(got.cpu(), reference_of(kind, name))
    print(f"[pag-measure] forward {name} kind {kind} {dtype}: rel err {err:.2e} (bound {tol:.2e})")
    assert err < tol
    F = m(x, t, yd).clone()
    assert rel_err(F.cpu(), golden()[f"{name}.F"]) < numerics.FORWARD_TOL[dtype]
    lim = g(x, t, dict(y, guidance_interval=MID))
    assert torch.equal(lim[:2], F[:2]) and torch.equal(lim[2], got[2])
    eng = m._get_engine(dev())
    before = eng.forward_samples()
    g(x, t, y)
    assert eng.forward_samples() - before == (2 if kind == pr.ONLY else 3) * x.shape[0]


def test_forward_is_the_rule_on_plain_passes_bit_for_bit():
    """fp32: the guided forward equals the rule in torch's separate ops on the handle's own F (GDX_COND), U (GDX_UNCOND) and P,
    which the kind-1 call at scale 0 returns (P + 0 * (F - P))."""
    x, t, yd, layers = inputs(V2)
    m = model_of(V2)
    F, U = m(x, t, yd).clone(), m(x, t, dict(yd, uncond=True)).clone()
    P = PerturbedAttentionSampleModel(m)(x, t, dict(yd, pag_scale=torch.full((3,), -1.0, device=dev()), pag_layers=layers)).clone()
    assert not torch.equal(P, F)
    p = {"F": F, "P": P, "U": U}
    y1, y2 = keys_of(pr.ONLY, yd, layers), keys_of(pr.CFG, yd, layers)
    assert torch.equal(PerturbedAttentionSampleModel(m)(x, t, y1), pr.compose_only(p, 1.0 + y1["pag_scale"]))
    assert torch.equal(ClassifierFreeSampleModel(m)(x, t, y2), pr.compose_cfg(p, y2["scale"], y2["pag_scale"]))
    # the default layer is the middle one
    mid = PerturbedAttentionSampleModel(m)(x, t, {k: v for k, v in y1.items() if k != "pag_layers"})
    assert torch.equal(mid, PerturbedAttentionSampleModel(m)(x, t, dict(y1, pag_layers=[1])))


# ----------------------------------------------------------------------------------------------------------- 4. empty mask
@pytest.mark.parametrize("dtype", DTYPES)
def test_an_empty_mask_gives_the_conditional_forward(dtype):
    """layer_mask = 0 through the engine (y['pag_layers'] must not be empty): P is F, so P + s * 0 is the GDX_COND forward."""
    x, t, yd, _ = inputs(V2)
    m = model_of(V2, dtype)
    want = m(x, t, yd).clone()
    eng = m._get_engine(dev())
    eng.set_attention_guidance(_lib.GDX_PAG_ONLY, 0)
    eng.prepare(x.shape[0], x.shape[3])
    eng.set_condition(yd["seed"], yd["mfcc"])
    got = eng.forward(x, t, GDX_CFG, torch.tensor(ONLY_W, device=dev()))
    assert torch.equal(got.view_as(want), want)
    eng.set_attention_guidance()


# ---------------------------------------------------------------------------------------------------------------- 5. loops
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", [pr.ONLY, pr.CFG])
def test_p_loop_vs_reference_fixture(kind, dtype):
    """p_sample_loop on [20] steps with the recorded tape against the reference's own loop around the composed passes."""
    gold = golden()
    tag = "only" if kind == pr.ONLY else "cfg"
    x, t, yd, layers = inputs(V2)
    g = wrap(kind, model_of(V2, dtype))
    tape = torch.from_numpy(gold[f"{V2}.{tag}_p20.tape"]).to(dev())
    y = keys_of(kind, yd, layers)
    assert np.array_equal(gold[f"{V2}.{tag}_w"], np.float32(ONLY_W if kind == pr.ONLY else CFG_W))
    r = diffusion(pr.RESPACING).p_sample_loop(g, tuple(x.shape), noise_tape=tape, clip_denoised=False, model_kwargs={"y": y}, progress=False)
    tol = numerics.LOOP_TOL[dtype] * factor_of(kind)
    err = rel_err(r.cpu(), gold[f"{V2}.{tag}_p20.out"])
    print(f"[pag-measure] p20 loop kind {kind} {dtype}: rel err {err:.2e} (bound {tol:.2e})")
    assert err < tol


def _loops(df, dfd, g, x, y, fused):
    """Every in-library loop on the guided model g, each as (name, result tensors)."""
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


@pytest.mark.parametrize("kind", [pr.ONLY, pr.CFG])
@pytest.mark.parametrize("name", [V2, OLD])
def test_fused_loops_equal_their_stepwise_and_blockwise_twins(name, kind, monkeypatch):
    """Each fused loop equals its step-by-step Python twin (fused=False) and the same loop issued in blocks of three steps, bit for
    bit; kind 1 also under graph replay; the progressive generator ends on the fused loop's bits."""
    x, t, yd, layers = inputs(name)
    m = model_of(name)
    g = wrap(kind, m)
    df, dfd = diffusion("ddim10"), diffusion("logsnr10")
    y = keys_of(kind, yd, layers)
    fused = {k: [v.clone() for v in r] for k, r in _loops(df, dfd, g, x, y, True)}
    step = {k: [v.clone() for v in r] for k, r in _loops(df, dfd, g, x, y, False)}
    whole = GaussianDiffusion._issue_blocks
    monkeypatch.setattr(GaussianDiffusion, "_issue_blocks",
                        staticmethod(lambda n, device, progress, issue, block=None: whole(n, device, False, issue, block=3)))
    blocks = {k: [v.clone() for v in r] for k, r in _loops(df, dfd, g, x, y, True)}
    monkeypatch.undo()
    assert len(fused) == 8
    for k in fused:
        for a, b, c in zip(fused[k], step[k], blocks[k]):
            assert bool(torch.isfinite(a).all()) and torch.equal(a, b) and torch.equal(a, c), k
    plain = df.p_sample_loop(m, tuple(x.shape), clip_denoised=False, progress=False, rng="philox", philox_seed=5, model_kwargs={"y": yd})
    assert not torch.equal(plain, fused["p"][0])
    last = None
    for last in df.ddim_sample_loop_progressive(g, tuple(x.shape), noise=x.clone(), clip_denoised=False, model_kwargs={"y": y}, eta=0.0):
        pass
    assert torch.equal(last["sample"], fused["ddim"][0])
    if kind == pr.ONLY:
        # graph replay: inpainting keeps the loop off the token-major path, ten steps reach the capture
        mask = torch.zeros_like(x, dtype=torch.bool)
        mask[..., :5] = True
        yi = dict(y, inpainting_mask=mask, inpainted_motion=0.5 * x)
        kw = dict(clip_denoised=False, progress=False, rng="philox", philox_seed=5, model_kwargs={"y": yi})
        eager = df.p_sample_loop(g, tuple(x.shape), **kw).clone()
        eng = m._get_engine(dev())
        eng.set_graph_replay(True)
        try:
            replay = df.p_sample_loop(g, tuple(x.shape), **kw).clone()
        finally:
            eng.set_graph_replay(False)
        assert torch.equal(replay, eager)


# ------------------------------------------------------------------------------------------------- 6. features under kind 1
def test_interval_rescale_refresh_cache_and_parallel_under_kind_1():
    x, t, yd, layers = inputs(V2)
    B, L = x.shape[0], 2
    m = model_of(V2)
    g = PerturbedAttentionSampleModel(m)
    eng = m._get_engine(dev())
    y = keys_of(pr.ONLY, yd, layers)
    df = diffusion(pr.RESPACING)
    n = df.num_timesteps
    shape = tuple(x.shape)
    kw = dict(clip_denoised=False, progress=False, rng="philox", philox_seed=7)
    # interval: an unguided step runs B samples
    flags = df.guided_steps(MID)
    assert 0 < sum(flags) < len(flags)
    before = eng.forward_samples()
    df.p_sample_loop(g, shape, model_kwargs={"y": dict(y, guidance_interval=MID)}, **kw)
    assert eng.forward_samples() - before == sum(2 * B if f else B for f in flags)
    # rescale: out = fl32(g * f), f within one fp32 ulp of an fp64 evaluation of phi * std(F) / std(g) + (1 - phi), c = F
    phi = 0.5
    comp, F = g(x, t, y).clone(), m(x, t, yd).clone()
    out = g(x, t, dict(y, guidance_rescale=phi))
    c64, g64 = F.double().reshape(B, -1), comp.double().reshape(B, -1)
    f32 = (phi * c64.std(dim=1, unbiased=False) / g64.std(dim=1, unbiased=False) + (1 - phi)).float()
    for b in range(B):
        cands = [f32[b], torch.nextafter(f32[b], f32[b] + 1), torch.nextafter(f32[b], f32[b] - 1)]
        assert any(bool(torch.equal(out[b], comp[b] * c)) for c in cands), b
    assert not torch.equal(out, comp)
    runs = [df.p_sample_loop(g, shape, model_kwargs={"y": dict(y, guidance_rescale=phi)}, fused=f, **kw).clone() for f in (True, False)]
    assert torch.equal(runs[0], runs[1])
    # refresh and layer cache: the counters follow the plan, and the first (refresh, full) step has the bits of the loop without
    coef, tmap = df.coef_table(GDX_SAMPLER_P, dev(), 0.0), df._timestep_map()

    def first_step(yy):
        state = x.clone()
        e, mode, scale, mask, motion = df._native_loop_setup(g, state, {"y": yy})
        e.sample_loop(state, GDX_SAMPLER_P, mode, coef, tmap, n - 1, scale=scale, philox_seed=7, run_steps=1, k_base=0)
        return state
    base = first_step(y)
    for extra in (dict(guidance_refresh=2), dict(layer_cache=(2, 1)), dict(guidance_refresh=2, layer_cache=(2, 1))):
        yy = dict(y, **extra)
        assert torch.equal(first_step(yy), base), extra
        s0, l0 = eng.forward_samples(), eng.forward_layer_samples()
        r = df.p_sample_loop(g, shape, model_kwargs={"y": yy}, **kw)
        assert bool(torch.isfinite(r).all())
        every = extra.get("guidance_refresh", 1)
        rows = [2 * B if c == "refresh" else B for c in df.guidance_plan(None, every)]
        lc = df.layer_cache_plan(extra.get("layer_cache", (1, 0)), None, every, guided=True)
        assert eng.forward_samples() - s0 == sum(rows), extra
        assert eng.forward_layer_samples() - l0 == sum(r_ * (L if c == "full" else 1) for r_, c in zip(rows, lc)), extra
    # the parallel loop at tolerance 0 is the sequential loop
    seq = df.p_sample_loop(g, shape, model_kwargs={"y": y}, **kw)
    par = df.parallel_sample_loop(g, shape, clip_denoised=False, model_kwargs={"y": y}, window=4, tolerance=0.0, philox_seed=7)
    assert torch.equal(par, seq)


# ------------------------------------------------------------------------------------------------------------- 7. refusals
def test_refusals_on_the_device():
    x, t, yd, layers = inputs(V2)
    B = x.shape[0]
    m = model_of(V2)
    g = ClassifierFreeSampleModel(m)
    df = diffusion(pr.RESPACING)
    n = df.num_timesteps
    y = keys_of(pr.CFG, yd, layers)
    state = x.clone()
    eng, mode, scale, mask, motion = df._native_loop_setup(g, state, {"y": y})
    assert mode == GDX_CFG and tuple(scale.shape) == (2, B)
    coef, tmap = df.coef_table(GDX_SAMPLER_P, dev(), 0.0), df._timestep_map()
    before = eng.forward_samples()
    eng.set_guidance_refresh(2)
    with pytest.raises(GdxError, match="guidance refresh"):
        eng.sample_loop(state, GDX_SAMPLER_P, mode, coef, tmap, n - 1, scale=scale, philox_seed=1)
    eng.set_guidance_refresh(1)
    eng.set_layer_cache(2, 1)
    with pytest.raises(GdxError, match="layer cache"):
        eng.sample_loop(state, GDX_SAMPLER_P, mode, coef, tmap, n - 1, scale=scale, philox_seed=1)
    eng.set_layer_cache(1, 0)
    planes = torch.zeros(3, B, *x.shape[1:], device=dev())
    with pytest.raises(GdxError, match="not supported by the parallel loop"):
        eng.parallel_loop(planes, GDX_SAMPLER_P, mode, coef, tmap, np.zeros(n), n - 1, scale=scale)
    assert eng.forward_samples() == before and torch.equal(state, x)
    for extra, says in ((dict(guidance_refresh=2), "guidance_refresh"), (dict(layer_cache=(2, 1)), "layer_cache")):
        with pytest.raises(ValueError, match=says):
            df.p_sample_loop(g, tuple(x.shape), model_kwargs={"y": dict(y, **extra)}, progress=False)
    with pytest.raises(ValueError, match="parallel_sample_loop"):
        df.parallel_sample_loop(g, tuple(x.shape), model_kwargs={"y": y}, window=2)
    assert eng.forward_samples() == before
    # a refused setter call leaves the handle as it was
    want = g(x, t, y).clone()
    lib = eng.lib
    assert lib.gdx_set_attention_guidance(eng.handle, 3, 1) != 0 and b"unknown kind" in lib.gdx_last_error()
    assert lib.gdx_set_attention_guidance(eng.handle, 2, 1 << 2) != 0 and b"beyond num_layers" in lib.gdx_last_error()
    with pytest.raises(GdxError, match="beyond num_layers"):
        eng.set_attention_guidance(_lib.GDX_PAG_ONLY, 1 << 5)
    assert torch.equal(g(x, t, y), want)
    # a compose mode other than JOINT: a guided call is refused, the others run
    import text_restatement as tr
    from gesturediffusion_amd.utils.init import init_state_dict, synthetic_inputs
    cfg = tr.text_cfg(40, 32)
    tm = tr.build_text_model(cfg, init_state_dict(cfg, seed=4, perturb=True)).to(dev())
    xs, seedp, mfcc, text = (v.to(dev()) for v in synthetic_inputs(cfg, 2, 20, seed=6))
    ts = torch.tensor([7, 500], device=dev())
    ty = {"seed": seedp, "mfcc": mfcc, "text_embed": text}
    want = tm(xs, ts, ty).clone()
    te = tm._get_engine(dev())
    te.set_guidance_compose(_lib.GDX_GUIDE_TEXT, attention=(_lib.GDX_PAG_ONLY, 1))
    te.prepare(2, 20)
    te.set_condition(seedp, mfcc, text=text)
    before = te.forward_samples()
    with pytest.raises(GdxError, match="four are not supported"):
        te.forward(xs, ts, GDX_CFG, torch.ones(2, device=dev()))
    assert te.forward_samples() == before
    assert torch.equal(te.forward(xs, ts).view_as(want), want)
    with pytest.raises(ValueError, match="exclude each other"):
        ClassifierFreeSampleModel(tm)(xs, ts, dict(ty, scale=torch.ones(2, device=dev()), pag_scale=torch.ones(2, device=dev()),
                                                   guidance_drop="text"))
    assert torch.equal(tm(xs, ts, ty), want)


# --------------------------------------------------------------------------------------- 8. a model without condition dropout
def test_a_model_trained_without_dropout_samples_under_pag():
    x, t, yd, layers = inputs(V2)
    m = model_of(V2, cond_mask_prob=0.0)
    with pytest.raises(AssertionError, match="has not been trained with no conditions"):
        ClassifierFreeSampleModel(m)
    g = PerturbedAttentionSampleModel(m)
    assert isinstance(g, ClassifierFreeSampleModel)
    y = keys_of(pr.ONLY, yd, layers)
    r = diffusion("ddim10").p_sample_loop(g, tuple(x.shape), clip_denoised=False, progress=False, rng="philox", philox_seed=5,
                                          model_kwargs={"y": y})
    want = diffusion("ddim10").p_sample_loop(PerturbedAttentionSampleModel(model_of(V2)), tuple(x.shape), clip_denoised=False,
                                             progress=False, rng="philox", philox_seed=5, model_kwargs={"y": y})
    assert bool(torch.isfinite(r).all()) and torch.equal(r, want)
    for bad, says in ((dict(scale=torch.ones(3, device=dev())), "belongs to classifier-free guidance"),
                      (dict(pag_layers=[2]), "distinct encoder layers"), (dict(pag_layers=[]), "non-empty")):
        with pytest.raises(ValueError, match=says):
            g(x, t, dict(y, **bad))
    with pytest.raises(ValueError, match=r"needs y\['pag_scale'\]"):
        g(x, t, yd)
    with pytest.raises(ValueError, match="needs a PerturbedAttentionSampleModel"):
        m(x, t, y)
