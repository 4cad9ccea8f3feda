"""use_text models on the GPU: MDM(use_text=True) conditioned through gdx_set_condition_text against what the reference's own
class computed (tests/golden/forward_text_tiny.npz, tools/make_golden_text.py) and against the CPU restatement
(tests/text_restatement.py) -- forwards in every compute mode, the layout of the condition token, the guided loop and the chunk
driver, the agreement of the loop paths, the conditioning cache, the packed image and the CLI.  Need an MI355X.

Tolerances: gesturediffusion_amd/numerics.py (FORWARD_TOL / LOOP_TOL, guidance_factor, stated_tolerance)."""
import functools

import numpy as np
import pytest
import torch

import text_restatement as tr
from conftest import load_golden, rel_err
from gesturediffusion_amd import numerics
from gesturediffusion_amd._lib import GdxError
from gesturediffusion_amd.model.cfg_sampler import ClassifierFreeSampleModel
from test_gpu_parity import dev

pytestmark = pytest.mark.gpu
T64 = "mdm_128_t64"


@functools.lru_cache(maxsize=None)
def golden():
    return load_golden("forward_text_tiny.npz")


@functools.lru_cache(maxsize=None)
def case(name):
    """(cfg, weights, x, t, y) of a fixture case on the host; shared, read only."""
    return tr.case(golden(), name)


def model_of(name, dtype="fp32", seed=None):
    from gesturediffusion_amd.utils.init import init_state_dict
    cfg, sd = case(name)[:2]
    m = tr.build_text_model(cfg, sd if seed is None else init_state_dict(cfg, seed=seed, perturb=True)).to(dev())
    m.compute_dtype = dtype
    return m


def on_dev(y):
    return {k: v.to(dev()) if isinstance(v, torch.Tensor) else v for k, v in y.items()}


def diffusion(resp):
    from gesturediffusion_amd.diffusion import gaussian_diffusion as gd
    from gesturediffusion_amd.diffusion.respace import SpacedDiffusion, space_timesteps
    betas = gd.get_named_beta_schedule("cosine", 1000)
    return SpacedDiffusion(use_timesteps=space_timesteps(1000, resp, betas=betas), betas=betas,
                           model_mean_type=gd.ModelMeanType.START_X, model_var_type=gd.ModelVarType.FIXED_SMALL,
                           loss_type=gd.LossType.MSE)


# ------------------------------------------------------------------------------------------------------------------ forwards
@pytest.mark.parametrize("dtype", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("name", sorted(tr.CASES))
def test_forwards_vs_reference_golden(name, dtype):
    """Conditional and unconditional forwards of both cases (text_dim 64 / clip_dim 512, B = 2; text_dim 40 / clip_dim 32,
    B = 3: no multiple of a tile, clip_dim one K pad) against the reference's, fp32 at FORWARD_TOL, 16-bit at the stated one."""
    g = golden()
    cfg, sd, x, t, y = case(name)
    m = model_of(name, dtype)
    tol = numerics.FORWARD_TOL["fp32"] if dtype == "fp32" else numerics.stated_tolerance(dtype, loop=False)
    yd = on_dev(y)
    for tag, yy in (("cond", yd), ("uncond", dict(yd, uncond=True))):
        out = m(x.to(dev()), t.to(dev()), yy).cpu()
        err = rel_err(out, g[f"{name}.{tag}.out"])
        print(f"[text-measure] forward {name} {tag} {dtype}: rel err {err:.2e}")
        assert out.shape == x.shape and err < tol, (tag, err)


def test_forward_batch_of_one_vs_restatement():
    """B = 1 (where the reference's .squeeze(0) breaks its own concatenation) against the CPU restatement, cond and uncond; a
    float64 text_embed is converted like a float64 seed."""
    cfg, sd, x, t, y = case(T64)
    one = {k: v[1:2] for k, v in y.items()}
    m = model_of(T64)
    for extra in ({}, {"uncond": True}):
        with torch.no_grad():
            want = tr.forward(sd, cfg, x[1:2], t[1:2], dict(one, **extra))
        yd = on_dev(dict(one, **extra))
        out = m(x[1:2].to(dev()), t[1:2].to(dev()), yd)
        assert rel_err(out.cpu(), want) < numerics.FORWARD_TOL["fp32"]
        assert torch.equal(m(x[1:2].to(dev()), t[1:2].to(dev()), dict(yd, text_embed=yd["text_embed"].double())), out)


# --------------------------------------------------------------------------------------------------------- token-0 layout
def token0(m, x, t, y):
    """(token 0 of every sample [B, d], the whole encoder input [B, S, d]) of one fp32 forward, through tap 0; RoPE at
    position 0 is the identity, so token 0 is emb_t + the condition row itself."""
    eng = m._get_engine(dev())
    eng.keep_taps(True)
    m(x, t, y)
    B, S, d = x.shape[0], x.shape[3] + 1, m.latent_dim
    tap = eng.tap(0, 2 * B * S, d, dev())[: B * S].view(B, S, d).clone()
    return tap[:, 0], tap


@pytest.mark.parametrize("name", sorted(tr.CASES))
def test_token0_is_text_columns_then_seed_columns(name):
    cfg, sd, x, t, y = case(name)
    td, B = cfg["text_dim"], x.shape[0]
    m = model_of(name)
    xd, tdev, yd = x.to(dev()), t.to(dev()), on_dev(y)
    base, base_all = token0(m, xd, tdev, yd)
    b = B - 1
    text2, seed2 = yd["text_embed"].clone(), yd["seed"].clone()
    text2[b] += 1.0
    seed2[b] -= 1.0
    got, got_all = token0(m, xd, tdev, dict(yd, text_embed=text2))
    assert torch.equal(got[:b], base[:b]) and torch.equal(got_all[:b], base_all[:b])          # the other samples: every bit
    assert torch.equal(got[b, td:], base[b, td:]) and bool((got[b, :td] != base[b, :td]).all())
    got, got_all = token0(m, xd, tdev, dict(yd, seed=seed2))
    assert torch.equal(got[:b], base[:b]) and torch.equal(got_all[:b], base_all[:b])
    assert torch.equal(got[b, :td], base[b, :td]) and bool((got[b, td:] != base[b, td:]).all())
    # against the fp64 restatement, the condition part and the timestep part apart
    rows, cond = tr.token0_rows(sd, cfg, t, y["seed"], y["text_embed"])
    err = float((base.cpu().double() - rows).abs().max() / rows.abs().max())
    print(f"[text-measure] token 0 {name}: max err / max|row| {err:.2e}")
    assert err < 1e-5
    # uncond: [embed_text.bias | seed_embed.bias] whatever the text and the seed are
    un = token0(m, xd, tdev, dict(yd, uncond=True))[0]
    assert torch.equal(token0(m, xd, tdev, dict(yd, uncond=True, text_embed=text2, seed=seed2))[0], un)
    want = tr.token0_rows(sd, cfg, t, y["seed"], y["text_embed"], uncond=True)[0]
    assert float((un.cpu().double() - want).abs().max() / want.abs().max()) < 1e-5
    assert not torch.equal(un, base)
    m._get_engine(dev()).keep_taps(False)


# ------------------------------------------------------------------------------------------------------ loops and chunks
def test_guided_loop_vs_reference_golden():
    """p_sample_loop on [20] steps under ClassifierFreeSampleModel at scale 2.5 with the recorded noise tape, fused."""
    g = golden()
    cfg, sd, x, t, y = case(T64)
    m = ClassifierFreeSampleModel(model_of(T64))
    tape = torch.from_numpy(g[T64 + ".cfg_p20.tape"]).to(dev())
    yd = dict(on_dev(y), scale=torch.ones(x.shape[0], device=dev()) * tr.SCALE)
    r = diffusion(tr.RESPACING).p_sample_loop(m, tuple(x.shape), noise_tape=tape, clip_denoised=False, model_kwargs={"y": yd},
                                              progress=False)
    err = rel_err(r.cpu(), g[T64 + ".cfg_p20.out"])
    print(f"[text-measure] guided p20 loop: rel err {err:.2e}")
    assert err < numerics.LOOP_TOL["fp32"] * numerics.guidance_factor(tr.SCALE)


def test_chunk_driver_vs_reference_golden():
    """sample_chunks with a text per chunk against the reference's chunk statements: seed poses chained on the device."""
    from gesturediffusion_amd.sample.generate import sample_chunks
    g = golden()
    cfg, sd, x, t, y = case(T64)
    m = ClassifierFreeSampleModel(model_of(T64))
    texts, mfccs, tapes = (torch.from_numpy(g[f"{T64}.chunks.{k}"]).to(dev()) for k in ("text", "mfcc", "tape"))
    outs = sample_chunks(m, diffusion(tr.RESPACING), y["seed"].to(dev()), lambda c: mfccs[c], texts.shape[0], x.shape[3],
                         cfg["seed_poses"], guidance_param=tr.SCALE, sampler="p", noise_tapes=list(tapes),
                         text_of_chunk=lambda c: texts[c])
    for c, o in enumerate(outs):
        err = rel_err(o.cpu(), g[T64 + ".chunks.out"][c])
        print(f"[text-measure] chunk {c}: rel err {err:.2e}")
        assert err < numerics.LOOP_TOL["fp32"] * numerics.guidance_factor(tr.SCALE), c


def test_loop_paths_agree_bit_for_bit():
    """The in-library loops condition through _native_loop_setup, the step-wise ones through the model's forward on every step
    (with the conditioning cache): the same bits, for the guided ancestral loop on Philox noise and for one DPM++ 2M loop."""
    cfg, sd, x, t, y = case(T64)
    inner = model_of(T64)
    m = ClassifierFreeSampleModel(inner)
    shape = tuple(x.shape)
    yd = dict(on_dev(y), scale=torch.ones(x.shape[0], device=dev()) * tr.SCALE)
    runs = []
    for fused in (True, False):
        runs.append(diffusion(tr.RESPACING).p_sample_loop(m, shape, clip_denoised=False, model_kwargs={"y": yd}, progress=False,
                                                          rng="philox", philox_seed=5, fused=fused).clone())
        # between the two, the same handle is conditioned on another text: a cache that missed it would show below
        inner(x.to(dev()), t.to(dev()), dict(on_dev(y), text_embed=yd["text_embed"] + 1.0))
    assert torch.equal(runs[0], runs[1]) and bool(torch.isfinite(runs[0]).all())
    other = diffusion(tr.RESPACING).p_sample_loop(m, shape, clip_denoised=False, progress=False, rng="philox", philox_seed=5,
                                                  model_kwargs={"y": dict(yd, text_embed=yd["text_embed"] + 1.0)})
    assert not torch.equal(other, runs[0])                                   # the text reaches the fused loop
    xT = x.to(dev())
    dpm = [diffusion("logsnr10").dpm_solver_sample_loop(inner, shape, noise=xT.clone(), clip_denoised=False, progress=False,
                                                        model_kwargs={"y": on_dev(y)}, order=2, fused=fused).clone()
           for fused in (True, False)]
    assert torch.equal(dpm[0], dpm[1]) and bool(torch.isfinite(dpm[0]).all())


# ------------------------------------------------------------------------------------------------------ conditioning cache
def test_conditioning_cache_covers_the_text_tensor():
    cfg, sd, x, t, y = case(T64)
    m = model_of(T64)
    xd, tdev, yd = x.to(dev()), t.to(dev()), on_dev(y)                       # one seed and one mfcc tensor throughout
    text = yd["text_embed"]
    out = m(xd, tdev, yd).clone()
    other = text.clone() + 0.5
    out_other = m(xd, tdev, dict(yd, text_embed=other)).clone()
    assert not torch.equal(out_other, out)                                   # another tensor: re-conditioned
    assert torch.equal(m(xd, tdev, yd), out)                                 # and back
    # the same tensor again reuses the cache: an edit that bypasses the version counter goes unseen ...
    text.data.add_(0.5)
    assert torch.equal(text, other) and torch.equal(m(xd, tdev, yd), out)
    # ... until an in-place edit bumps the counter: now the output is the one of these values
    text.mul_(1.0)
    assert torch.equal(m(xd, tdev, yd), out_other)
    text.copy_(y["text_embed"])                                              # the first values again, the counter bumped
    assert torch.equal(m(xd, tdev, yd), out)
    # the errors y['seed'] gets: a host tensor has no fallback, a missing key is the reference's KeyError
    with pytest.raises(GdxError, match="text_embed"):
        m(xd, tdev, dict(yd, text_embed=text.cpu()))
    with pytest.raises(KeyError, match="text"):
        m(xd, tdev, {k: v for k, v in yd.items() if k != "text_embed"})
    with pytest.raises(ValueError, match="clip_dim"):
        m(xd, tdev, dict(yd, text_embed=text[:, :-1]))
    m.set_text_encoder(lambda texts: torch.stack([other[int(s)] for s in texts]))
    assert torch.equal(m(xd, tdev, {"seed": yd["seed"], "mfcc": yd["mfcc"], "text": ["0", "1"]}), out_other)


# ------------------------------------------------------------------------------------------------------------ packed image
def _fwd(m, name):
    cfg, sd, x, t, y = case(name)
    return m(x.to(dev()), t.to(dev()), on_dev(y)).clone()


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_packed_image_roundtrip_text(dtype):
    a, b = model_of(T64, dtype), model_of(T64, dtype, seed=32)
    out_a, out_b = _fwd(a, T64), _fwd(b, T64)
    assert not torch.equal(out_a, out_b)
    b.load_packed(a.export_packed(dev()), dev())
    assert torch.equal(_fwd(b, T64), out_a)


def test_packed_image_text_and_no_text_refuse_each_other():
    """A handle only takes an image of its own configuration, text_dim and clip_dim included; a refused image leaves it as it
    was.  An image with the header of before the two fields is refused the same way, not misparsed."""
    from gesturediffusion_amd.utils.init import init_state_dict, synthetic_inputs
    from test_gpu_parity import build_model
    cfg = case(T64)[0]
    plain_cfg = {k: v for k, v in cfg.items() if k not in ("text_dim", "clip_dim")}
    text, plain = model_of(T64), build_model("mdm", plain_cfg, init_state_dict(plain_cfg, seed=3, perturb=True))
    x, seedp, mfcc = synthetic_inputs(plain_cfg, 2, 20, seed=5)
    t = torch.tensor([3, 999], device=dev())
    yp = {"seed": seedp.to(dev()), "mfcc": mfcc.to(dev())}
    want_text, want_plain = _fwd(text, T64), plain(x.to(dev()), t, yp).clone()
    blob_text, blob_plain = text.export_packed(dev()), plain.export_packed(dev())
    for m, blob in ((plain, blob_text), (text, blob_plain), (model_of("mdm_128_t40"), blob_text)):
        with pytest.raises(GdxError, match="another configuration"):
            m.load_packed(blob, dev())
    old = blob_plain[:8 + 44] + blob_plain[8 + 52:]                        # the header without text_dim / clip_dim
    for m in (plain, text):
        with pytest.raises(GdxError, match="another configuration"):
            m.load_packed(old, dev())
    assert torch.equal(_fwd(text, T64), want_text) and torch.equal(plain(x.to(dev()), t, yp), want_plain)
    plain.load_packed(blob_plain, dev())
    assert torch.equal(plain(x.to(dev()), t, yp), want_plain)


def test_packed_cache_replaces_an_image_of_the_earlier_format(tmp_path):
    """load_model_cached on a cache file with the header of before text_dim / clip_dim: refused, re-packed from the checkpoint and
    rewritten; the next start takes the image."""
    from gesturediffusion_amd.utils.model_util import load_model_cached, packed_image_path
    a = model_of(T64)
    ck = tmp_path / "model000000001.pt"
    torch.save(a.state_dict(), ck)
    blob = a.export_packed(dev())
    b = model_of(T64, seed=32)
    path = packed_image_path(str(tmp_path), str(ck), b)
    with open(path, "wb") as f:
        f.write(blob[:8 + 44] + blob[8 + 52:])
    assert load_model_cached(b, str(ck), dev(), str(tmp_path)) == "checkpoint"
    assert open(path, "rb").read() == blob and torch.equal(_fwd(b, T64), _fwd(a, T64))
    c = model_of(T64, seed=33)
    assert load_model_cached(c, str(ck), dev(), str(tmp_path)) == "image" and torch.equal(_fwd(c, T64), _fwd(a, T64))


def test_set_condition_entries_on_the_device():
    """The library's own refusals with real handles: each entry names the other, before any device work."""
    cfg, sd, x, t, y = case(T64)
    m = model_of(T64)
    yd = on_dev(y)
    _fwd(m, T64)
    eng = m._get_engine(dev())
    with pytest.raises(GdxError, match="gdx_set_condition_text"):
        eng.set_condition(yd["seed"], yd["mfcc"], cache=False)
    import ctypes as C
    lib, one = eng.lib, lambda v: C.c_void_p(v.data_ptr())
    assert lib.gdx_set_condition(eng.handle, one(yd["seed"]), one(yd["mfcc"]), None) != 0
    assert b"call gdx_set_condition_text" in lib.gdx_last_error()
    assert lib.gdx_set_condition_text(eng.handle, one(yd["seed"]), one(yd["mfcc"]), None, None) != 0
    assert b"null argument" in lib.gdx_last_error()
    assert torch.equal(_fwd(m, T64), _fwd(model_of(T64), T64))               # the refusals left the conditioning alone
    # a text handle without its two tensors names them, and only them, as missing; a no-text handle does not know them
    from gesturediffusion_amd.engine import Engine
    named = {k: v.detach() for k, v in {**m._engine_tensors(), **m._extra_engine_tensors(dev())}.items()}
    fresh = Engine(m._arch, 16, 128, 192, 1, 4, 10, text_dim=64, clip_dim=512)
    with pytest.raises(GdxError, match=r"^missing weights: embed_text.weight, embed_text.bias$"):
        fresh.load_tensors({k: v for k, v in named.items() if not k.startswith("embed_text.")})
    with pytest.raises(GdxError, match="unexpected key embed_text.weight"):
        Engine(m._arch, 16, 128, 192, 1, 4, 10).load_tensors(named)


# --------------------------------------------------------------------------------------------------------------------- CLI
def test_generate_cli_synthetic_use_text(tmp_path):
    """`sample.generate --synthetic --use_text`, two chunks, equals a direct sample_chunks call on the same features."""
    from gesturediffusion_amd.sample import generate
    from gesturediffusion_amd.utils.init import MFCC_DIM, init_state_dict
    from gesturediffusion_amd.utils.model_util import create_model_and_diffusion
    from gesturediffusion_amd.utils.parser_util import generate_args
    out = tmp_path / "out"
    argv = ["--synthetic", "--use_text", "--layers", "1", "--latent_dim", "128", "--num_samples", "2", "--chunks", "2",
            "--num_frames", "20", "--synthetic_njoints", "37", "--output_dir", str(out), "--seed", "7", "--timestep_respacing", "10",
            "--rng", "philox"]
    assert generate.main(argv) == 0
    res = np.load(out / "results.npy", allow_pickle=True).item()             # written by this test a moment ago
    assert res["motion"].shape == (2, 37, 1, 40) and np.isfinite(res["motion"]).all()
    args = generate_args(argv)
    args.mfcc_input = True
    model, diff = create_model_and_diffusion(args, None)
    assert model._text_dims() == (64, 512)
    cfg = dict(arch="mdm", njoints=37, nfeats=1, latent_dim=128, ff_size=1024, num_layers=1, num_heads=4, seed_poses=10,
               text_dim=64, clip_dim=512)
    model.load_state_dict(init_state_dict(cfg, seed=7), strict=False)
    model = ClassifierFreeSampleModel(model).to(dev()).eval()
    g = torch.Generator().manual_seed(7)
    first_seed = torch.randn(2, 37, 1, 10, generator=g).to(dev())
    mfccs = [torch.randn(2, MFCC_DIM, 1, 20, generator=g).to(dev()) for _ in range(2)]
    feats = generate.synthetic_text_features(7, 2, 512, 2)
    outs = generate.sample_chunks(model, diff, first_seed, lambda c: mfccs[c], 2, 20, 10, guidance_param=args.guidance_param,
                                  sampler="p", rng="philox", philox_seed=7, text_of_chunk=lambda c: feats[c].to(dev()))
    assert np.array_equal(res["motion"], torch.cat(outs, dim=3).cpu().numpy())
    # other features, other motion
    outs2 = generate.sample_chunks(model, diff, first_seed, lambda c: mfccs[c], 2, 20, 10, guidance_param=args.guidance_param,
                                   sampler="p", rng="philox", philox_seed=7, text_of_chunk=lambda c: feats[1 - c].to(dev()))
    assert not torch.equal(outs2[0], outs[0])
