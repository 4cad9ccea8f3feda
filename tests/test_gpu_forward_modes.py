"""The branches of the per-step kernel sequence that depend on the compute mode and on keep_taps (csrc/forward.hip: forward_core and
its helpers linear / attend / add_norm), at the smallest models that take them.  Need an MI355X.

fp32 runs every sublayer in fp32; fp16 keeps a 16-bit residual stream, whose fp32 copies exist only while taps are kept; bf16 keeps
an fp32 residual stream beside the 16-bit GEMM operands.  With taps kept the last layer runs both the plain and the compacting
LayerNorm.  V2 at d=512 (d / cl_head = 64) takes the 16-bit front-end kernel in the 16-bit modes, at d=256 (32) the fp32 one."""
import functools

import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

DTYPES = ("fp32", "fp16", "bf16")
B, T, J, L = 3, 20, 16, 2
MODELS = {"v1": ("mdm_old", 128, 256), "v2d512": ("mdm", 512, 1024), "v2d256": ("mdm", 256, 512)}


def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


def _cfg(arch, d, ff, njoints=J, layers=L):
    return dict(arch=arch, njoints=njoints, nfeats=1, latent_dim=d, ff_size=ff, num_layers=layers, num_heads=4, seed_poses=10)


def _model(cfg, dtype, seed):
    from gesturediffusion_amd.model.mdm import MDM
    from gesturediffusion_amd.model.mdm_old import MDM_Old
    from gesturediffusion_amd.utils.init import init_state_dict
    m = (MDM if cfg["arch"] == "mdm" else MDM_Old)(
        njoints=cfg["njoints"], nfeats=1, translation=True, pose_rep="rot6d", glob=True, glob_rot=True,
        latent_dim=cfg["latent_dim"], ff_size=cfg["ff_size"], num_layers=cfg["num_layers"], num_heads=4, data_rep="genea_vec",
        cond_mask_prob=0.1, dataset="genea2023", mfcc_input=True, seed_poses=10, compute_dtype=dtype)
    m.load_state_dict(init_state_dict(cfg, seed=seed, perturb=True), strict=False)
    return m.to(dev()).eval()


def _engine(name, dtype):
    """A prepared engine of MODELS[name] with its inputs: (engine, x, t, seed poses, mfcc, scale)."""
    from gesturediffusion_amd.utils.init import synthetic_inputs
    cfg = _cfg(*MODELS[name])
    m = _model(cfg, dtype, seed=31)
    x, seedp, mfcc = (v.to(dev()) for v in synthetic_inputs(cfg, B, T, seed=5))
    eng = m._get_engine(dev())
    eng.prepare(B, T)
    return eng, x, torch.tensor([17, 803, 0], device=dev()), seedp, mfcc, torch.tensor([2.5, 1.0, 0.5], device=dev())


def _forwards(eng, x, t, seedp, mfcc, scale, taps):
    """{mode: (output, [taps])} of the three forward modes with keep_taps as given."""
    from gesturediffusion_amd.engine import GDX_CFG, GDX_COND, GDX_UNCOND
    eng.keep_taps(taps)
    eng.set_condition(seedp, mfcc, cache=False)
    d = eng.cfg.latent_dim
    res = {}
    for mode in (GDX_COND, GDX_UNCOND, GDX_CFG):
        out = eng.forward(x, t, mode, scale if mode == GDX_CFG else None)
        rows = (2 * B if mode == GDX_CFG else B) * (T + 1)
        res[mode] = (out, [eng.tap(i, rows, d, dev()) for i in range(L + 1)] if taps else [])
    return res


@functools.lru_cache(maxsize=None)
def _with_taps(name, dtype):
    return _forwards(*_engine(name, dtype), taps=True)


@pytest.mark.parametrize("name", sorted(MODELS))
@pytest.mark.parametrize("dtype", DTYPES)
def test_output_is_the_same_with_taps_kept(name, dtype):
    """Keeping taps adds the un-compacted last LayerNorm and, in the 16-bit stream, the fp32 copies: the prediction keeps its bits."""
    plain = _forwards(*_engine(name, dtype), taps=False)
    kept = _with_taps(name, dtype)
    for mode, (out, _) in plain.items():
        assert torch.isfinite(out).all()
        assert torch.equal(out, kept[mode][0]), mode


@pytest.mark.parametrize("name", sorted(MODELS))
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_half_mode_taps_are_their_own_stream(name, dtype):
    """The taps of a 16-bit mode are copies of ITS encoder stream (fp16: written beside the 16-bit stream by the front end and by
    LN2; bf16: its fp32 stream): finite, and not the fp32 mode's."""
    for mode, (_, taps) in _with_taps(name, dtype).items():
        assert len(taps) == L + 1
        for tap, ref in zip(taps, _with_taps(name, "fp32")[mode][1]):
            assert tap.shape == ref.shape and torch.isfinite(tap).all()
            assert not torch.equal(tap, ref), mode


def test_bf16_mode_taps_match_fp32_taps():
    """test_fp16_mode_taps_match_fp32_taps (test_gpu_parity.py) for bf16, at its configuration: every encoder-layer activation
    stays within the mode's stated forward tolerance of the fp32 path's.  Measured before this test was written:
    profiles/forward_unify_bits_ab.txt."""
    from gesturediffusion_amd.numerics import FORWARD_TOL
    from gesturediffusion_amd.utils.init import synthetic_inputs
    cfg = _cfg("mdm", 512, 1024, njoints=48, layers=3)
    x, seedp, mfcc = synthetic_inputs(cfg, 2, 30, seed=2)
    t = torch.tensor([17, 803], device=dev())
    y = {"seed": seedp.to(dev()), "mfcc": mfcc.to(dev())}
    taps = {}
    for dt in ("fp32", "bf16"):
        m = _model(cfg, dt, seed=1)
        eng = m._get_engine(dev())
        eng.keep_taps(True)
        m(x.to(dev()), t, y)
        taps[dt] = [eng.tap(i, 2 * 2 * 31, 512, dev())[: 2 * 31].cpu() for i in range(cfg["num_layers"] + 1)]
    errs = [rel_err(b, a) for a, b in zip(taps["fp32"], taps["bf16"])]
    print("bf16 tap rel_err vs fp32:", " ".join(f"{e:.3e}" for e in errs))
    for a, b, e in zip(taps["fp32"], taps["bf16"], errs):
        assert e < FORWARD_TOL["bf16"] and not torch.equal(a, b)


@pytest.mark.parametrize("dtype", DTYPES)
def test_switching_taps_on_one_engine(dtype):
    """gdx_set_keep_taps re-prepares the workspace at the current shape (the conditioning must be set again), and the same
    engine then computes the same bits, with the taps on and off again."""
    from gesturediffusion_amd.engine import GDX_CFG, GdxError
    eng, x, t, seedp, mfcc, scale = _engine("v2d512", dtype)
    outs = []
    for taps in (False, True, False):
        eng.keep_taps(taps)
        if outs:
            with pytest.raises(GdxError, match="gdx_set_condition"):
                eng.forward(x, t, GDX_CFG, scale)
        eng.set_condition(seedp, mfcc, cache=False)
        outs.append(eng.forward(x, t, GDX_CFG, scale))
        if taps:
            assert torch.isfinite(eng.tap(L, 2 * B * (T + 1), 512, dev())).all()
        else:
            with pytest.raises(GdxError, match="taps not kept"):
                eng.tap(0, 1, 512, dev())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
