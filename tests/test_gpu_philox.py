"""philox_normal4 (csrc/gdx_pose_device.h) on the GPU, held to tests/philox_restatement.py: gdx_randn per element against the float64
restatement at keys that set every counter and key word, the Box-Muller edge rows, the statistics of the key sets fixed on the
CPU (tests/test_philox_host.py), and every kernel that draws in-kernel noise against the same call fed gdx_randn's tape, bit for
bit, at a seed >= 2^32 and a batch that crosses sample 2^32.  The bound, its unit and K: philox_restatement.py."""
import itertools

import numpy as np
import pytest
import torch

import philox_restatement as P
from test_dpm_host import diffusion
from test_gpu_parity import _diffusion, build_model, dev

pytestmark = pytest.mark.gpu

SEED, OFFSET, BATCH = 2 ** 32 + 0x9e3779b9, 2 ** 32 - 2, 4          # samples 2^32 - 2 .. 2^32 + 1
DRAW = 2 ** 31 + 5
# (J, T): 37 * 20 = 740 elements per sample run the float4 instantiations, 37 * 10 = 370 the scalar ones with a 2-element tail
LAYOUTS = {"float4": (37, 20), "tail": (37, 10)}


def _randn_guarded(batch, per, seed, off, step):
    """gdx_randn into the middle of a larger buffer: (draw [batch, per] on the host, the four sentinels around it)."""
    from gesturediffusion_amd import _lib
    from gesturediffusion_amd import engine as E
    lib = _lib.load()
    n = batch * per
    buf = torch.full((n + 4,), -7.0, device=dev(), dtype=torch.float32)
    _lib.check(lib.gdx_randn(E._ptr(buf[2:]), batch, per, seed, off, step, E._stream(buf.device)), lib)
    host = buf.cpu().numpy()
    return host[2:2 + n].reshape(batch, per), np.concatenate((host[:2], host[2 + n:]))


@pytest.mark.parametrize("seed", P.SEEDS)
@pytest.mark.parametrize("shape", P.SHAPES, ids=["5x63", "3x320", "1x262157"])
def test_randn_vs_normal64(shape, seed):
    """Every sample_offset x step of the grid at one seed and shape: each element within K 2^-24 max(r, 2^-12) of the float64
    restatement, the two floats before and after the output untouched.  Prints the worst error in that unit."""
    per = int(np.prod(shape[1:]))
    worst = 0.0
    for off, step in itertools.product(P.OFFSETS, P.STEPS):
        b = P.batch_of(off, shape)
        got, guard = _randn_guarded(b, per, seed, off, step)
        assert np.array_equal(guard, np.full(4, -7.0, dtype=np.float32)), (off, step)
        z, r = P.reference(b, per, seed, off, step)
        units = P.error_units(got, z, r)
        worst = max(worst, float(units.max()))
        assert np.isfinite(got).all() and P.within_bound(got, z, r), (off, step, float(units.max()), np.argmax(units))
    print(f"philox-k gpu seed {seed:#x} per-sample {per}: worst error {worst:.4g} units of 2^-24 max(r, 2^-12) (K = {P.K})")


def test_engine_randn_is_the_guarded_call():
    from gesturediffusion_amd import engine as E
    got = E.randn((5, 7, 1, 9), dev(), SEED, OFFSET, DRAW)
    want, _ = _randn_guarded(5, 63, SEED, OFFSET, DRAW)
    assert got.shape == (5, 7, 1, 9) and np.array_equal(got.cpu().numpy().reshape(5, 63), want)


@pytest.mark.parametrize("shape", [(1, 1, 1, 128), (1, 127)], ids=["128", "127-tail"])
@pytest.mark.parametrize("step,group,slot,word,what", P.EDGES)
def test_edge_rows(step, group, slot, word, what, shape):
    """u0 = 1 gives +-0 exactly, angle 0 gives (radius, 0 exactly), u0 = 2^-24 gives the largest radius with z0^2 + z1^2 = r^2,
    nothing is NaN or Inf, every element of the row within the bound (philox_restatement.edge_failures)."""
    from gesturediffusion_amd import engine as E
    row = E.randn(shape, dev(), P.EDGE_SEED, 0, step).cpu().numpy().reshape(-1)
    e = 4 * group + 2 * (slot // 2)
    print(f"philox-edge {what} slot {slot}: {row[e]!r}, {row[e + 1]!r}")
    assert not P.edge_failures(row, step, group, slot)


@pytest.mark.parametrize("key", P.STAT_KEYS, ids=[f"key{i}" for i in range(len(P.STAT_KEYS))])
def test_statistics_of_the_device_draw(key):
    """The conditions the float64 restatement meets on the CPU at these key sets, on the device's 2^20 values."""
    from gesturediffusion_amd import engine as E
    flat = P.stat_draw(key, lambda b, per, seed, off, step: E.randn((b, per), dev(), seed, off, step).cpu().numpy())
    assert flat.size == 2 ** 20
    fig = P.stat_figures(flat)
    print(f"philox-stat gpu {key}:", {k: round(v, 2) for k, (v, _) in fig.items()})
    assert not P.stat_failures(flat)


# ------------------------------------------------------------------------------------------ the kernels that draw the tape
def _operands(J, T, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(BATCH, J, 1, T, generator=g).to(dev()) for _ in range(3)]


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("kind,eta", [("p", 0.0), ("ddim", 0.5)])
def test_sampler_update_draws_randns_tape(kind, eta, layout):
    from gesturediffusion_amd import engine as E
    from gesturediffusion_amd._lib import GDX_SAMPLER_DDIM, GDX_SAMPLER_P
    d = dev()
    J, T = LAYOUTS[layout]
    assert (J * T % 4 == 0) == (layout == "float4")
    k = GDX_SAMPLER_P if kind == "p" else GDX_SAMPLER_DDIM
    coef = _diffusion([20] if kind == "p" else "ddim100").coef_table(k, d, eta)
    x, x0, _ = _operands(J, T, 11)
    t = torch.tensor([3, 1, 9, 17], device=d)
    assert bool((coef[t][:, 2 if kind == "p" else 4] != 0).all())          # every row adds noise
    kw = dict(t=t)
    tape = E.randn(x.shape, d, SEED, OFFSET, DRAW)
    got = E.sampler_update(k, coef, x, x0, torch.empty_like(x), philox_seed=SEED, sample_offset=OFFSET, rng_step=DRAW, **kw)
    want = E.sampler_update(k, coef, x, x0, torch.empty_like(x), noise=tape, **kw)
    assert torch.isfinite(got).all() and torch.equal(got, want)
    assert not torch.equal(got, E.sampler_update(k, coef, x, x0, torch.empty_like(x), noise=torch.zeros_like(x), **kw))
    # const_noise: sample 0's tape (not sample_offset's) for every row
    tape0 = E.randn((1,) + tuple(x.shape[1:]), d, SEED, 0, DRAW)
    got = E.sampler_update(k, coef, x, x0, torch.empty_like(x), const_noise=True, philox_seed=SEED, sample_offset=OFFSET,
                           rng_step=DRAW, **kw)
    want = E.sampler_update(k, coef, x, x0, torch.empty_like(x), noise=tape0.expand_as(x).contiguous(), **kw)
    assert torch.equal(got, want)
    assert torch.equal(got, E.sampler_update(k, coef, x, x0, torch.empty_like(x), noise=tape0, const_noise=True, **kw))


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("order", [1, 2])
def test_dpm_sde_step_draws_randns_tape(order, layout):
    from gesturediffusion_amd import engine as E
    d = dev()
    J, T = LAYOUTS[layout]
    coef = diffusion("linear", "logsnr20").dpm_sde_coef_table(d, 1.0)
    assert float(coef[6, 7]) != 0                                            # the row's noise scale
    x, x0, m1 = _operands(J, T, 12)
    kw = dict(hist=[m1] if order == 2 else (), step_index=6)
    tape = E.randn(x.shape, d, SEED, OFFSET, DRAW)
    got = E.dpm_sde_step(order, coef, x, x0, torch.empty_like(x), philox_seed=SEED, sample_offset=OFFSET, rng_step=DRAW, **kw)
    want = E.dpm_sde_step(order, coef, x, x0, torch.empty_like(x), noise=tape, **kw)
    assert torch.isfinite(got).all() and torch.equal(got, want)
    assert not torch.equal(got, E.dpm_sde_step(order, coef, x, x0, torch.empty_like(x), noise=torch.zeros_like(x), **kw))


def _model(arch, T):
    """The tiny denoiser of the loop tests at J = 37 (the last channel quad of the token-major update is partial)."""
    from gesturediffusion_amd.utils.init import init_state_dict, synthetic_inputs
    cfg = dict(arch=arch, njoints=37, nfeats=1, latent_dim=128, ff_size=256, num_layers=2, num_heads=4, seed_poses=10)
    m = build_model(arch, cfg, init_state_dict(cfg, seed=2))
    x, seedp, mfcc = synthetic_inputs(cfg, BATCH, T, seed=6)
    return m, x.to(dev()), {"seed": seedp.to(dev()), "mfcc": mfcc.to(dev())}


@pytest.mark.parametrize("replay", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("arch,kind", [("mdm", "p"), ("mdm_old", "ddim_eta")])
def test_sample_loop_draws_randns_tape(arch, kind, replay):
    """gdx_sample_loop with in-kernel noise (T % 4 == 0, no inpainting, no dumps: the token-major update; under graph replay the
    captured pose-layout step, which reads its draw number from device memory) == the loop run step by step from randn's tape:
    x_T is draw 0, executed step k takes draw k + 1."""
    from gesturediffusion_amd import engine as E
    d = dev()
    m, _, y = _model(arch, 20)
    shape = (BATCH, 37, 1, 20)
    df = _diffusion([10])
    kw = dict(clip_denoised=False, model_kwargs={"y": y})
    fn, extra = (df.p_sample_loop, {}) if kind == "p" else (df.ddim_sample_loop, dict(eta=0.5))
    tape = torch.stack([E.randn(shape, d, SEED, OFFSET, k) for k in range(df.num_timesteps + 1)])
    want = fn(m, shape, noise_tape=tape, fused=False, **kw, **extra)
    eng = m._get_engine(d)
    eng.set_graph_replay(replay)
    try:
        got = fn(m, shape, rng="philox", philox_seed=SEED, sample_offset=OFFSET, **kw, **extra)
    finally:
        eng.set_graph_replay(False)
    assert torch.isfinite(got).all() and torch.equal(got, want)
    low = fn(m, shape, rng="philox", philox_seed=SEED & 0xffffffff, sample_offset=OFFSET, **kw, **extra)
    assert not torch.equal(low, got)                                       # the seed's high word is part of the key


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_bpd_loop_draws_randns_tape(layout):
    """calc_bpd_loop with a Philox seed (bpd_xt_kernel draws z and forms x_t) == the same call on the tape of randn's draws
    0 .. num_timesteps - 1."""
    from gesturediffusion_amd import engine as E
    d = dev()
    J, T = LAYOUTS[layout]
    m, x, y = _model("mdm_old", T)
    xs = (x * 0.6).contiguous()
    df = _diffusion([10])
    tape = torch.stack([E.randn(tuple(xs.shape), d, SEED, OFFSET, k) for k in range(df.num_timesteps)])
    kw = dict(clip_denoised=True, model_kwargs={"y": y})
    got = df.calc_bpd_loop(m, xs, rng="philox", philox_seed=SEED, sample_offset=OFFSET, **kw)
    want = df.calc_bpd_loop(m, xs, noise_tape=tape, **kw)
    for k in ("vb", "xstart_mse", "mse", "prior_bpd", "total_bpd"):
        assert torch.isfinite(got[k]).all() and torch.equal(got[k], want[k]), k
    # rows 2, 3 are samples 2^32 and 2^32 + 1: a shard that starts past the carry draws them again
    ys = {k: v[2:].contiguous() for k, v in y.items()}
    shard = df.calc_bpd_loop(m, xs[2:].contiguous(), rng="philox", philox_seed=SEED, sample_offset=2 ** 32,
                             clip_denoised=True, model_kwargs={"y": ys})
    assert torch.equal(shard["mse"], got["mse"][2:])
    low = df.calc_bpd_loop(m, xs[2:].contiguous(), rng="philox", philox_seed=SEED, sample_offset=0, clip_denoised=True,
                           model_kwargs={"y": ys})
    assert not torch.equal(low["mse"], shard["mse"])                       # the sample's high word is part of the key
