"""Encoder head widths 96 and 192 (latent_dim 384 / 768 at the reference's four heads) on the GPU: the fp32 and 16-bit
self-attention kernels alone against float64 attention, then forwards, loops, the packed image and batch independence of
whole models at these widths in every compute mode.  At cl_head = 8 the V2 front end runs its general kernel at local head
widths 48 / 96.  Need an MI355X.

Helpers and tolerances are those of tests/test_gpu_parity.py (rel_err, build_model, FWD_TOL, LOOP_TOL), of
tests/test_gpu_attention_half.py (float64 reference, per-element bound and whole-output bound per dtype) and of
gesturediffusion_amd/numerics.py (the stated 16-bit tolerance)."""
import ctypes as C
import functools

import pytest
import torch

from conftest import load_golden, rel_err
from gesturediffusion_amd import _lib
from gesturediffusion_amd.numerics import stated_tolerance
from test_gpu_attention_half import BF16, F16, H8, NAME, check, reference
from test_gpu_parity import FWD_TOL, LOOP_TOL, _diffusion, build_model, dev

pytestmark = pytest.mark.gpu

# single token, exact block, one short of and one past the 32-key tile, a ragged last query group of the 128-row workgroup
SEQ = [1, 16, 31, 33, 65, 128, 197]
SHAPES = [(4, 384), (4, 768), (2, 192)]                      # (H, d): head widths 96, 192, 96


def vp(t):
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------------------ fp32 attention
@pytest.mark.parametrize("version", [1, 0])
@pytest.mark.parametrize("B,S,H,dm", [(2 + (S + H) % 2, S, H, dm) for H, dm in SHAPES for S in SEQ] + [(66, 197, 4, 384)])
def test_fp32_attention_heads_vs_fp64(B, S, H, dm, version):
    """csrc/attention.hip at head widths 96 / 192 (version 1, and version 0 = the forward's choice, which attention3 does not
    take at these widths) against fp64 softmax attention, the bound of test_fp32_attention_vs_torch.  Q is scaled by 3 so the
    running-max rescale acts; ctx starts as NaN; the last row has more workgroups than CUs."""
    lib = _lib.load()
    d = dev()
    hd = dm // H
    g = torch.Generator(device=d).manual_seed(S + dm)
    qkv = torch.randn(B * S, 3 * dm, device=d, generator=g)
    qkv[:, :dm] *= 3.0
    ctx = torch.full((B * S, dm), float("nan"), device=d)
    _lib.check(lib.gdx_attention_f32(vp(qkv), vp(ctx), B, S, H, dm, version, stream()), lib)
    r = qkv.double().view(B, S, 3, H, hd)
    q, k, v = (r[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    p = torch.softmax(q @ k.transpose(-1, -2) / hd ** 0.5, dim=-1)
    ref = (p @ v).permute(0, 2, 1, 3).reshape(B * S, dm)
    err = rel_err(ctx.cpu().double(), ref.cpu())
    print(f"[heads-measure] fp32 attention v{version} B={B} S={S} H={H} d={dm}: rel err {err:.2e}")
    assert err < 2e-6


# ---------------------------------------------------------------------------------------------------------- 16-bit attention
PAD = 48                                                     # readable qkv rows past B*S
CTX_PAD = 3


def run_half(qkv, B, S, H, dm, dtype, kernel, grid=0):
    """gdx_attention_half on qkv ([B*S + PAD][3d], NaN in the rows past B*S) into a ctx of B*S + CTX_PAD rows: NaN below B*S,
    small integers (exact in both 16-bit types) in the rows past it, which must come back unchanged."""
    lib = _lib.load()
    rows = B * S
    ctx = torch.full((rows + CTX_PAD, dm), float("nan"), device=qkv.device)
    keep = (torch.arange(CTX_PAD * dm, device=qkv.device) % 17 - 8).float().view(CTX_PAD, dm)
    ctx[rows:] = keep
    rep = (C.c_int32 * 3)()
    _lib.check(lib.gdx_attention_half(vp(qkv), qkv.shape[0], vp(ctx), ctx.shape[0], B, S, H, dm, dtype, kernel, grid, rep,
                                      stream()), lib)
    what = f"{NAME[dtype]} kernel={kernel} B={B} S={S} H={H} d={dm}"
    assert bool(torch.isfinite(ctx[:rows]).all()), f"{what}: a row below B*S holds a non-finite value"
    assert torch.equal(ctx[rows:], keep), f"{what}: a ctx row past B*S was changed"
    return ctx[:rows], tuple(rep)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("H,dm", SHAPES)
@pytest.mark.parametrize("S", SEQ + [100])
def test_attention_half_heads_vs_fp64(S, H, dm, dtype):
    """attentionh8_kernel<96 / 192>, forced (kernel = 1) and through the forward's dispatch (kernel = 0, which keeps these widths
    on it: the 8 x 2 and persistent kernels are not instantiated for them), at every sequence length of SEQ and at
    B = 3, S = 100 (the shape the persistent form's small-grid walk uses where it exists): per-element and whole-output bounds of
    tests/test_gpu_attention_half.py against fp64 attention on the rounded inputs; NaN in the readable qkv rows past B*S must
    not reach any output; `launched` reports kernel 1 and one workgroup per (sample, head, chunk of 8 query blocks)."""
    d = dev()
    B = 3 if S == 100 else 2 + (S + H) % 2
    g = torch.Generator(device=d).manual_seed(S * 10 + dm + dtype)
    qkv = torch.randn(B * S + PAD, 3 * dm, device=d, generator=g)
    qkv[:, :dm] *= 2.0
    qkv[B * S:] = float("nan")
    refw = reference(qkv, B, S, H, dm, dtype)
    n8 = B * H * (((S + 15) // 16 + 7) // 8)
    outs = []
    for kernel in (H8, 0):
        got, rep = run_half(qkv, B, S, H, dm, dtype, kernel)
        assert rep == (H8, n8, n8), f"{NAME[dtype]} kernel={kernel} B={B} S={S} H={H} d={dm}: launched {rep}"
        check(got, refw, dtype, f"{NAME[dtype]} heads hd={dm // H} B={B} S={S} kernel={kernel}")
        outs.append(got.contiguous().view(torch.int32))
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("hd", [96, 192])
def test_attention_half_heads_many_workgroups_and_independence(hd, dtype):
    """More workgroups than CUs (B = 66, S = 197: 528 workgroups of two query chunks each), and every sample's rows bit-equal
    to a B = 1 call on that sample alone with nothing readable past it (the K/V tile rows past a sample's last key are never
    looked at)."""
    H, S, B = 4, 197, 66
    dm = H * hd
    d = dev()
    g = torch.Generator(device=d).manual_seed(hd + dtype)
    qkv = torch.randn(B * S + PAD, 3 * dm, device=d, generator=g)
    qkv[:, :dm] *= 2.0
    qkv[B * S:] = float("nan")
    got, rep = run_half(qkv, B, S, H, dm, dtype, 0)
    assert rep == (H8, B * H * 2, B * H * 2)
    for b in (0, 31, B - 1):
        sl = slice(b * S, (b + 1) * S)
        check(got[sl], reference(qkv[sl], 1, S, H, dm, dtype), dtype, f"{NAME[dtype]} heads hd={hd} sample {b} of {B}")
        alone, _ = run_half(qkv[sl].contiguous(), 1, S, H, dm, dtype, H8)
        assert torch.equal(alone.contiguous().view(torch.int32), got[sl].contiguous().view(torch.int32)), b


# ------------------------------------------------------------------------------------------------------------------ forwards
def heads_cfg(arch, dm, layers=2, J=37):
    return dict(arch=arch, njoints=J, nfeats=1, latent_dim=dm, ff_size=192, num_layers=layers, num_heads=4, seed_poses=10)


FWD_ROWS = [("mdm_old", 384, 37), ("mdm", 384, 40), ("mdm", 384, 10), ("mdm_old", 768, 37), ("mdm", 768, 40), ("mdm", 768, 10)]


@functools.lru_cache(maxsize=None)
def oracle_forward(arch, dm, T, B=3):
    """Weights, inputs and the CPU oracle's output of one row, computed once and shared by the compute modes (read only)."""
    from gesturediffusion_amd.utils.init import init_state_dict, synthetic_inputs
    from oracle import mdm_forward as omf
    cfg = heads_cfg(arch, dm)
    sd = init_state_dict(cfg, seed=5, perturb=True)
    x, seedp, mfcc = synthetic_inputs(cfg, B, T, seed=11)
    t = (torch.arange(B) * 97 + 3) % 1000
    with torch.no_grad():
        want = omf.forward(sd, cfg, x, t, {"seed": seedp, "mfcc": mfcc})
    return cfg, sd, x, seedp, mfcc, t, want


@pytest.mark.parametrize("dtype", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("arch,dm,T", FWD_ROWS)
def test_forward_heads_vs_oracle(arch, dm, T, dtype):
    """MDM_Old (T = 37) and MDM (T = 40, and one window only: T = 10) at latent_dim 384 / 768, four heads, B = 3, in every compute
    mode against the CPU oracle: fp32 at FWD_TOL, the 16-bit modes at their stated forward tolerance; with the workspace
    guard zones on, none of which may be touched."""
    cfg, sd, x, seedp, mfcc, t, want = oracle_forward(arch, dm, T)
    m = build_model(arch, cfg, sd)
    m.compute_dtype = dtype
    d = dev()
    eng = m._get_engine(d)
    eng.set_guards(True)
    try:
        out = m(x.to(d), t.to(d), {"seed": seedp.to(d), "mfcc": mfcc.to(d)})
        bad, zone = eng.check_guards(d)
        assert bad == 0, f"{bad} guard bytes overwritten, first in workspace allocation #{zone}"
    finally:
        eng.set_guards(False)
    err = rel_err(out.cpu(), want)
    print(f"[heads-measure] forward {arch} d={dm} T={T} {dtype}: rel err {err:.2e}")
    assert err < (FWD_TOL if dtype == "fp32" else stated_tolerance(dtype, loop=False))


GOLDEN_CASES = {"mdm_old_384": ("mdm_old", 384), "mdm_384": ("mdm", 384), "mdm_768": ("mdm", 768)}


@pytest.mark.parametrize("name", sorted(GOLDEN_CASES))
def test_forward_heads_vs_reference_golden(name):
    """The reference's own forwards at latent_dim 384 / 768 (tests/golden/forward_heads_tiny.npz), fp32, conditional and
    unconditional."""
    from gesturediffusion_amd.utils.init import init_state_dict
    arch, dm = GOLDEN_CASES[name]
    g = load_golden("forward_heads_tiny.npz")
    cfg = heads_cfg(arch, dm, layers=1, J=16)
    m = build_model(arch, cfg, init_state_dict(cfg, seed=11, perturb=True))
    d = dev()
    x, t = torch.from_numpy(g[name + ".x"]).to(d), torch.from_numpy(g[name + ".t"]).to(d)
    y = {"seed": torch.from_numpy(g[name + ".seed"]).to(d), "mfcc": torch.from_numpy(g[name + ".mfcc"]).to(d)}
    out = m(x, t, y).cpu()
    assert rel_err(out, g[name + ".cond.out"]) < FWD_TOL
    assert rel_err(m(x, t, dict(y, uncond=True)).cpu(), g[name + ".uncond.out"]) < FWD_TOL
    # against the reference run in fp64, measured in units of the reference's own fp32 round-off (as
    # test_gpu_parity.py::test_forward_error_vs_fp64_is_at_noise_floor does at head width 32)
    floor = rel_err(g[name + ".cond.out"], g[name + ".cond.out_fp64"])
    ours = rel_err(out, g[name + ".cond.out_fp64"])
    print(f"[heads-measure] {name}: from the fp64 reference {ours:.2e}, the fp32 reference's own {floor:.2e}")
    assert ours < 10 * max(floor, 1e-7), (ours, floor)


@pytest.mark.parametrize("extra", [["--arch_version", "mdm", "--latent_dim", "768"],
                                   ["--arch_version", "mdm_old", "--latent_dim", "768", "--compute_dtype", "fp16"],
                                   ["--arch_version", "mdm", "--latent_dim", "768", "--compute_dtype", "bf16"],
                                   ["--arch_version", "mdm_old", "--latent_dim", "384"]])
def test_generate_cli_synthetic_heads(tmp_path, extra):
    """`sample.generate --synthetic --latent_dim 768` (and 384) end to end, as tests/test_gpu_parity.py::test_generate_cli_synthetic
    runs it at 128: the CLI's four heads make these head widths 192 / 96; guided, chunked sampling with seed chaining in each
    compute mode writes finite, non-zero motion of the right shape."""
    import numpy as np
    from gesturediffusion_amd.sample import generate
    out = tmp_path / "out"
    argv = ["--synthetic", "--layers", "2", "--num_samples", "3", "--chunks", "2", "--num_frames", "20", "--synthetic_njoints", "37",
            "--output_dir", str(out), "--seed", "7", "--timestep_respacing", "25"] + extra
    assert generate.main(argv) == 0
    res = np.load(out / "results.npy", allow_pickle=True).item()      # written by this test a moment ago
    assert res["motion"].shape == (3, 37, 1, 40)
    assert np.isfinite(res["motion"]).all() and np.abs(res["motion"]).max() > 0


# --------------------------------------------------------------------------------------------------------------------- loops
@functools.lru_cache(maxsize=None)
def loop_inputs(arch, B=3):
    from gesturediffusion_amd.utils.init import init_state_dict, synthetic_inputs
    cfg = heads_cfg(arch, 384)
    T = 40 if arch == "mdm" else 37
    sd = init_state_dict(cfg, seed=6, perturb=True)
    _, seedp, mfcc = synthetic_inputs(cfg, B, T, seed=12)
    tape = torch.randn(11, B, cfg["njoints"], 1, T, generator=torch.Generator().manual_seed(4321))
    return cfg, sd, seedp, mfcc, tape


def oracle_ddim10(arch, scale=None):
    from oracle import mdm_forward as omf
    from oracle import sampler as osamp
    from oracle import schedule as osch
    cfg, sd, seedp, mfcc, tape = loop_inputs(arch)
    y = {"seed": seedp, "mfcc": mfcc}
    fn = lambda x, t, yy: omf.forward(sd, cfg, x, t, yy)          # noqa: E731
    if scale is not None:
        y["scale"] = scale
        fn = lambda x, t, yy: omf.cfg_forward(sd, cfg, x, t, yy)  # noqa: E731
    tab, tmap = osch.make_tables("cosine", 1000, "ddim10")
    with torch.no_grad():
        return osamp.sample_loop(fn, tab, tmap, tape[0].shape, tape, y, kind="ddim")


@pytest.mark.parametrize("arch", ["mdm", "mdm_old"])
def test_ddim_loop_heads_vs_oracle(arch):
    """The fused ddim_sample_loop (ddim10, recorded noise tape) at latent_dim 384 against the oracle sampler, fp32."""
    cfg, sd, seedp, mfcc, tape = loop_inputs(arch)
    d = dev()
    m = build_model(arch, cfg, sd)
    y = {"seed": seedp.to(d), "mfcc": mfcc.to(d)}
    r = _diffusion("ddim10").ddim_sample_loop(m, tuple(tape[0].shape), noise_tape=tape.to(d), clip_denoised=False,
                                               model_kwargs={"y": y}, progress=False)
    assert rel_err(r.cpu(), oracle_ddim10(arch)) < LOOP_TOL


def test_cfg_loop_heads_fp16_vs_oracle():
    """The guided loop (scales 2.5, 0, 1) at latent_dim 384 in fp16 against the oracle's fp32 loop, at the mode's stated loop
    tolerance under guidance."""
    from gesturediffusion_amd.model.cfg_sampler import ClassifierFreeSampleModel
    arch = "mdm"
    cfg, sd, seedp, mfcc, tape = loop_inputs(arch)
    scale = torch.tensor([2.5, 0.0, 1.0])
    d = dev()
    m = build_model(arch, cfg, sd)
    m.compute_dtype = "fp16"
    y = {"seed": seedp.to(d), "mfcc": mfcc.to(d), "scale": scale.to(d)}
    r = _diffusion("ddim10").ddim_sample_loop(ClassifierFreeSampleModel(m), tuple(tape[0].shape), noise_tape=tape.to(d),
                                               clip_denoised=False, model_kwargs={"y": y}, progress=False)
    err = rel_err(r.cpu(), oracle_ddim10(arch, scale))
    print(f"[heads-measure] cfg ddim10 loop fp16 d=384: rel err {err:.2e}")
    assert err < stated_tolerance("fp16", 2.5, loop=True)


# -------------------------------------------------------------------------------------------------------------- packed image
def _forward(m, cfg, B=3, T=20):
    from gesturediffusion_amd.utils.init import synthetic_inputs
    x, seedp, mfcc = synthetic_inputs(cfg, B, T, seed=5)
    t = torch.tensor([3, 500, 999][:B])
    return m(x.to(dev()), t.to(dev()), y={"seed": seedp.to(dev()), "mfcc": mfcc.to(dev())}).clone()


@pytest.mark.parametrize("arch", ["mdm", "mdm_old"])
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_packed_image_roundtrip_heads(arch, dtype):
    """Export at latent_dim 384, import into a model holding other weights: the forward after import is bit-equal to the
    exporter's."""
    from gesturediffusion_amd.utils.init import init_state_dict
    cfg = heads_cfg(arch, 384)
    a = build_model(arch, cfg, init_state_dict(cfg, seed=31, perturb=True))
    b = build_model(arch, cfg, init_state_dict(cfg, seed=32, perturb=True))
    a.compute_dtype = b.compute_dtype = dtype
    out_a, out_b = _forward(a, cfg), _forward(b, cfg)
    assert not torch.equal(out_a, out_b)
    b.load_packed(a.export_packed(dev()), dev())
    assert torch.equal(_forward(b, cfg), out_a)
    assert torch.equal(_forward(b, cfg, B=2, T=30), _forward(a, cfg, B=2, T=30))


# -------------------------------------------------------------------------------------------------------- batch independence
@pytest.mark.parametrize("dtype", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("arch", ["mdm", "mdm_old"])
def test_batch_independence_heads_768(arch, dtype):
    """Row b of a B = 40 forward at latent_dim 768 equals the same samples run as a batch of 2, bit for bit (the property
    test_full_size_properties_config2 checks at head width 128)."""
    from gesturediffusion_amd.utils.init import init_state_dict, synthetic_inputs
    cfg = heads_cfg(arch, 768)
    m = build_model(arch, cfg, init_state_dict(cfg, seed=7, perturb=True))
    m.compute_dtype = dtype
    d = dev()
    B, T = 40, 40 if arch == "mdm" else 37
    x, seedp, mfcc = synthetic_inputs(cfg, B, T, seed=10)
    t = torch.full((B,), 321, device=d)
    full = m(x.to(d), t, {"seed": seedp.to(d), "mfcc": mfcc.to(d)}).clone()
    assert torch.isfinite(full).all()
    for lo in (0, 17, 38):
        sub = m(x[lo:lo + 2].to(d), t[:2], {"seed": seedp[lo:lo + 2].to(d), "mfcc": mfcc[lo:lo + 2].to(d)})
        assert torch.equal(full[lo:lo + 2], sub), lo
