"""CPU-only tests for encoder head widths 96 and 192 (latent_dim 384 / 768 at the reference's four heads): which widths the
library accepts and refuses before any HIP call, and the CPU oracle against the reference's own forwards at these widths
(tests/golden/forward_heads_tiny.npz, written by tools/make_golden_heads.py; at cl_head = 8 the V2 front end then has local
head widths 48 and 96)."""
import ctypes as C
import os

import pytest
import torch

from conftest import load_golden, rel_err

CASES = {"mdm_old_384": ("mdm_old", 384), "mdm_384": ("mdm", 384), "mdm_768": ("mdm", 768)}
WEIGHT_SEED = 11                                    # tools/make_golden_heads.py


def heads_cfg(arch, d):
    return dict(arch=arch, njoints=16, nfeats=1, latent_dim=d, ff_size=192, num_layers=1, num_heads=4, seed_poses=10)


def _lib_or_skip():
    from gesturediffusion_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgdx.so not built (run python __graft_entry__.py)")
    return _lib, _lib.load()


@pytest.mark.parametrize("hd", [48, 80, 160, 320])
@pytest.mark.parametrize("dtype", [0, 1, 2], ids=["fp32", "fp16", "bf16"])
def test_create_refuses_other_head_widths_and_names_the_supported_ones(hd, dtype):
    """latent_dim = 4 hd passes every other check of gdx_create (a multiple of 64, even d / cl_head), so the refusal is the
    head width's; the message lists the supported widths, 96 and 192 among them."""
    _lib, lib = _lib_or_skip()
    h = C.c_void_p()
    for arch in (1, 2):
        cfg = _lib.Config(arch=arch, njoints=16, latent_dim=4 * hd, ff_size=192, num_layers=1, num_heads=4, seed_poses=10,
                          mfcc_dim=26, cl_head=8, window=10, compute_dtype=dtype)
        assert lib.gdx_create(C.byref(cfg), C.byref(h)) != 0
        msg = lib.gdx_last_error()
        assert b"head_dim" in msg and b"96" in msg and b"192" in msg, msg
        for w in (b"32", b"64", b"128", b"256"):
            assert w in msg, msg


def test_attention_half_refusals_at_the_new_widths():
    """Before the first HIP call (the pointers are never dereferenced, `launched` stays untouched): head width 48 is still an
    unsupported shape, and the 8 x 2 and persistent kernels, which have no instantiation at 96 / 192, say so."""
    _lib, lib = _lib_or_skip()
    p = C.c_void_p(0x1000)
    rep = (C.c_int32 * 3)(-1, -1, -1)
    ok = dict(qkv_rows=2 * 61, ctx_rows=2 * 61, B=2, S=61, H=4, d=384, dtype=1, kernel=1, grid=0)
    cases = [
        (dict(d=4 * 48), b"unsupported shape"),
        (dict(d=4 * 48, dtype=2, kernel=0), b"unsupported shape"),
        (dict(d=4 * 160), b"unsupported shape"),
        (dict(d=384, kernel=2), b"no head_dim 96"),
        (dict(d=384, kernel=3), b"no head_dim 96"),
        (dict(d=384, kernel=3, dtype=2, grid=2), b"no head_dim 96"),
        (dict(d=768, kernel=2), b"no head_dim 192"),
        (dict(d=768, kernel=3, dtype=2), b"no head_dim 192"),
        (dict(d=192, H=2, kernel=2), b"no head_dim 96"),
    ]
    for change, msg in cases:
        a = dict(ok, **change)
        rc = lib.gdx_attention_half(p, a["qkv_rows"], p, a["ctx_rows"], a["B"], a["S"], a["H"], a["d"], a["dtype"], a["kernel"],
                                    a["grid"], rep, None)
        assert rc != 0 and msg in lib.gdx_last_error(), (change, lib.gdx_last_error())
        assert list(rep) == [-1, -1, -1], change
    # the unsupported-shape message names the widths too
    lib.gdx_attention_half(p, 122, p, 122, 2, 61, 4, 4 * 48, 1, 0, 0, rep, None)
    assert b"96" in lib.gdx_last_error() and b"192" in lib.gdx_last_error()


@pytest.mark.parametrize("hd", [48, 80, 160, 320])
def test_attention_entry_points_refuse_other_head_widths(hd):
    """gdx_attention_f32, gdx_attention_f16 and gdx_bench_attention refuse the width before touching the device."""
    _lib, lib = _lib_or_skip()
    p = C.c_void_p(0x1000)
    us = C.c_float(-1.0)
    assert lib.gdx_attention_f32(p, p, 2, 61, 4, 4 * hd, 1, None) != 0 and b"head_dim" in lib.gdx_last_error()
    assert b"96" in lib.gdx_last_error() and b"192" in lib.gdx_last_error()
    assert lib.gdx_attention_f16(p, p, 2, 61, 4, 4 * hd, None) != 0 and b"unsupported shape" in lib.gdx_last_error()
    for version in (1, 3):
        assert lib.gdx_bench_attention(2, 61, 4, 4 * hd, version, 1, C.byref(us), None) != 0
        assert b"head_dim" in lib.gdx_last_error() and us.value == -1.0


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("uncond", [False, True])
def test_oracle_reproduces_the_reference_at_head_widths_96_and_192(name, uncond):
    """The tolerance of the oracle-vs-fixture forward tests (tests/test_oracle_golden.py: 2e-6)."""
    from gesturediffusion_amd.utils.init import init_state_dict
    from oracle import mdm_forward as omf
    arch, d = CASES[name]
    g = load_golden("forward_heads_tiny.npz")
    cfg = heads_cfg(arch, d)
    sd = init_state_dict(cfg, seed=WEIGHT_SEED, perturb=True)
    y = {"seed": torch.from_numpy(g[name + ".seed"]), "mfcc": torch.from_numpy(g[name + ".mfcc"])}
    if uncond:
        y["uncond"] = True
    with torch.no_grad():
        out = omf.forward(sd, cfg, torch.from_numpy(g[name + ".x"]), torch.from_numpy(g[name + ".t"]), y)
    want = g[name + (".uncond.out" if uncond else ".cond.out")]
    assert out.shape == want.shape
    assert rel_err(out, want) < 2e-6


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_error_vs_fp64_reference_is_at_the_noise_floor(name):
    """As tests/test_oracle_golden.py does at head width 32: the fp32 reference's distance from its own fp64 run calibrates how
    far the oracle may lie from the fp64 result."""
    from gesturediffusion_amd.utils.init import init_state_dict
    from oracle import mdm_forward as omf
    arch, d = CASES[name]
    g = load_golden("forward_heads_tiny.npz")
    floor = rel_err(g[name + ".cond.out"], g[name + ".cond.out_fp64"])
    assert floor < 1e-5
    cfg = heads_cfg(arch, d)
    sd = init_state_dict(cfg, seed=WEIGHT_SEED, perturb=True)
    y = {"seed": torch.from_numpy(g[name + ".seed"]), "mfcc": torch.from_numpy(g[name + ".mfcc"])}
    with torch.no_grad():
        out = omf.forward(sd, cfg, torch.from_numpy(g[name + ".x"]), torch.from_numpy(g[name + ".t"]), y)
    assert rel_err(out, g[name + ".cond.out_fp64"]) < 10 * max(floor, 1e-7)
