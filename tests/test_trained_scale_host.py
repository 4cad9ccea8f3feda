"""Host checks (no GPU) that keep the inputs of tests/test_gpu_trained_scale.py and tests/test_gpu_activations.py honest: the
scaled weights really push FFN-1's GELU arguments beyond the 16-bit kernels' clamp (and initialisation-scale weights never
do: the gap those modules close), the oracle runs in every dtype the GPU module compares against and its float32 run stays at
fp32 round-off of its float64 run, and the activation grid is exact in every number format it passes through.

Measured on the CPU oracle at (s_ffn, s_qk) = (6, 3), conditional (share beyond |x| > 4.24, share below -4.24, minimum):
  v1_tiny 21.6 % 10.3 % -13.2;  v2_tiny 23.5 % 12.3 % -12.7;  v1_d512 22.5 % 10.7 % -14.9;  v2_d512 21.9 % 11.3 % -15.5;
  v1_d96 21.7 % 10.9 % -13.0 (unconditional: within a point of these).  At (1, 1) the largest |x| is 2.1 - 2.7: no argument
  beyond the clamp in any case."""
import pytest
import torch

import activation_grid as AG
import trained_scale as TS


@pytest.mark.parametrize("name", sorted(TS.CASES))
def test_scaled_weights_reach_the_gelu_tails(name):
    """At (6, 3): at least 15 % of the GELU arguments beyond +-4.24, at least 8 % below -4.24, one below -8; at (1, 1) none
    beyond +-4.24."""
    for uncond in (False, True):
        pre = TS.ffn1_preactivations(name, 6, 3, uncond)
        beyond = float((pre.abs() > TS.CLAMP).double().mean())
        below = float((pre < -TS.CLAMP).double().mean())
        print(f"\n[{name} uncond={uncond} (6, 3)] beyond {100 * beyond:.1f} %, below {100 * below:.1f} %, min {float(pre.min()):.1f}, "
              f"max {float(pre.max()):.1f}")
        assert beyond >= 0.15 and below >= 0.08 and float(pre.min()) < -8.0
        init = TS.ffn1_preactivations(name, 1, 1, uncond)
        print(f"[{name} uncond={uncond} (1, 1)] max |x| {float(init.abs().max()):.2f}")
        assert not bool((init.abs() > TS.CLAMP).any()), "initialisation-scale weights already reach the clamp"


def test_trained_scale_touches_only_what_it_says():
    from gesturediffusion_amd.utils.init import init_state_dict
    cfg = TS.case_cfg("v2_tiny")
    d = cfg["latent_dim"]
    sd = init_state_dict(cfg, seed=41, perturb=True)
    keep = {k: v.clone() for k, v in sd.items()}
    out = TS.trained_scale(sd, cfg, 6, 3)
    assert all(torch.equal(sd[k], keep[k]) for k in sd), "the input state dict was modified"
    for k, v in out.items():
        if ".linear1." in k:
            assert torch.equal(v, 6 * sd[k])
        elif k.endswith("in_proj_weight") or k.endswith("in_proj_bias"):
            assert torch.equal(v[: 2 * d], 3 * sd[k][: 2 * d]) and torch.equal(v[2 * d:], sd[k][2 * d:])
        else:
            assert torch.equal(v, sd[k]), k


@pytest.mark.parametrize("name", ["v1_tiny", "v2_tiny"])
def test_oracle_runs_in_every_dtype(name):
    """The oracle's tables follow the parameters' dtype: float64, float16 and bfloat16 runs stay in their dtype (asserted in
    TS.oracle), the float32 run is within 5e-6 of the float64 one at both scales (a quarter of FWD_TOL = 2e-5; measured
    6.9e-7 - 2.8e-6: the reference itself is well inside the bound the GPU forwards are held to), and the 16-bit runs are
    finite and further from float64 than float32 is."""
    from conftest import rel_err
    for s_ffn, s_qk in TS.SCALES:
        ref = TS.oracle(name, s_ffn, s_qk, False, "fp64")[0]
        e32 = rel_err(TS.oracle(name, s_ffn, s_qk, False, "fp32")[0], ref)
        e16 = {dt: rel_err(TS.oracle(name, s_ffn, s_qk, False, dt)[0], ref) for dt in ("fp16", "bf16")}
        print(f"\n[{name} ({s_ffn}, {s_qk})] oracle error against float64: fp32 {e32:.2e}, fp16 {e16['fp16']:.2e}, bf16 {e16['bf16']:.2e}")
        assert 0 < e32 < 5e-6
        assert all(torch.isfinite(TS.oracle(name, s_ffn, s_qk, False, dt)[0]).all() for dt in e16)
        assert e32 < e16["fp16"] < e16["bf16"] < 0.1


def test_activation_grid_is_exact():
    """Every grid x_m survives bf16 and fp16; every x_m + b_n is the same number in float32 and float64 (so the kernels'
    pre-activation has no rounding and the fp64 reference sees the kernels' own argument)."""
    for name, (rows, bias) in AG.GRIDS.items():
        x, b = rows(), bias()
        assert x.dtype == torch.float32 and b.dtype == torch.float32
        if name != "silu":                       # SiLU's kernel is fp32 only
            for dt in (torch.bfloat16, torch.float16):
                assert torch.equal(x.to(dt).float(), x), f"{name}: a row value is not exact in {dt}"
        s32 = x[:, None] + b[None, :]
        s64 = x.double()[:, None] + b.double()[None, :]
        assert torch.equal(s32.double(), s64), f"{name}: x_m + b_n rounds in float32"
        assert s64.unique().numel() == s64.numel(), f"{name}: the grid repeats a pre-activation"
    x, b = AG.GRIDS["wide"][0](), AG.GRIDS["wide"][1]()
    s = x[:, None] + b[None, :]
    assert float(s.min()) == -16.0 and float(s.max()) == 16.0 - 1.0 / 512 and s.numel() == 16384
