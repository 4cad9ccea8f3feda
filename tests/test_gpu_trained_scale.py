"""Forwards away from initialisation scale, in every compute mode, against the oracle in float64.  Need an MI355X.

Every other end-to-end comparison of the suite runs on init_state_dict weights (or golden fixtures made with the same
initialiser): FFN-1's GELU arguments stay inside [-3, 3] and the self-attention's softmax rows are near uniform.  Here linear1 is
multiplied by s_ffn and the q and k rows of in_proj by s_qk (tests/trained_scale.py; tests/test_trained_scale_host.py checks
on the CPU that a fifth of the GELU arguments then lie beyond +-4.24, down to -13 .. -16): (s_ffn, s_qk) = (6, 3) and (12, 4).

Cases (tests/trained_scale.py CASES; two layers, B = 2): both architectures at d = 128, ff = 256, 4 heads, T = 20; both at
d = 512, ff = 1024, 8 heads (persistent fp32 GEMM, attention3), MDM_Old at T = 37 and MDM at T = 40 (its local attention takes
whole windows of 10 only; the reference raises at T = 37); MDM_Old at d = 96, ff = 160, 3 heads, T = 37 (csrc/gemm.hip), fp32 only:
gdx_create refuses a 16-bit mode whose widths are not multiples of 64.  Each conditional and unconditional; one guided forward
(scale 2.5) through ClassifierFreeSampleModel per architecture at the tiny shape.

fp32 mode: the encoder input, every layer's output and the prediction against the float64 oracle, each held to
ours < 10 max(floor, 1e-7) (floor = the float32 oracle's own error against float64, computed here: the convention of
test_gpu_parity.py::test_forward_error_vs_fp64_is_at_noise_floor) and to FWD_TOL = 2e-5.

fp16 / bf16 modes: the prediction is finite and ours <= 2 floor16, where floor16 is the error of the same oracle run entirely in
that 16-bit dtype on the CPU.  The kernels keep fp32 accumulators and fp32 LayerNorm statistics, so they should not be worse
than a pipeline that rounds every intermediate; the factor 2 allows for CPU kernels that accumulate wider than they store.

Measured on an MI355X (error relative to max|float64 output|; cond / uncond).
fp32, worst stage of the five (floor in brackets):
  v1_tiny (6,3) 6.6e-7 / 8.7e-7 [7.1e-7 / 7.8e-7]     (12,4) 7.6e-7 / 9.7e-7 [7.3e-7 / 1.1e-6]
  v2_tiny (6,3) 1.7e-6 / 2.9e-6 [1.9e-6 / 2.9e-6]     (12,4) 3.3e-6 / 3.1e-6 [3.2e-6 / 3.3e-6]
  v1_d512 (6,3) 1.1e-6 / 1.3e-6 [8.6e-7 / 1.0e-6]     (12,4) 2.1e-6 / 2.3e-6 [1.4e-6 / 1.2e-6]
  v2_d512 (6,3) 1.6e-6 / 5.7e-6 [1.6e-6 / 5.8e-6]     (12,4) 2.4e-6 / 6.4e-6 [2.3e-6 / 6.7e-6]
  v1_d96  (6,3) 9.2e-7 / 1.5e-6 [9.2e-7 / 1.3e-6]     (12,4) 1.2e-6 / 1.4e-6 [9.7e-7 / 1.4e-6]
  guided (6,3): v1_tiny 1.7e-6 [1.6e-6], v2_tiny 1.8e-6 [1.9e-6].  No stage of any case is above 2 x its floor.
16-bit, ours / floor16 = ratio:
  fp16 v1_tiny (6,3) 1.0e-3 / 1.6e-3 = 0.63, 8.6e-4 / 1.3e-3 = 0.67     (12,4) 1.2e-3 / 2.6e-3 = 0.46, 1.75e-3 / 1.6e-3 = 1.10
  fp16 v2_tiny (6,3) 1.1e-3 / 1.4e-3 = 0.78, 1.1e-3 / 1.8e-3 = 0.62     (12,4) 1.1e-3 / 1.7e-3 = 0.63, 1.3e-3 / 2.1e-3 = 0.63
  fp16 v1_d512 (6,3) 1.0e-3 / 1.3e-3 = 0.79, 8.6e-4 / 1.3e-3 = 0.67     (12,4) 1.5e-3 / 1.7e-3 = 0.86, 1.3e-3 / 1.7e-3 = 0.74
  fp16 v2_d512 (6,3) 7.8e-4 / 1.3e-3 = 0.59, 1.2e-3 / 1.8e-3 = 0.67     (12,4) 9.3e-4 / 1.5e-3 = 0.64, 1.2e-3 / 2.1e-3 = 0.58
  bf16 v1_tiny (6,3) 5.5e-3 / 1.0e-2 = 0.53, 6.3e-3 / 1.2e-2 = 0.53     (12,4) 8.4e-3 / 1.3e-2 = 0.67, 1.22e-2 / 1.56e-2 = 0.78
  bf16 v2_tiny (6,3) 6.3e-3 / 1.1e-2 = 0.58, 5.9e-3 / 1.1e-2 = 0.52     (12,4) 9.2e-3 / 1.5e-2 = 0.63, 7.1e-3 / 1.5e-2 = 0.47
  bf16 v1_d512 (6,3) 6.9e-3 / 1.2e-2 = 0.59, 7.3e-3 / 1.1e-2 = 0.68     (12,4) 9.5e-3 / 1.4e-2 = 0.68, 9.4e-3 / 1.1e-2 = 0.82
  bf16 v2_d512 (6,3) 5.7e-3 / 9.3e-3 = 0.62, 7.7e-3 / 1.3e-2 = 0.60     (12,4) 6.8e-3 / 1.1e-2 = 0.61, 1.07e-2 / 1.4e-2 = 0.77
The modes' stated forward tolerance (numerics.py FORWARD_TOL: 2e-2, set at initialisation scale) held in all of these, bf16 with
little room at (12, 4) (1.22e-2, and an all-bf16 pipeline is at 1.56e-2): it may not hold at larger scales and is not asserted
here; the constant is left as it is.
"""
import functools

import pytest
import torch

import trained_scale as TS
from conftest import rel_err
from test_gpu_parity import FWD_TOL, build_model, dev

pytestmark = pytest.mark.gpu

HALF_CASES = [n for n in sorted(TS.CASES) if TS.CASES[n][1] % 64 == 0]
GUIDANCE = 2.5


@functools.lru_cache(maxsize=None)
def model(name, s_ffn, s_qk, dtype):
    cfg = TS.case_cfg(name)
    m = build_model(cfg["arch"], cfg, TS.weights(name, s_ffn, s_qk))
    m.compute_dtype = dtype
    return m


def gpu_forward(name, s_ffn, s_qk, uncond, dtype, taps):
    """The drop-in module's forward -> (prediction, [encoder input, layer outputs] as [B (T + 1), d]) on the CPU."""
    d = dev()
    cfg = TS.case_cfg(name)
    m = model(name, s_ffn, s_qk, dtype)
    x, t, seedp, mfcc = TS.inputs(name)
    y = {"seed": seedp.to(d), "mfcc": mfcc.to(d)}
    if uncond:
        y["uncond"] = True
    eng = m._get_engine(d)
    eng.keep_taps(taps)
    out = m(x.to(d), t.to(d), y).cpu()
    got = []
    if taps:
        rows = x.shape[0] * (x.shape[-1] + 1)
        got = [eng.tap(i, 2 * rows, cfg["latent_dim"], d)[:rows].cpu() for i in range(TS.LAYERS + 1)]
        eng.keep_taps(False)
    return out, got


def oracle_taps(taps, dm):
    """The oracle's [S, B, d] taps in the kernels' [B S, d] layout, encoder input first."""
    names = ["enc_in"] + [f"seqTransEncoder.layers.{l}.out" for l in range(TS.LAYERS)]
    return [taps[n].permute(1, 0, 2).reshape(-1, dm) for n in names]


@pytest.mark.parametrize("s_ffn,s_qk", TS.SCALES)
@pytest.mark.parametrize("name", sorted(TS.CASES))
def test_fp32_forward_at_trained_scale(name, s_ffn, s_qk):
    dm = TS.case_cfg(name)["latent_dim"]
    for uncond in (False, True):
        out, taps = gpu_forward(name, s_ffn, s_qk, uncond, "fp32", taps=True)
        o64, t64 = TS.oracle(name, s_ffn, s_qk, uncond, "fp64")
        o32, t32 = TS.oracle(name, s_ffn, s_qk, uncond, "fp32")
        stages = list(zip(["encoder input"] + [f"layer {l}" for l in range(TS.LAYERS)], taps, oracle_taps(t64, dm), oracle_taps(t32, dm)))
        stages.append(("output", out, o64, o32))
        line = []
        for stage, got, want, ref32 in stages:
            floor, ours = rel_err(ref32, want), rel_err(got, want)
            line.append(f"{stage} {ours:.2e} (floor {floor:.2e})")
        print(f"\n[trained-scale fp32 {name} ({s_ffn}, {s_qk}) uncond={uncond}] " + ", ".join(line))
        for stage, got, want, ref32 in stages:
            floor, ours = rel_err(ref32, want), rel_err(got, want)
            assert ours < 10 * max(floor, 1e-7), (stage, ours, floor)
            assert ours < FWD_TOL, (stage, ours)


@pytest.mark.parametrize("arch", ["v1_tiny", "v2_tiny"])
def test_fp32_guided_forward_at_trained_scale(arch):
    """ClassifierFreeSampleModel at scale 2.5 on the (6, 3) weights against the float64 blend u + s (c - u) of the oracle."""
    from gesturediffusion_amd.model.cfg_sampler import ClassifierFreeSampleModel
    d = dev()
    x, t, seedp, mfcc = TS.inputs(arch)
    scale = torch.full((x.shape[0],), GUIDANCE)
    y = {"seed": seedp.to(d), "mfcc": mfcc.to(d), "scale": scale.to(d)}
    out = ClassifierFreeSampleModel(model(arch, 6, 3, "fp32"))(x.to(d), t.to(d), y).cpu()

    def blend(dtype):
        c, u = (TS.oracle(arch, 6, 3, uncond, dtype)[0].to(TS.TORCH_DT[dtype]) for uncond in (False, True))
        return (u + GUIDANCE * (c - u)).double()
    floor, ours = rel_err(blend("fp32"), blend("fp64")), rel_err(out, blend("fp64"))
    print(f"\n[trained-scale fp32 guided {arch} (6, 3)] {ours:.2e} (floor {floor:.2e})")
    assert ours < 10 * max(floor, 1e-7) and ours < FWD_TOL, (ours, floor)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("s_ffn,s_qk", TS.SCALES)
@pytest.mark.parametrize("name", HALF_CASES)
def test_half_forward_at_trained_scale(name, s_ffn, s_qk, dtype):
    res = []
    for uncond in (False, True):
        out, _ = gpu_forward(name, s_ffn, s_qk, uncond, dtype, taps=False)
        o64 = TS.oracle(name, s_ffn, s_qk, uncond, "fp64")[0]
        floor16 = rel_err(TS.oracle(name, s_ffn, s_qk, uncond, dtype)[0], o64)
        assert bool(torch.isfinite(out).all()), f"uncond={uncond}: a non-finite prediction"
        ours = rel_err(out, o64)
        print(f"\n[trained-scale {dtype} {name} ({s_ffn}, {s_qk}) uncond={uncond}] ours {ours:.2e}, floor16 {floor16:.2e}, "
              f"ratio {ours / floor16:.2f}")
        res.append((uncond, ours, floor16))
    for uncond, ours, floor16 in res:
        assert ours <= 2 * floor16, (uncond, ours, floor16)
