"""Shared by tests/test_gpu_trained_scale.py and tests/test_trained_scale_host.py: weights away from initialisation scale, and
the CPU oracle (oracle/mdm_forward.py) run in float64, float32 and the 16-bit dtypes on them.

init_state_dict draws linear1.weight ~ U(+-1/sqrt(d)) on a LayerNorm output, so FFN-1's pre-activations (the GELU arguments)
have a standard deviation of about 0.58 and never leave [-3, 3], and the self-attention's softmax rows stay near uniform.
trained_scale multiplies linear1 by s_ffn and the q and k rows of in_proj by s_qk (logits grow s_qk^2-fold): at (6, 3) a
fifth of the GELU arguments lie beyond +-4.24, where the 16-bit kernels' erf is clamped, and they span about +-14."""
import functools

import torch

# name: (arch, latent_dim, ff_size, num_heads, T, B); two layers, 16 joints
CASES = {
    "v1_tiny": ("mdm_old", 128, 256, 4, 20, 2),
    "v2_tiny": ("mdm", 128, 256, 4, 20, 2),
    "v1_d512": ("mdm_old", 512, 1024, 8, 37, 2),          # persistent fp32 GEMM, attention3
    "v2_d512": ("mdm", 512, 1024, 8, 37, 2),
    "v1_d96": ("mdm_old", 96, 160, 3, 37, 2),             # N % 64 != 0: csrc/gemm.hip
}
SCALES = [(6, 3), (12, 4)]
LAYERS = 2
CLAMP = 4.24                    # 3 sqrt(2): beyond it csrc/gemmh.hip gelu2 clamps its erf argument
TORCH_DT = {"fp64": torch.float64, "fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}


def case_cfg(name):
    arch, d, ff, heads, T, B = CASES[name]
    return dict(arch=arch, njoints=16, nfeats=1, latent_dim=d, ff_size=ff, num_layers=LAYERS, num_heads=heads, seed_poses=10)


def case_frames(name):
    """V2's local attention needs T to be a multiple of its window (10): the T = 37 cases run it at T = 40."""
    arch, T = CASES[name][0], CASES[name][4]
    return T if arch == "mdm_old" or T % 10 == 0 else (T + 9) // 10 * 10


def trained_scale(sd, cfg, s_ffn, s_qk):
    """A copy of the state dict with every linear1.weight / linear1.bias times s_ffn and the first 2 d rows (q and k) of every
    in_proj_weight / in_proj_bias times s_qk."""
    d = cfg["latent_dim"]
    out = {k: v.clone() for k, v in sd.items()}
    for k, v in out.items():
        if ".linear1." in k:
            v *= s_ffn
        elif k.endswith("in_proj_weight") or k.endswith("in_proj_bias"):
            v[: 2 * d] *= s_qk
    return out


@functools.lru_cache(maxsize=None)
def weights(name, s_ffn, s_qk):
    from gesturediffusion_amd.utils.init import init_state_dict
    cfg = case_cfg(name)
    return trained_scale(init_state_dict(cfg, seed=41, perturb=True), cfg, s_ffn, s_qk)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(x, timesteps, seed poses, mfcc) on the CPU in float32."""
    from gesturediffusion_amd.utils.init import synthetic_inputs
    B = CASES[name][5]
    x, seedp, mfcc = synthetic_inputs(case_cfg(name), B, case_frames(name), seed=7)
    return x, torch.tensor([17, 803][:B]), seedp, mfcc


@functools.lru_cache(maxsize=None)
def oracle(name, s_ffn, s_qk, uncond, dtype):
    """The oracle in TORCH_DT[dtype] on the float32 weights and inputs converted to it -> (output, taps), both float64.
    Nothing here touches torch's default dtype."""
    from oracle import mdm_forward as omf
    dt = TORCH_DT[dtype]
    cfg = case_cfg(name)
    p = {k: v.to(dt) for k, v in weights(name, s_ffn, s_qk).items()}
    x, t, seedp, mfcc = inputs(name)
    y = {"seed": seedp.to(dt), "mfcc": mfcc.to(dt)}
    if uncond:
        y["uncond"] = True
    taps = {}
    with torch.no_grad():
        out = omf.forward(p, cfg, x.to(dt), t, y, taps)
    assert out.dtype == dt and all(v.dtype == dt for v in taps.values()), "the oracle left the requested dtype"
    return out.double(), {k: v.double() for k, v in taps.items()}


def ffn1_preactivations(name, s_ffn, s_qk, uncond=False, dtype="fp32"):
    """Every GELU argument of the case, all layers, as one float64 vector."""
    taps = oracle(name, s_ffn, s_qk, uncond, dtype)[1]
    return torch.cat([taps[f"seqTransEncoder.layers.{l}.ffn1"].flatten() for l in range(LAYERS)])
