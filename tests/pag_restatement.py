"""CPU restatement of perturbed-attention guidance (include/gdx.h, gdx_set_attention_guidance) on top of the unchanged
oracle/mdm_forward.py.  Test infrastructure; pinned by tests/golden/forward_pag.npz, which the reference's own MDM and MDM_Old
wrote with an identity attention mask on the chosen layers (tools/make_golden_pag.py).

With the attention map replaced by the identity every token attends to itself alone: the context of a perturbed layer is the V
third of its in-projection, and everything behind it (out-projection, residual, LayerNorm, FFN) is the plain layer's."""
import contextlib

import torch
import torch.nn.functional as F

from oracle import mdm_forward as omf

OFF, ONLY, CFG = range(3)                                                # gdx.h GDX_PAG_*
# case -> (arch, encoder layers, the perturbed ones) of forward_pag.npz
CASES = {"v2_l2_m1": ("mdm", 2, (1,)), "v2_l3_m02": ("mdm", 3, (0, 2)), "old_l2_m0": ("mdm_old", 2, (0,))}
LOOP_CASE = "v2_l2_m1"
WEIGHT_SEED, RESPACING = 23, [20]


def pag_cfg(arch, layers):
    return dict(arch=arch, njoints=16, nfeats=1, latent_dim=128, ff_size=192, num_layers=layers, num_heads=4, seed_poses=10)


def layer_mask(layers):
    return sum(1 << l for l in layers)


def identity_layer(p, prefix, x, taps=None):
    """omf.encoder_layer with ctx = V.  x: [S, B, d]."""
    d = x.shape[-1]
    qkv = F.linear(x, p[prefix + "self_attn.in_proj_weight"], p[prefix + "self_attn.in_proj_bias"])
    ctx = qkv[..., 2 * d:]
    sa = F.linear(ctx, p[prefix + "self_attn.out_proj.weight"], p[prefix + "self_attn.out_proj.bias"])
    x = F.layer_norm(x + sa, (d,), p[prefix + "norm1.weight"], p[prefix + "norm1.bias"], 1e-5)
    ff = F.linear(F.gelu(F.linear(x, p[prefix + "linear1.weight"], p[prefix + "linear1.bias"])),
                  p[prefix + "linear2.weight"], p[prefix + "linear2.bias"])
    x = F.layer_norm(x + ff, (d,), p[prefix + "norm2.weight"], p[prefix + "norm2.bias"], 1e-5)
    if taps is not None:
        taps[prefix + "ctx"] = ctx
        taps[prefix + "out"] = x
    return x


def layer(p, l, x, nhead, perturbed):
    """Encoder layer l on x [S, B, d], plain or with identity attention."""
    prefix = f"seqTransEncoder.layers.{l}."
    return identity_layer(p, prefix, x) if perturbed else omf.encoder_layer(p, prefix, x, nhead)


@contextlib.contextmanager
def perturbed(layers):
    """While open, omf's forwards run identity attention in encoder layers `layers` (omf.encoder is swapped and put back)."""
    plain = omf.encoder

    def encoder(p, x, num_layers, nhead, taps=None):
        for l in range(num_layers):
            prefix = f"seqTransEncoder.layers.{l}."
            x = identity_layer(p, prefix, x, taps) if l in layers else omf.encoder_layer(p, prefix, x, nhead, taps)
        return x
    omf.encoder = encoder
    try:
        yield
    finally:
        omf.encoder = plain


def passes(sd, cfg, x, t, y, layers, tags="FPU"):
    """{tag: the denoiser's output}: F the conditional pass, P the perturbed one, U the unconditional one."""
    cond = {"seed": y["seed"], "mfcc": y["mfcc"]}
    out = {}
    with torch.no_grad():
        if "F" in tags:
            out["F"] = omf.forward(sd, cfg, x, t, cond)
        if "P" in tags:
            with perturbed(layers):
                out["P"] = omf.forward(sd, cfg, x, t, cond)
        if "U" in tags:
            out["U"] = omf.forward(sd, cfg, x, t, dict(cond, uncond=True))
    return out


def per_sample(s, like):
    return s.to(like.dtype).view(-1, *([1] * (like.dim() - 1)))


def compose_only(p, s):
    """GDX_PAG_ONLY: g = P + s*(F - P), every difference, product and sum on its own."""
    return p["P"] + per_sample(s, p["F"]) * (p["F"] - p["P"])


def compose_cfg(p, s0, s1):
    """GDX_PAG_CFG: g = (U + s0*(F - U)) + s1*(F - P)."""
    f = p["F"]
    return (p["U"] + per_sample(s0, f) * (f - p["U"])) + per_sample(s1, f) * (f - p["P"])


def guided_forward(sd, cfg, x, t, y, layers, kind):
    """The wrappers' forward: PerturbedAttentionSampleModel (ONLY: y['pag_scale'] = w, the operand is fl32(1 + w)) or
    ClassifierFreeSampleModel with y['scale'] and y['pag_scale'] (CFG)."""
    if kind == ONLY:
        return compose_only(passes(sd, cfg, x, t, y, layers, "FP"), (1.0 + y["pag_scale"].float()).to(x.dtype))
    return compose_cfg(passes(sd, cfg, x, t, y, layers), y["scale"], y["pag_scale"])


def case(g, name):
    """(cfg, weights, x, t, y, layers) of a case of forward_pag.npz (`g`: the loaded archive); the weights are regenerated."""
    from gesturediffusion_amd.utils.init import init_state_dict
    arch, L, layers = CASES[name]
    cfg = pag_cfg(arch, L)
    sd = init_state_dict(cfg, seed=WEIGHT_SEED, perturb=True)
    y = {"seed": torch.from_numpy(g[name + ".seed"]), "mfcc": torch.from_numpy(g[name + ".mfcc"])}
    return cfg, sd, torch.from_numpy(g[name + ".x"]), torch.from_numpy(g[name + ".t"]), y, layers
