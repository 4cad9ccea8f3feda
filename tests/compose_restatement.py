"""CPU restatement of per-condition guidance for use_text models (include/gdx.h, gdx_set_guidance_compose) on top of
tests/text_restatement.py.  Test infrastructure; pinned by tests/golden/forward_text_compose.npz, which the reference's own
class wrote under zeroed inputs (tools/make_golden_compose.py).

The reference's mask_cond hands a dropped condition's Linear an all-zero input, so the four conditioning states are four plain
forwards: F (text + seed), S (text zeroed), X (seed zeroed), U (both zeroed)."""
import torch

import text_restatement as tr

JOINT, TEXT, SEED, SEED_TEXT, TEXT_SEED = range(5)                      # gdx.h GDX_GUIDE_*
MODES = {"joint": JOINT, "text": TEXT, "seed": SEED, "seed_text": SEED_TEXT, "text_seed": TEXT_SEED}
# the passes of a guided call in row-group order, F first
GROUPS = {JOINT: "FU", TEXT: "FS", SEED: "FX", SEED_TEXT: "FSU", TEXT_SEED: "FXU"}
CASES = tr.CASES
WEIGHT_SEED, RESPACING = 21, [20]


def dropped(y, tag):
    """y as pass `tag` (F, S, X or U) sees it: the dropped inputs zeroed in front of their Linear."""
    out = dict(y)
    if tag in "SU":
        out["text_embed"] = torch.zeros_like(y["text_embed"])
    if tag in "XU":
        out["seed"] = torch.zeros_like(y["seed"])
    return out


def passes(sd, cfg, x, t, y, tags="FSXU"):
    """{tag: the denoiser's output under that conditioning state}"""
    with torch.no_grad():
        return {tag: tr.forward(sd, cfg, x, t, dropped(y, tag)) for tag in tags}


def per_sample(s, like):
    return s.to(like.dtype).view(-1, *([1] * (like.dim() - 1)))


def compose(mode, p, scale, text_scale=None):
    """The guided prediction of `mode` from the passes p in p's dtype, every difference, product and sum on its own in the order
    gdx.h writes them.  Modes 0 .. 2: one scale.  3-pass modes: scale is the seed scale, text_scale the text's; the stage stepped
    to first gets s0."""
    g = GROUPS[mode]
    f, m = p["F"], p[g[1]]
    if len(g) == 2:
        return m + per_sample(scale, f) * (f - m)
    s0, s1 = (scale, text_scale) if mode == SEED_TEXT else (text_scale, scale)
    u = p["U"]
    return (u + per_sample(s0, f) * (m - u)) + per_sample(s1, f) * (f - m)


def packed(mode, scale, text_scale):
    """[2][B] in stage order: row 0 multiplies M - U, row 1 multiplies F - M."""
    return torch.stack([scale, text_scale] if mode == SEED_TEXT else [text_scale, scale])


def compose_forward(sd, cfg, x, t, y, mode):
    """ClassifierFreeSampleModel.forward under the new keys: y holds 'scale' and, in a 3-pass mode, 'text_scale'."""
    return compose(mode, passes(sd, cfg, x, t, y, GROUPS[mode]), y["scale"], y.get("text_scale"))


def case(g, name):
    """(cfg, weights, x, t, y) of a case of forward_text_compose.npz (`g`: the loaded archive); the weights are regenerated."""
    from gesturediffusion_amd.utils.init import init_state_dict
    cfg = tr.text_cfg(*CASES[name])
    sd = init_state_dict(cfg, seed=WEIGHT_SEED, perturb=True)
    y = {"seed": torch.from_numpy(g[name + ".seed"]), "mfcc": torch.from_numpy(g[name + ".mfcc"]),
         "text_embed": torch.from_numpy(g[name + ".text"])}
    return cfg, sd, torch.from_numpy(g[name + ".x"]), torch.from_numpy(g[name + ".t"]), y


def scalar_case(B=2, J=37, T=30, seed=31):
    """The shape whose J*T % 4 == 2 sends every pose-layout kernel down its scalar path: text_dim 40 / clip_dim 32 at 37 joints."""
    from gesturediffusion_amd.utils.init import init_state_dict, synthetic_inputs
    cfg = tr.text_cfg(40, 32, J=J)
    sd = init_state_dict(cfg, seed=WEIGHT_SEED, perturb=True)
    x, seedp, mfcc, text = synthetic_inputs(cfg, B, T, seed=seed)
    return cfg, sd, x, torch.tensor([7, 993, 500][:B]), {"seed": seedp, "mfcc": mfcc, "text_embed": text}
