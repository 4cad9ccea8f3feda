#!/usr/bin/env python3
"""Generate tests/golden/forward_pag.npz by running the REFERENCE's own MDM and MDM_Old with the self-attention map of chosen
encoder layers replaced by the identity -- the contrast pass of perturbed-attention guidance (Ahn et al. 2024, arXiv:2403.17377;
include/gdx.h gdx_set_attention_guidance).

Development-machine tool in the shape of tools/make_golden_compose.py: the reference is imported at run time (never copied) and
the archive holds DATA only -- inputs, the reference's outputs, noise tapes and loop results; the weights come from
init_state_dict(cfg, seed, perturb=True) on both sides.

The perturbation touches no arithmetic of the reference: seqTransEncoder.layers[l].self_attn.forward of a masked layer is wrapped
to call the ORIGINAL forward with an additive attn_mask that is 0 on the diagonal and -inf elsewhere.  nn.TransformerEncoderLayer
takes its slow path for batch_first=False, so the wrapped forward is what runs; the softmax row is then exactly (.., 0, 1, 0, ..),
and the module's output equals out_proj(v_proj(x)) bit for bit, asserted here on the layer's own input.

Cases (16 joints, latent_dim 128, 4 heads, ff_size 192, seed_poses 10, B = 3, T = 20, t = [7, 993, 500]):
  v2_l2_m1    MDM, 2 layers, layer 1 perturbed          v2_l3_m02   MDM, 3 layers, layers 0 and 2
  old_l2_m0   MDM_Old, 2 layers, layer 0
Per case: <case>.x / .seed / .mfcc / .t, <case>.F (the plain conditional pass), <case>.P (the perturbed pass) and <case>.U (the
reference's uncond pass).

Loops (v2_l2_m1): the reference's own p_sample_loop on [20] steps from a recorded tape, around a wrapper that calls the reference's
model two or three times and composes with torch's separate ops in the order gdx.h writes the rule:
  <case>.only_p20.tape / .out   g = P + s (F - P), s = fl32(1 + w), w = <case>.only_w
  <case>.cfg_p20.tape / .out    g = (U + s (F - U)) + w (F - P), s = <case>.cfg_s, w = <case>.cfg_w

The archive is written with fixed zip timestamps: the same machine regenerates it byte for byte.

Usage:  python tools/make_golden_pag.py --ref <checkout of the reference> [--out tests/golden]
"""
import argparse
import contextlib
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle", "tools"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import make_golden as mg  # noqa: E402
from make_golden_bpd import save_npz  # noqa: E402
from gesturediffusion_amd.utils.init import init_state_dict, synthetic_inputs  # noqa: E402

WEIGHT_SEED, INPUT_SEED, B, T = 23, 31, 3, 20
CASES = {"v2_l2_m1": ("mdm", 2, (1,)), "v2_l3_m02": ("mdm", 3, (0, 2)), "old_l2_m0": ("mdm_old", 2, (0,))}
LOOP_CASE = "v2_l2_m1"
LOOP = dict(respacing=[20], only_w=[3.0, 0.5, 1.25], cfg_s=[1.5, 2.5, 0.75], cfg_w=[3.0, -1.0, 2.25], tape_seed=2468)


def pag_cfg(arch, layers):
    return dict(arch=arch, njoints=16, nfeats=1, latent_dim=128, ff_size=192, num_layers=layers, num_heads=4, seed_poses=10)


@contextlib.contextmanager
def identity_attention(model, layers):
    """The reference model with the attention map of `layers` replaced by the identity, through the module's own forward."""
    saved = []
    for l in layers:
        attn = model.seqTransEncoder.layers[l].self_attn
        orig = attn.forward

        def forward(query, key, value, _orig=orig, _attn=attn, **kw):
            S = query.shape[0]
            mask = torch.full((S, S), float("-inf"), dtype=query.dtype)
            mask.fill_diagonal_(0.0)
            kw["attn_mask"] = mask
            out = _orig(query, key, value, **kw)
            d = query.shape[-1]
            v = F.linear(value, _attn.in_proj_weight[2 * d:], _attn.in_proj_bias[2 * d:])
            assert torch.equal(out[0], F.linear(v, _attn.out_proj.weight, _attn.out_proj.bias)), "identity attention is out_proj(v_proj(x))"
            return out
        attn.forward = forward
        saved.append(attn)
    try:
        yield model
    finally:
        for attn in saved:
            del attn.forward                       # the instance attribute: the class's forward is back


class Guided(torch.nn.Module):
    """What the reference's sampling loop calls: the passes of one guided step, composed in the rule's order."""

    def __init__(self, model, layers, kind):
        super().__init__()
        self.model, self.layers, self.kind = model, layers, kind

    def forward(self, x, timesteps, y=None):
        cond = {"seed": y["seed"], "mfcc": y["mfcc"]}
        f = self.model(x, timesteps, cond)
        with identity_attention(self.model, self.layers):
            p = self.model(x, timesteps, cond)
        w = y["pag_scale"].view(-1, 1, 1, 1)
        if self.kind == "only":
            return p + (1.0 + w) * (f - p)
        u = self.model(x, timesteps, dict(cond, uncond=True))
        return (u + y["scale"].view(-1, 1, 1, 1) * (f - u)) + w * (f - p)


def gen(mods, out):
    gd, rs = mods[3], mods[4]
    d = {}
    for name, (arch, L, layers) in CASES.items():
        cfg = pag_cfg(arch, L)
        sd = init_state_dict(cfg, seed=WEIGHT_SEED, perturb=True)
        x, seedp, mfcc = synthetic_inputs(cfg, B, T, seed=INPUT_SEED)
        t = torch.tensor([7, 993, 500])
        m = mg.build_ref_model(mods, cfg, sd)
        y = {"seed": seedp, "mfcc": mfcc}
        d.update({f"{name}.x": x.numpy(), f"{name}.seed": seedp.numpy(), f"{name}.mfcc": mfcc.numpy(), f"{name}.t": t.numpy()})
        with torch.no_grad():
            d[f"{name}.F"] = m(x, t, y).contiguous().numpy()
            with identity_attention(m, layers):
                d[f"{name}.P"] = m(x, t, y).contiguous().numpy()
            again = m(x, t, y).contiguous().numpy()
            d[f"{name}.U"] = m(x, t, dict(y, uncond=True)).contiguous().numpy()
        assert np.array_equal(again, d[f"{name}.F"]), "the perturbation is undone"
        assert not np.array_equal(d[f"{name}.P"], d[f"{name}.F"])
        if name != LOOP_CASE:
            continue
        df = mg.make_diffusion(gd, rs, LOOP["respacing"])
        shape = (B, cfg["njoints"], 1, T)
        g = torch.Generator().manual_seed(LOOP["tape_seed"])
        for kind in ("only", "cfg"):
            tape = torch.randn(LOOP["respacing"][0] + 1, *shape, generator=g)
            yy = dict(y, pag_scale=torch.tensor(LOOP[f"{kind}_w"]))
            d[f"{name}.{kind}_w"] = yy["pag_scale"].numpy()
            if kind == "cfg":
                yy["scale"] = torch.tensor(LOOP["cfg_s"])
                d[f"{name}.cfg_s"] = yy["scale"].numpy()
            with mg.TapeNoise(tape[1:]), torch.no_grad():
                r = df.p_sample_loop(Guided(m, layers, kind), shape, noise=tape[0].clone(), clip_denoised=False, progress=False,
                                     model_kwargs={"y": yy})
            d.update({f"{name}.{kind}_p20.tape": tape.numpy(), f"{name}.{kind}_p20.out": r.numpy()})
    for k, v in d.items():
        assert np.isfinite(v).all(), k
    path = os.path.join(out, "forward_pag.npz")
    save_npz(path, d)
    return path


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    torch.set_num_threads(8)
    path = gen(mg.import_reference(args.ref), args.out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
