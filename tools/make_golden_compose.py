#!/usr/bin/env python3
"""Generate tests/golden/forward_text_compose.npz by running the REFERENCE's MDM(use_text=True) under each of the four
conditioning states its trainer produces (mask_cond is drawn once for the text features and once for the seed poses,
model/mdm.py:121,127,242-250).

Development-machine tool in the shape of tools/make_golden_text.py, whose stand-in for CLIP and model builder it imports: the
reference is imported at run time (never copied) and the archive holds DATA only -- inputs, recorded text features and the
reference's outputs; the weights come from init_state_dict(cfg, seed, perturb=True) on both sides.

mask_cond hands a dropped condition's Linear an all-zero input.  The reference's class is therefore given, per case,
  F  the recorded features and the seed poses          S  zeroed features, the seed poses
  X  the recorded features, a zero seed                U  both zeroed
and <case>.F / .S / .X / .U are its outputs (U is also what its own `uncond` flag gives, asserted here).

Cases (16 joints, one layer, ff_size 192, seed_poses 10, latent_dim 128, B = 3, T = 20, t = [7, 993, 500]):
  mdm_128_t64   text_dim 64, clip_dim 512          mdm_128_t40   text_dim 40, clip_dim 32
Inputs per case: <case>.x / .seed / .mfcc / .t / .text.

Loops (mdm_128_t64): the reference's own p_sample_loop on [20] steps, noise tape <case>.<order>_p20.tape, around a wrapper that
calls the reference's model three times and composes g = U + s0*(M - U) + s1*(F - M) with torch's separate ops:
  <case>.seed_text_p20.out   M = S, s0 = .seed_scale, s1 = .text_scale
  <case>.text_seed_p20.out   M = X, s0 = .text_scale, s1 = .seed_scale
with the two different scale vectors <case>.seed_scale / .text_scale [B].

The archive is written with fixed zip timestamps: the same machine regenerates it byte for byte.

Usage:  python tools/make_golden_compose.py --ref <checkout of the reference> [--out tests/golden]
"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle", "tools"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import make_golden as mg  # noqa: E402
from make_golden_bpd import save_npz  # noqa: E402
from make_golden_text import CASES, Recorded, build_ref_text_model, text_cfg  # noqa: E402
from gesturediffusion_amd.utils.init import init_state_dict, synthetic_inputs  # noqa: E402

WEIGHT_SEED, INPUT_SEED, B, T = 21, 29, 3, 20
LOOP = dict(respacing=[20], seed_scale=[1.5, 2.5, 0.75], text_scale=[3.0, 1.0, 2.25], tape_seed=1357)


class Composed(torch.nn.Module):
    """What the reference's sampling loop calls: three passes of its model, the middle one with the text (order "seed_text") or
    the seed (order "text_seed") zeroed, composed in stage order."""

    def __init__(self, model, rec, order):
        super().__init__()
        self.model, self.rec, self.order = model, rec, order

    def forward(self, x, timesteps, y=None):
        text = self.rec.table
        zero_text, zero_seed = torch.zeros_like(text), torch.zeros_like(y["seed"])
        s_seed, s_text = (y[k].view(-1, 1, 1, 1) for k in ("scale", "text_scale"))

        def run(feats, seed):
            out = self.model(x, timesteps, {"seed": seed, "mfcc": y["mfcc"], "text": self.rec.names(feats)})
            self.rec.names(text)
            return out
        f, u = run(text, y["seed"]), run(zero_text, zero_seed)
        if self.order == "seed_text":
            m, s0, s1 = run(zero_text, y["seed"]), s_seed, s_text
        else:
            m, s0, s1 = run(text, zero_seed), s_text, s_seed
        return (u + s0 * (m - u)) + s1 * (f - m)


def gen(mods, out):
    gd, rs = mods[3], mods[4]
    rec = Recorded()
    rec.install(sys.modules["clip"])
    d = {}
    for name, (td, cd, _) in CASES.items():
        cfg = text_cfg(td, cd)
        sd = init_state_dict(cfg, seed=WEIGHT_SEED, perturb=True)
        x, seedp, mfcc, text = synthetic_inputs(cfg, B, T, seed=INPUT_SEED)
        t = torch.tensor([7, 993, 500])
        m = build_ref_text_model(mods, cfg, sd)
        d.update({f"{name}.x": x.numpy(), f"{name}.seed": seedp.numpy(), f"{name}.mfcc": mfcc.numpy(), f"{name}.t": t.numpy(),
                  f"{name}.text": text.numpy()})
        zt, zs = torch.zeros_like(text), torch.zeros_like(seedp)
        with torch.no_grad():
            for tag, feats, sp in (("F", text, seedp), ("S", zt, seedp), ("X", text, zs), ("U", zt, zs)):
                d[f"{name}.{tag}"] = m(x, t, {"seed": sp, "mfcc": mfcc, "text": rec.names(feats)}).contiguous().numpy()
            un = m(x, t, {"seed": seedp, "mfcc": mfcc, "text": rec.names(text), "uncond": True}).contiguous().numpy()
        assert np.array_equal(un, d[f"{name}.U"]), "zeroed inputs are what the reference's uncond flag gives"
        if name != "mdm_128_t64":
            continue
        df = mg.make_diffusion(gd, rs, LOOP["respacing"])
        shape = (B, cfg["njoints"], 1, T)
        g = torch.Generator().manual_seed(LOOP["tape_seed"])
        s_seed, s_text = torch.tensor(LOOP["seed_scale"]), torch.tensor(LOOP["text_scale"])
        d.update({f"{name}.seed_scale": s_seed.numpy(), f"{name}.text_scale": s_text.numpy()})
        for order in ("seed_text", "text_seed"):
            tape = torch.randn(LOOP["respacing"][0] + 1, *shape, generator=g)
            rec.names(text)
            y = {"seed": seedp, "mfcc": mfcc, "scale": s_seed, "text_scale": s_text}
            with mg.TapeNoise(tape[1:]), torch.no_grad():
                r = df.p_sample_loop(Composed(m, rec, order), shape, noise=tape[0].clone(), clip_denoised=False, progress=False,
                                     model_kwargs={"y": y})
            d.update({f"{name}.{order}_p20.tape": tape.numpy(), f"{name}.{order}_p20.out": r.numpy()})
    for k, v in d.items():
        assert np.isfinite(v).all(), k
    path = os.path.join(out, "forward_text_compose.npz")
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
