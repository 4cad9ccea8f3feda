#!/usr/bin/env python3
"""Generate tests/golden/forward_heads_tiny.npz by running the REFERENCE's forward at head widths 96 and 192.

Development-machine tool: imports the reference at run time through the shims of oracle/tools/make_golden.py (never
copied) and writes DATA only -- inputs and the reference's forward outputs.  The weights come from
init_state_dict(cfg, seed, perturb=True) on both sides, so the file holds none.

The reference fixes num_heads = 4 (utils/model_util.py get_model_args) and lets --latent_dim vary, so latent_dim 384 / 768
are head widths 96 / 192 in the encoder and, at the V2 front end's cl_head = 8, local head widths 48 / 96.

Cases (ff_size 192, one layer, 16 joints, B = 2, T = 20, t = [7, 993]; conditional and unconditional):
  mdm_old_384   MDM_Old, latent_dim 384
  mdm_384       MDM,     latent_dim 384
  mdm_768       MDM,     latent_dim 768
Per case: <case>.x / .seed / .mfcc / .t, <case>.cond.out, <case>.uncond.out and <case>.cond.out_fp64 (the same model in
fp64: the reference's own fp32 round-off).

The archive is written with fixed zip timestamps: the same machine regenerates it byte for byte.

Usage:  python tools/make_golden_heads.py --ref <checkout of the reference> [--out tests/golden]
"""
import argparse
import os
import sys

import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle", "tools"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import make_golden as mg  # noqa: E402
from make_golden_bpd import save_npz  # noqa: E402
from gesturediffusion_amd.utils.init import init_state_dict, synthetic_inputs  # noqa: E402

CASES = {"mdm_old_384": ("mdm_old", 384), "mdm_384": ("mdm", 384), "mdm_768": ("mdm", 768)}
WEIGHT_SEED, INPUT_SEED, B, T = 11, 13, 2, 20


def heads_cfg(arch, d):
    return dict(arch=arch, njoints=16, nfeats=1, latent_dim=d, ff_size=192, num_layers=1, num_heads=4, seed_poses=10)


def gen(mods, out):
    d = {}
    for name, (arch, dim) in CASES.items():
        cfg = heads_cfg(arch, dim)
        sd = init_state_dict(cfg, seed=WEIGHT_SEED, perturb=True)
        x, seedp, mfcc = synthetic_inputs(cfg, B, T, seed=INPUT_SEED)
        t = torch.tensor([7, 993])
        m = mg.build_ref_model(mods, cfg, sd)
        d.update({f"{name}.x": x.numpy(), f"{name}.seed": seedp.numpy(), f"{name}.mfcc": mfcc.numpy(), f"{name}.t": t.numpy()})
        with torch.no_grad():
            d[f"{name}.cond.out"] = m(x, t, {"seed": seedp, "mfcc": mfcc}).contiguous().numpy()
            d[f"{name}.uncond.out"] = m(x, t, {"seed": seedp, "mfcc": mfcc, "uncond": True}).contiguous().numpy()
            m64 = mg.build_ref_model(mods, cfg, sd, double=True)
            d[f"{name}.cond.out_fp64"] = m64(x.double(), t, {"seed": seedp.double(), "mfcc": mfcc.double()}).contiguous().numpy()
    path = os.path.join(out, "forward_heads_tiny.npz")
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
