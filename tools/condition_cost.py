#!/usr/bin/env python3
"""What one conditioning costs, with and without text: python tools/condition_cost.py [B] [T] [J] [d] [layers]
(defaults: the GENEA chunk shape, B = 41, T = 120, J = 498, d = 256).  gdx_set_condition on a no-text model and
gdx_set_condition_text on a use_text one (text_dim 64, clip_dim 512), each called uncached `reps` times between two
synchronisations, median of 5 rounds.  A one-off cost per chunk: one call in front of a loop of hundreds of steps."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from gesturediffusion_amd.model.mdm import MDM  # noqa: E402
from gesturediffusion_amd.utils.init import init_state_dict, synthetic_inputs  # noqa: E402

B, T, J, d, L = (int(sys.argv[i]) if len(sys.argv) > i else v for i, v in ((1, 41), (2, 120), (3, 498), (4, 256), (5, 8)))
dev = torch.device("cuda:0")
REPS = 200


def model_of(cfg):
    m = MDM(njoints=J, nfeats=1, pose_rep="rot6d", data_rep="genea_vec", latent_dim=d, ff_size=1024, num_layers=L, num_heads=4,
            text_dim=cfg.get("text_dim", 64), clip_dim=cfg.get("clip_dim", 512), cond_mask_prob=0.1, dataset="genea2023",
            use_text="text_dim" in cfg, mfcc_input=True, seed_poses=10)
    m.load_state_dict(init_state_dict(cfg, seed=0), strict=False)
    return m.to(dev).eval()


def cost(cfg):
    m = model_of(cfg)
    inputs = [v.to(dev) for v in synthetic_inputs(cfg, B, T, seed=10)]
    x, seedp, mfcc, text = inputs + [None] * (4 - len(inputs))
    eng = m._get_engine(dev)
    eng.prepare(B, T)
    rounds = []
    for _ in range(6):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(REPS):
            eng.set_condition(seedp, mfcc, text=text, cache=False)
        torch.cuda.synchronize()
        rounds.append((time.perf_counter() - t0) / REPS * 1e6)
    return statistics.median(rounds[1:])                      # the first round warms up


base = dict(arch="mdm", njoints=J, nfeats=1, latent_dim=d, ff_size=1024, num_layers=L, num_heads=4, seed_poses=10)
plain, text = cost(base), cost(dict(base, text_dim=64, clip_dim=512))
print(f"B={B} T={T} J={J} d={d}: gdx_set_condition {plain:.1f} us, gdx_set_condition_text {text:.1f} us per call "
      f"(median of 5 rounds of {REPS} uncached calls)", flush=True)
