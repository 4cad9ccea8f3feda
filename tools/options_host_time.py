#!/usr/bin/env python3
"""What one call of the guided step-wise forward costs, reading y included:
python tools/options_host_time.py [B] [T] [J] [d] [layers] (defaults: the GENEA chunk shape, B = 41, T = 120, J = 498, d = 256).
ClassifierFreeSampleModel.forward with the same y on every call, as a step-wise loop of 1000 steps makes it: 5 rounds of `REPS`
calls between two synchronisations (the whole call), and the host's share of it (the clock read in front of the second
synchronisation).  Run it on two trees alternating to compare them."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from gesturediffusion_amd.model.cfg_sampler import ClassifierFreeSampleModel  # noqa: E402
from gesturediffusion_amd.model.mdm import MDM  # noqa: E402
from gesturediffusion_amd.utils.init import init_state_dict, synthetic_inputs  # noqa: E402

B, T, J, d, L = (int(sys.argv[i]) if len(sys.argv) > i else v for i, v in ((1, 41), (2, 120), (3, 498), (4, 256), (5, 8)))
dev = torch.device("cuda:0")
REPS = 200

cfg = dict(arch="mdm", njoints=J, nfeats=1, latent_dim=d, ff_size=1024, num_layers=L, num_heads=4, seed_poses=10)
m = MDM(njoints=J, nfeats=1, pose_rep="rot6d", data_rep="genea_vec", latent_dim=d, ff_size=1024, num_layers=L, num_heads=4,
        cond_mask_prob=0.1, dataset="genea2023", mfcc_input=True, seed_poses=10)
m.load_state_dict(init_state_dict(cfg, seed=0), strict=False)
model = ClassifierFreeSampleModel(m.to(dev).eval())
x, seedp, mfcc = (v.to(dev) for v in synthetic_inputs(cfg, B, T, seed=10))
y = {"seed": seedp, "mfcc": mfcc, "scale": torch.full((B,), 2.5, device=dev)}
t = torch.full((B,), 500, device=dev, dtype=torch.long)
whole, host = [], []
with torch.no_grad():
    for _ in range(6):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(REPS):
            model(x, t, y=y)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        whole.append((time.perf_counter() - t0) / REPS * 1e6)
        host.append((t1 - t0) / REPS * 1e6)
whole, host = whole[1:], host[1:]                             # the first round warms up
print(f"B={B} T={T} J={J} d={d}: guided forward {statistics.median(whole):.1f} us per call (min {min(whole):.1f}, "
      f"max {max(whole):.1f}), host share {statistics.median(host):.1f} us (min {min(host):.1f}, max {max(host):.1f}); "
      f"median of 5 rounds of {REPS} calls", flush=True)
