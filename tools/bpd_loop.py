#!/usr/bin/env python3
"""ms/step of calc_bpd_loop next to p_sample_loop at the same shape, in one process:
    python tools/bpd_loop.py [--config 2|1|genea] [--steps 200] [--repeats 3] [--stepwise] [--out profiles/FILE.jsonl]
Both loops run the same forward once per step; the sampling loop adds one update kernel, the bound q_sample + gdx_bpd_terms
(two kernels).  Each loop is warmed once at the timed shape, then timed `repeats` times, alternating the two, around a device
synchronise; the median is reported with the spread.  --stepwise also times calc_bpd_loop(fused=False), the step-wise
protocol from Python.  One JSON line per configuration; kernel-level numbers come from running this under
`rocprofv3 --kernel-trace --stats` (tools/kstats.py) in a run of its own."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from bench import PRESETS, build_model  # noqa: E402
from gesturediffusion_amd.diffusion import gaussian_diffusion as gd  # noqa: E402
from gesturediffusion_amd.diffusion.respace import SpacedDiffusion, space_timesteps  # noqa: E402
from gesturediffusion_amd.model.cfg_sampler import ClassifierFreeSampleModel  # noqa: E402
from gesturediffusion_amd.utils.init import synthetic_inputs  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="2", choices=["1", "2", "genea"])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--stepwise", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    p = PRESETS[a.config]
    dev = torch.device("cuda:0")
    model, cfg, _ = build_model(p["arch"], p["J"], p["d"], p["L"], dev)
    model.compute_dtype = p["dtype"]
    B, T, J = p["batch"], p["T"], p["J"]
    df = SpacedDiffusion(use_timesteps=space_timesteps(1000, [a.steps]), betas=gd.get_named_beta_schedule("cosine", 1000),
                         model_mean_type=gd.ModelMeanType.START_X, model_var_type=gd.ModelVarType.FIXED_SMALL,
                         loss_type=gd.LossType.MSE)
    x, seedp, mfcc = synthetic_inputs(cfg, B, T, seed=10)
    y = {"seed": seedp.to(dev), "mfcc": mfcc.to(dev)}
    m = model
    if p["cfg"]:
        y["scale"] = torch.full((B,), 2.5, device=dev)
        m = ClassifierFreeSampleModel(model)
    xs = (x * 0.6).to(dev)
    kw = dict(clip_denoised=False, model_kwargs={"y": y}, rng="philox", philox_seed=1)
    loops = {"p_sample_loop": lambda: df.p_sample_loop(m, (B, J, 1, T), **kw),
             "calc_bpd_loop": lambda: df.calc_bpd_loop(m, xs, **kw)["total_bpd"]}
    if a.stepwise:
        loops["calc_bpd_loop_stepwise"] = lambda: df.calc_bpd_loop(m, xs, fused=False, **kw)["total_bpd"]
    first = {k: timed(fn)[1] for k, fn in loops.items()}                       # warm-up at the timed shape
    ms = {k: [] for k in loops}
    for _ in range(a.repeats):
        for k, fn in loops.items():                                            # alternate the loops inside each repeat
            t, r = timed(fn)
            assert torch.equal(r, first[k]) and torch.isfinite(r).all(), k
            ms[k].append(t / a.steps)
    rec = dict(tool="bpd_loop", config=a.config, label=p["label"], arch=p["arch"], B=B, T=T, J=J, d=p["d"], dtype=p["dtype"],
               guidance=bool(p["cfg"]), steps=a.steps, repeats=a.repeats, device=torch.cuda.get_device_name(0))
    for k, v in ms.items():
        rec[k + "_ms_per_step"] = round(statistics.median(v), 5)
        rec[k + "_ms_per_step_min_max"] = [round(min(v), 5), round(max(v), 5)]
    rec["bpd_over_sample"] = round(rec["calc_bpd_loop_ms_per_step"] / rec["p_sample_loop_ms_per_step"], 4)
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
