#!/usr/bin/env python3
"""ms/step of plms_sample_loop (order 2 by default) at a benchmark shape, in one process:
    python tools/plms_loop.py [--config 1|genea|2] [--dtype fp32|fp16|bf16] [--steps 50] [--order 2] [--repeats 5]
                              [--stepwise] [--out profiles/FILE.jsonl]
The loop runs once as a warm-up at the timed shape, then `repeats` times between two events on the stream; the median is
reported with the spread, per step of the respacing (the first step runs two forwards, so a loop of n steps holds n + 1).
The script only uses plms_sample_loop's reference keywords unless the build has the in-library loop, so it also runs on a
checkout from before gdx_plms_loop and times the step-wise protocol there (an A/B of two checkouts on one box); --stepwise
adds plms_sample_loop(fused=False) of this build.  One JSON line per run; kernel-level numbers come from running this under
`rocprofv3 --kernel-trace --stats` in a run of its own."""
import argparse
import inspect
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from bench import PRESETS, build_model  # noqa: E402
from gesturediffusion_amd.diffusion import gaussian_diffusion as gd  # noqa: E402
from gesturediffusion_amd.diffusion.respace import SpacedDiffusion, space_timesteps  # noqa: E402
from gesturediffusion_amd.model.cfg_sampler import ClassifierFreeSampleModel  # noqa: E402
from gesturediffusion_amd.utils.init import synthetic_inputs  # noqa: E402


def timed(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    r = fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="1", choices=["1", "2", "genea"])
    ap.add_argument("--dtype", default=None, choices=["fp32", "fp16", "bf16"])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--order", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--stepwise", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    p = PRESETS[a.config]
    dtype = a.dtype or p["dtype"]
    dev = torch.device("cuda:0")
    model, cfg, _ = build_model(p["arch"], p["J"], p["d"], p["L"], dev)
    model.compute_dtype = dtype
    B, T, J = p["batch"], p["T"], p["J"]
    df = SpacedDiffusion(use_timesteps=space_timesteps(1000, [a.steps]), betas=gd.get_named_beta_schedule("cosine", 1000),
                         model_mean_type=gd.ModelMeanType.START_X, model_var_type=gd.ModelVarType.FIXED_SMALL,
                         loss_type=gd.LossType.MSE)
    x, seedp, mfcc = synthetic_inputs(cfg, B, T, seed=10)
    x = x.to(dev)
    y = {"seed": seedp.to(dev), "mfcc": mfcc.to(dev)}
    m = model
    if p["cfg"]:
        y["scale"] = torch.full((B,), 2.5, device=dev)
        m = ClassifierFreeSampleModel(model)
    kw = dict(noise=x, clip_denoised=False, model_kwargs={"y": y}, order=a.order)
    in_library = "fused" in inspect.signature(df.plms_sample_loop).parameters
    loops = {"plms_sample_loop": lambda: df.plms_sample_loop(m, (B, J, 1, T), **kw)}
    if a.stepwise and in_library:
        loops["plms_sample_loop_stepwise"] = lambda: df.plms_sample_loop(m, (B, J, 1, T), fused=False, **kw)
    first = {k: timed(fn)[1] for k, fn in loops.items()}                       # warm-up at the timed shape
    ms = {k: [] for k in loops}
    for _ in range(a.repeats):
        for k, fn in loops.items():                                            # alternate the loops inside each repeat
            t, r = timed(fn)
            assert torch.equal(r, first[k]) and torch.isfinite(r).all(), k
            ms[k].append(t / a.steps)
    if len(first) == 2:
        assert torch.equal(first["plms_sample_loop"], first["plms_sample_loop_stepwise"])
    rec = dict(tool="plms_loop", config=a.config, label=p["label"], arch=p["arch"], B=B, T=T, J=J, d=p["d"], dtype=dtype,
               guidance=bool(p["cfg"]), steps=a.steps, order=a.order, repeats=a.repeats, in_library_loop=in_library,
               device=torch.cuda.get_device_name(0), checksum=float(first["plms_sample_loop"].double().abs().sum()))
    for k, v in ms.items():
        rec[k + "_ms_per_step"] = round(statistics.median(v), 5)
        rec[k + "_ms_per_step_min_max"] = [round(min(v), 5), round(max(v), 5)]
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
