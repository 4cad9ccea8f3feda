#!/usr/bin/env python3
"""ms/step of dpm_solver_sample_loop (orders 1 to 3) next to ddim_sample_loop and plms_sample_loop (order 2) on the same
respacing, in one process:
    python tools/dpm_loop.py [--config genea|2|1] [--dtype fp32|fp16|bf16] [--respacing logsnr20] [--repeats 5]
                             [--sde | --unipc] [--out profiles/FILE.txt]
--sde measures dpm_solver_sde_sample_loop (orders 1 and 2, eta = 1, in-kernel Philox noise) next to dpm_solver_sample_loop at
order 2 and p_sample_loop (Philox) on the same respacing instead; the expectation is one Philox draw per element on top of the
ODE step.
--unipc measures unipc_sample_loop (orders 1 to 3) next to dpm_solver_sample_loop at the same order instead and records the
ratio per order; the expectation is the same forward plus one launch that reads up to one history tensor more and writes the
corrected state as well (the forward dominates; the ratio is recorded, not gated).
Every loop runs once as a warm-up at the timed shape, then `repeats` times between two events on the stream, the loops
alternating inside each repeat; the median is reported with the spread, per step of the respacing ("logsnrN" can keep fewer
than N steps: the record says how many; PLMS runs one forward more than it has steps).  One JSON line per run; kernel-level
numbers come from running this under `rocprofv3 --kernel-trace --stats` in a run of its own.  There is no threshold: the DPM
step is the same forward plus one launch in the pose layout, the DDIM loop keeps its state token-major."""
import argparse
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
    ap.add_argument("--config", default="genea", choices=["1", "2", "genea"])
    ap.add_argument("--dtype", default=None, choices=["fp32", "fp16", "bf16"])
    ap.add_argument("--respacing", default="logsnr20")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sde", action="store_true", help="time the stochastic loop against the ODE loop and p_sample_loop")
    ap.add_argument("--unipc", action="store_true", help="time unipc_sample_loop against dpm_solver_sample_loop, order by order")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    p = PRESETS[a.config]
    dtype = a.dtype or p["dtype"]
    dev = torch.device("cuda:0")
    model, cfg, _ = build_model(p["arch"], p["J"], p["d"], p["L"], dev)
    model.compute_dtype = dtype
    B, T, J = p["batch"], p["T"], p["J"]
    betas = gd.get_named_beta_schedule("cosine", 1000)
    df = SpacedDiffusion(use_timesteps=space_timesteps(1000, a.respacing, betas=betas), betas=betas,
                         model_mean_type=gd.ModelMeanType.START_X, model_var_type=gd.ModelVarType.FIXED_SMALL,
                         loss_type=gd.LossType.MSE)
    steps = df.num_timesteps
    x, seedp, mfcc = synthetic_inputs(cfg, B, T, seed=10)
    x = x.to(dev)
    y = {"seed": seedp.to(dev), "mfcc": mfcc.to(dev)}
    m = model
    if p["cfg"]:
        y["scale"] = torch.full((B,), 2.5, device=dev)
        m = ClassifierFreeSampleModel(model)
    kw = dict(noise=x, clip_denoised=False, model_kwargs={"y": y})
    assert not (a.sde and a.unipc), "--sde and --unipc are two measurements"
    if a.unipc:
        loops = {}
        for o in (1, 2, 3):                                                    # neighbours in the alternation: same order
            loops[f"dpm_order{o}"] = lambda o=o: df.dpm_solver_sample_loop(m, (B, J, 1, T), order=o, **kw)
            loops[f"unipc_order{o}"] = lambda o=o: df.unipc_sample_loop(m, (B, J, 1, T), order=o, **kw)
    elif a.sde:
        loops = {f"dpm_sde_order{o}": (lambda o=o: df.dpm_solver_sde_sample_loop(m, (B, J, 1, T), order=o, eta=1.0, rng="philox",
                                                                                 philox_seed=10, **kw)) for o in (1, 2)}
        loops["dpm_order2"] = lambda: df.dpm_solver_sample_loop(m, (B, J, 1, T), order=2, **kw)
        loops["p_sample"] = lambda: df.p_sample_loop(m, (B, J, 1, T), rng="philox", philox_seed=10, **kw)
    else:
        loops = {f"dpm_order{o}": (lambda o=o: df.dpm_solver_sample_loop(m, (B, J, 1, T), order=o, **kw)) for o in (1, 2, 3)}
        loops["ddim"] = lambda: df.ddim_sample_loop(m, (B, J, 1, T), eta=0.0, rng="philox", **kw)
        loops["plms_order2"] = lambda: df.plms_sample_loop(m, (B, J, 1, T), order=2, **kw)
    first = {k: timed(fn)[1] for k, fn in loops.items()}                       # warm-up at the timed shape
    ms = {k: [] for k in loops}
    for _ in range(a.repeats):
        for k, fn in loops.items():                                            # alternate the loops inside each repeat
            t, r = timed(fn)
            assert torch.equal(r, first[k]) and torch.isfinite(r).all(), k
            ms[k].append(t / steps)
    rec = dict(tool="dpm_loop", config=a.config, label=p["label"], arch=p["arch"], B=B, T=T, J=J, d=p["d"], dtype=dtype,
               guidance=bool(p["cfg"]), respacing=a.respacing, steps=steps, repeats=a.repeats,
               device=torch.cuda.get_device_name(0))
    if a.unipc:
        rec["unipc"] = True
    elif a.sde:
        rec["sde"] = True
    else:
        ref = first["ddim"].double()
        rec["order1_vs_ddim_rel"] = float((first["dpm_order1"].double() - ref).abs().max() / ref.abs().max())
    for k, v in ms.items():
        rec[k + "_ms_per_step"] = round(statistics.median(v), 5)
        rec[k + "_ms_per_step_min_max"] = [round(min(v), 5), round(max(v), 5)]
    if a.unipc:
        for o in (1, 2, 3):
            med = {w: statistics.median(ms[f"{w}_order{o}"]) for w in ("unipc", "dpm")}
            rec[f"unipc_over_dpm_order{o}"] = round(med["unipc"] / med["dpm"], 4)
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
