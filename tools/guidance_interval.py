#!/usr/bin/env python3
"""ms/step of the fused sampling loops under a guidance interval (y['guidance_interval']), by guided fraction of the steps:
    python tools/guidance_interval.py [--config genea|2] [--dtype fp32|fp16] [--sampler p|dpmpp] [--fractions 0,0.25,0.5,1]
                                      [--repeats 3] [--references] [--baseline] [--tree DIR] [--out profiles/FILE.txt]
A fraction f guides round(f * steps) consecutive steps in the middle of the schedule (the interval is read off the timestep
map), 0 is the empty interval.  --references adds the two loops the ends are compared with: the guided model without the key
("nokey") and the inner model without guidance ("inner").  --baseline times ONLY those two and touches nothing a tree without the
feature lacks; with --tree DIR the package (and its library) are taken from that checkout -- the parent commit's, whose library
this package cannot load because it lacks the two new exports -- so both sides run in one job on one box, alternating processes.
`p` runs the full 1000-step schedule with in-kernel Philox noise, `dpmpp` order 2 on logsnr20 (the record says how many steps it
keeps; the 20-step loop is run `inner` times per timed window).  Every process first warms both batch shapes (a guided and an
unguided short loop), then times each row `repeats` times between two events on the stream, rows alternating inside each
repeat; median and min / max per step.  One JSON line per run.  GDX_TM_MIRROR=always (read once per process by the library)
makes every unguided step of a partly guided call mirror the token-major state: the A/B of DESIGN.md 4f."""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def timed(torch, fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    r = fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop), r


def interval_for(tmap, fraction):
    """(lo, hi) guiding round(fraction * n) consecutive steps in the middle of the ascending timestep map; (1, 0) for none."""
    n = len(tmap)
    G = int(round(fraction * n))
    if G <= 0:
        return (1, 0), 0
    first = (n - G) // 2
    return (int(tmap[first]), int(tmap[first + G - 1])), G


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="genea", choices=["2", "genea"])
    ap.add_argument("--dtype", default="fp32", choices=["fp32", "fp16"])
    ap.add_argument("--sampler", default="p", choices=["p", "dpmpp"])
    ap.add_argument("--fractions", default="0,0.25,0.5,1")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--references", action="store_true", help="also time the guided loop without the key and the inner model")
    ap.add_argument("--baseline", action="store_true", help="time only those two (runs on a tree without the feature)")
    ap.add_argument("--tree", default=os.path.join(HERE, ".."), help="checkout whose package and library are measured")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    sys.path.insert(1, os.path.join(HERE, ".."))                # bench.py (presets, model builder) is this checkout's
    import torch
    from gesturediffusion_amd import _lib                       # the measured tree's package first: bench.py imports lazily
    from gesturediffusion_amd.diffusion import gaussian_diffusion as gd
    from gesturediffusion_amd.diffusion.respace import SpacedDiffusion, space_timesteps
    from gesturediffusion_amd.model import mdm_old  # noqa: F401
    from gesturediffusion_amd.model.cfg_sampler import ClassifierFreeSampleModel
    from gesturediffusion_amd.utils.init import synthetic_inputs
    from bench import PRESETS, build_model
    assert os.path.abspath(_lib.__file__).startswith(os.path.abspath(a.tree) + os.sep), _lib.__file__
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    p = PRESETS[a.config]
    dev = torch.device("cuda:0")
    model, cfg, _ = build_model(p["arch"], p["J"], p["d"], p["L"], dev)
    model.compute_dtype = a.dtype
    B, T, J = p["batch"], p["T"], p["J"]
    betas = gd.get_named_beta_schedule("cosine", 1000)
    respacing = [1000] if a.sampler == "p" else "logsnr20"
    use = space_timesteps(1000, respacing, betas=betas) if a.sampler == "dpmpp" else space_timesteps(1000, respacing)
    df = SpacedDiffusion(use_timesteps=use, betas=betas, model_mean_type=gd.ModelMeanType.START_X,
                         model_var_type=gd.ModelVarType.FIXED_SMALL, loss_type=gd.LossType.MSE)
    steps = df.num_timesteps
    inner = 1 if a.sampler == "p" else 10                       # loops per timed window
    x, seedp, mfcc = synthetic_inputs(cfg, B, T, seed=10)
    x = x.to(dev)
    y_in = {"seed": seedp.to(dev), "mfcc": mfcc.to(dev)}
    y_cfg = dict(y_in, scale=torch.full((B,), 2.5, device=dev))
    guided = ClassifierFreeSampleModel(model)

    def loop(m, y, **kw):
        kw = dict(kw, noise=x, clip_denoised=False, model_kwargs={"y": y})
        if a.sampler == "p":
            return df.p_sample_loop(m, (B, J, 1, T), rng="philox", philox_seed=10, **kw)
        return df.dpm_solver_sample_loop(m, (B, J, 1, T), order=2, **kw)

    rows, guided_steps = {}, {}
    if not a.baseline:
        for f in (float(v) for v in a.fractions.split(",")):
            iv, G = interval_for(df.timestep_map, f)
            assert sum(df.guided_steps(iv)) == G
            rows[f"f{f:g}"] = lambda iv=iv: loop(guided, dict(y_cfg, guidance_interval=iv))
            guided_steps[f"f{f:g}"] = G
    if a.baseline or a.references:
        rows["nokey"] = lambda: loop(guided, y_cfg)
        rows["inner"] = lambda: loop(model, y_in)
    short = dict(skip_timesteps=max(0, steps - 40))
    loop(guided, y_cfg, **short)                                # warm-up: both batch shapes at the timed size
    loop(model, y_in, **short)
    torch.cuda.synchronize()
    ms = {k: [] for k in rows}
    for _ in range(a.repeats):
        for k, fn in rows.items():                              # alternate the rows inside each repeat
            t, r = timed(torch, lambda fn=fn: [fn() for _ in range(inner)][-1])
            assert torch.isfinite(r).all(), k
            ms[k].append(t / (steps * inner))
    own = os.path.abspath(a.tree) == os.path.abspath(os.path.join(HERE, ".."))
    rec = dict(tool="guidance_interval", tree="this checkout" if own else os.path.basename(os.path.abspath(a.tree)),
               config=a.config, label=p["label"], arch=p["arch"], B=B, T=T, J=J, d=p["d"], dtype=a.dtype, scale=2.5,
               sampler=a.sampler, steps=steps, loops_per_window=inner, repeats=a.repeats,
               tm_mirror=os.environ.get("GDX_TM_MIRROR", "next-guided"), device=torch.cuda.get_device_name(0))
    for k, v in ms.items():
        rec[k] = dict(ms_per_step=round(statistics.median(v), 5), min_max=[round(min(v), 5), round(max(v), 5)])
        if k in guided_steps:
            rec[k]["guided_steps"] = guided_steps[k]
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
