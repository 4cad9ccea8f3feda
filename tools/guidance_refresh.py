#!/usr/bin/env python3
"""ms/step of the fused sampling loops under the guidance refresh (y['guidance_refresh']), and how far its result moves:
    python tools/guidance_refresh.py [--config genea|3] [--dtype fp32|fp16] [--sampler p|dpmpp] [--every 2 4] [--steps N]
                                     [--repeats 3] [--baseline] [--tree DIR] [--deviation] [--out profiles/FILE.txt]
Rows: "nokey" = the guided model without the key (today's loop), "every1" = the key at 1 (the same launches), "everyK" = the
unconditional pass on every K-th guided call.  --baseline times ONLY "nokey" and touches nothing a tree without the feature
lacks; with --tree DIR the package (and its library) are taken from that checkout -- the parent commit's, whose library this
package cannot load through GDX_LIBGDX because it lacks the two new exports -- so both sides run in one job on one box,
alternating processes; repeating the parent's process gives the run-to-run spread the every = 1 path is held against.
`p` runs the 1000-step schedule with in-kernel Philox noise (--steps N: only its last N steps, for the large shapes): without the
key it takes gdx_sample_loop's token-major path, with every > 1 the pose-layout path, so the time holds the skipped passes, the
delta pass AND two transposes per step.  `dpmpp` (order 2 on logsnr20, the loop run `inner` times per timed window) is
pose-layout either way.  Every process first warms a short loop per row, then times each row `repeats` times between two events
on the stream, rows alternating inside each repeat; median and min / max per step, and the sample-count prediction
(1 + 1/K) / 2 of the every = 1 time beside each measured ratio.  One JSON line per run.
--deviation (instead of timing): the ancestral loop on ddim10 and ddim50 with a recorded x_T and Philox step noise; the final
sample's max-abs deviation from the fully guided loop relative to max|guided|, for every K and for the unguided loop (the whole
effect of guidance).  Random weights: nothing about motion quality on a trained checkpoint follows from it."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="genea", choices=["3", "genea"])
    ap.add_argument("--dtype", default="fp32", choices=["fp32", "fp16"])
    ap.add_argument("--sampler", default="p", choices=["p", "dpmpp"])
    ap.add_argument("--every", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--steps", type=int, default=0, help="--sampler p: time only the last N steps of the schedule (0 = all 1000)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--baseline", action="store_true", help="time only the loop without the key (runs on a tree without the feature)")
    ap.add_argument("--tree", default=os.path.join(HERE, ".."), help="checkout whose package and library are measured")
    ap.add_argument("--deviation", action="store_true", help="deviation from the fully guided loop instead of timing")
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

    def diffusion(respacing):
        use = space_timesteps(1000, respacing, betas=betas) if respacing == "logsnr20" else space_timesteps(1000, respacing)
        return SpacedDiffusion(use_timesteps=use, betas=betas, model_mean_type=gd.ModelMeanType.START_X,
                               model_var_type=gd.ModelVarType.FIXED_SMALL, loss_type=gd.LossType.MSE)

    x, seedp, mfcc = synthetic_inputs(cfg, B, T, seed=10)
    x = x.to(dev)
    y_in = {"seed": seedp.to(dev), "mfcc": mfcc.to(dev)}
    y_cfg = dict(y_in, scale=torch.full((B,), 2.5, device=dev))
    guided = ClassifierFreeSampleModel(model)
    own = os.path.abspath(a.tree) == os.path.abspath(os.path.join(HERE, ".."))
    rec = dict(tool="guidance_refresh", tree="this checkout" if own else "parent", config=a.config, label=p["label"], arch=p["arch"],
               B=B, T=T, J=J, d=p["d"], dtype=a.dtype, scale=2.5, device=torch.cuda.get_device_name(0))

    if a.deviation:
        rec["measure"] = "max|x - guided| / max|guided| of the final sample, ancestral loop, random weights"
        for respacing in ("ddim10", "ddim50"):
            df = diffusion(respacing)
            kw = dict(noise=x, clip_denoised=False, rng="philox", philox_seed=10)
            full = df.p_sample_loop(guided, (B, J, 1, T), model_kwargs={"y": y_cfg}, **kw)
            top = float(full.abs().max())
            row = {}
            for k in a.every:
                r = df.p_sample_loop(guided, (B, J, 1, T), model_kwargs={"y": dict(y_cfg, guidance_refresh=k)}, **kw)
                assert torch.isfinite(r).all(), k
                row[f"every{k}"] = float(f"{float((r - full).abs().max()) / top:.3e}")
            r = df.p_sample_loop(model, (B, J, 1, T), model_kwargs={"y": y_in}, **kw)
            row["unguided"] = float(f"{float((r - full).abs().max()) / top:.3e}")
            rec[respacing] = row
    else:
        respacing = [1000] if a.sampler == "p" else "logsnr20"
        df = diffusion(respacing)
        n = df.num_timesteps
        steps = min(n, a.steps) if a.sampler == "p" and a.steps > 0 else n
        inner = 1 if a.sampler == "p" else 10                   # loops per timed window

        def loop(y, skip):
            kw = dict(noise=x, clip_denoised=False, model_kwargs={"y": y}, skip_timesteps=skip)
            if a.sampler == "p":
                return df.p_sample_loop(guided, (B, J, 1, T), rng="philox", philox_seed=10, **kw)
            return df.dpm_solver_sample_loop(guided, (B, J, 1, T), order=2, **kw)

        rows = {"nokey": y_cfg}
        if not a.baseline:
            rows["every1"] = dict(y_cfg, guidance_refresh=1)
            for k in a.every:
                rows[f"every{k}"] = dict(y_cfg, guidance_refresh=k)
        for y in rows.values():                                 # warm-up: every row's kernels at the timed size
            loop(y, max(0, n - 20))
        torch.cuda.synchronize()
        ms = {k: [] for k in rows}
        for _ in range(a.repeats):
            for k, y in rows.items():                           # alternate the rows inside each repeat
                t, r = timed(torch, lambda y=y: [loop(y, n - steps) for _ in range(inner)][-1])
                assert torch.isfinite(r).all(), k
                ms[k].append(t / (steps * inner))
        rec.update(sampler=a.sampler, steps=steps, loops_per_window=inner, repeats=a.repeats)
        for k, v in ms.items():
            rec[k] = dict(ms_per_step=round(statistics.median(v), 5), min_max=[round(min(v), 5), round(max(v), 5)])
        if not a.baseline:
            base = rec["every1"]["ms_per_step"]
            for k in a.every:
                rec[f"every{k}"].update(ratio_to_every1=round(rec[f"every{k}"]["ms_per_step"] / base, 4),
                                        sample_count_prediction=round((1 + 1 / k) / 2, 4))
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
