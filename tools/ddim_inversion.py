#!/usr/bin/env python3
"""ms/step of the fused DDIM inversion (ddim_reverse_sample_loop) beside the ddim_sample_loop step, and the round-trip error:
    python tools/ddim_inversion.py [--config genea|2] [--dtype fp32|fp16] [--respacing ddim50] [--repeats 5] [--baseline]
                                   [--tree DIR] [--round_trip] [--out profiles/FILE.txt]
Timing.  Rows: "ddim_sample" = ddim_sample_loop at eta 0 over all steps of the respacing (x_T given, so nothing is drawn but the
step noise of weight 0), "inversion" = ddim_reverse_sample_loop over all of them (until = num_timesteps).  Both run the SAME model
on the conditional pass alone -- what --invert_gt inverts with -- so a step of either is one forward of B samples and one update
launch; the sampling loop takes gdx_sample_loop's token-major path (no transposes between steps), the inversion the pose-layout
path of the multistep loops (two transposes per step).  --baseline times ONLY "ddim_sample" and touches nothing a tree without the
feature lacks; with --tree DIR the package (and its library) are taken from that checkout -- the parent commit's -- so both sides
run in one job on one box, alternating processes.  Every process first warms each row once at the timed size, then times each row
`repeats` times between two events on the stream, rows alternating inside each repeat, `inner` loops per timed window; median and
min / max per step.  One JSON line per run.
--round_trip (instead of timing): x (the config's synthetic N(0,1) poses standing in for recorded motion) is inverted to
until = num_timesteps - 1 and re-generated with ddim_sample_loop(noise=latent) on ddim10 / 20 / 50 / 100, clip_denoised=False;
max|regenerated - x| / max|x| and max|latent|.  Random weights: nothing about motion quality on a trained checkpoint follows."""
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
    ap.add_argument("--config", default="genea", choices=["2", "genea"])
    ap.add_argument("--dtype", default="fp32", choices=["fp32", "fp16"])
    ap.add_argument("--respacing", default="ddim50")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=2, help="loops per timed window")
    ap.add_argument("--baseline", action="store_true", help="time only ddim_sample_loop (runs on a tree without the feature)")
    ap.add_argument("--tree", default=os.path.join(HERE, ".."), help="checkout whose package and library are measured")
    ap.add_argument("--round_trip", action="store_true", help="round-trip error instead of timing")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    sys.path.insert(1, os.path.join(HERE, ".."))                # bench.py (presets, model builder) is this checkout's
    import torch
    from gesturediffusion_amd import _lib                       # the measured tree's package first: bench.py imports lazily
    from gesturediffusion_amd.diffusion import gaussian_diffusion as gd
    from gesturediffusion_amd.diffusion.respace import SpacedDiffusion, space_timesteps
    from gesturediffusion_amd.model import mdm_old  # noqa: F401
    from gesturediffusion_amd.utils.init import synthetic_inputs
    from bench import PRESETS, build_model
    assert os.path.abspath(_lib.__file__).startswith(os.path.abspath(a.tree) + os.sep), _lib.__file__
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    p = PRESETS[a.config]
    dev = torch.device("cuda:0")
    model, cfg, _ = build_model(p["arch"], p["J"], p["d"], p["L"], dev)
    model.compute_dtype = a.dtype
    B, T, J = p["batch"], p["T"], p["J"]
    shape = (B, J, 1, T)

    def diffusion(respacing):
        return SpacedDiffusion(use_timesteps=space_timesteps(1000, respacing), betas=gd.get_named_beta_schedule("cosine", 1000),
                               model_mean_type=gd.ModelMeanType.START_X, model_var_type=gd.ModelVarType.FIXED_SMALL,
                               loss_type=gd.LossType.MSE)

    x, seedp, mfcc = synthetic_inputs(cfg, B, T, seed=10)
    x = x.to(dev)
    kw = dict(clip_denoised=False, model_kwargs={"y": {"seed": seedp.to(dev), "mfcc": mfcc.to(dev)}})
    own = os.path.abspath(a.tree) == os.path.abspath(os.path.join(HERE, ".."))
    rec = dict(tool="ddim_inversion", tree="this checkout" if own else "parent", config=a.config, label=p["label"], arch=p["arch"],
               B=B, T=T, J=J, d=p["d"], dtype=a.dtype, guidance="none (conditional pass)", device=torch.cuda.get_device_name(0))

    if a.round_trip:
        rec["measure"] = "max|regenerated - x| / max|x| after inversion to until = n - 1 and ddim_sample_loop(noise=latent), random weights"
        top = float(x.abs().max())
        for respacing in ("ddim10", "ddim20", "ddim50", "ddim100"):
            df = diffusion(respacing)
            latent = df.ddim_reverse_sample_loop(model, x, **kw)
            back = df.ddim_sample_loop(model, shape, noise=latent, eta=0.0, **kw)
            assert torch.isfinite(latent).all() and torch.isfinite(back).all(), respacing
            rec[respacing] = dict(round_trip=float(f"{float((back - x).abs().max()) / top:.3e}"),
                                  max_abs_latent=float(f"{float(latent.abs().max()):.3e}"))
    else:
        df = diffusion(a.respacing)
        n = df.num_timesteps
        rows = {"ddim_sample": lambda: df.ddim_sample_loop(model, shape, noise=x, eta=0.0, **kw)}
        if not a.baseline:
            rows["inversion"] = lambda: df.ddim_reverse_sample_loop(model, x, until=n, **kw)
        for fn in rows.values():                                # warm-up: every row's kernels at the timed size
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in rows}
        for _ in range(a.repeats):
            for k, fn in rows.items():                          # alternate the rows inside each repeat
                t, r = timed(torch, lambda fn=fn: [fn() for _ in range(a.inner)][-1])
                assert torch.isfinite(r).all(), k
                ms[k].append(t / (n * a.inner))
        rec.update(respacing=a.respacing, steps=n, loops_per_window=a.inner, repeats=a.repeats)
        for k, v in ms.items():
            rec[k] = dict(ms_per_step=round(statistics.median(v), 5), min_max=[round(min(v), 5), round(max(v), 5)])
        if not a.baseline:
            rec["inversion"]["ratio_to_ddim_sample"] = round(rec["inversion"]["ms_per_step"] / rec["ddim_sample"]["ms_per_step"], 4)
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
