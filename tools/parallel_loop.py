#!/usr/bin/env python3
"""Wall time of a whole sampling loop run parallel in time (parallel_sample_loop) against the sequential p_sample_loop:
    python tools/parallel_loop.py [--config 1|genea] [--batch N] [--windows 8 16 32 64] [--tols 0 1e-3 1e-2 1e-1] [--steps N]
                                  [--repeats 2] [--baseline] [--tree DIR] [--out profiles/FILE.txt]
Rows: "sequential" = p_sample_loop with in-kernel Philox noise (today's loop: gdx_sample_loop), "wWtT" = parallel_sample_loop at
window W and tolerance T under the same x_T and the same Philox step noise.  Per row: the wall time of the whole loop in ms (host
clock around a synchronised loop: the parallel loop synchronises once per iteration, which is part of its cost), its iterations,
the samples it pushed through the denoiser, and the final sample's max-abs deviation from the sequential sample relative to
max|sequential|.  --baseline times ONLY "sequential" and touches nothing a tree without the feature lacks; with --tree DIR the
package (and its library) are taken from that checkout -- the parent commit's -- so both sides run in one job on one box,
alternating processes.  The schedule is the full 1000 steps (--steps N: only its last N, from a q_sample'd zero image); the GENEA
chunk runs guided at scale 2.5, config 1 unguided, --batch overrides the preset's batch.  Every row is warmed on a 20-step loop at
its own shape (the workspace of window x batch samples is allocated there), then timed `repeats` times; median and min / max.
One JSON line per run.  Weights are random: nothing about motion quality on a trained checkpoint follows."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="genea", choices=["1", "genea"])
    ap.add_argument("--batch", type=int, default=0, help="samples (0 = the preset's)")
    ap.add_argument("--windows", type=int, nargs="+", default=[8, 16, 32, 64])
    ap.add_argument("--tols", type=float, nargs="+", default=[0.0, 1e-3, 1e-2, 1e-1])
    ap.add_argument("--steps", type=int, default=0, help="only the last N steps of the schedule (0 = all 1000)")
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--baseline", action="store_true", help="time only the sequential loop (runs on a tree without the feature)")
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
    B, T, J = a.batch or p["batch"], p["T"], p["J"]
    df = SpacedDiffusion(use_timesteps=space_timesteps(1000, [1000]), betas=gd.get_named_beta_schedule("cosine", 1000),
                         model_mean_type=gd.ModelMeanType.START_X, model_var_type=gd.ModelVarType.FIXED_SMALL,
                         loss_type=gd.LossType.MSE)
    n = df.num_timesteps
    steps = min(n, a.steps) if a.steps > 0 else n
    x, seedp, mfcc = synthetic_inputs(cfg, B, T, seed=10)
    x = x.to(dev)
    y = {"seed": seedp.to(dev), "mfcc": mfcc.to(dev)}
    guided = a.config == "genea"
    if guided:
        y["scale"] = torch.full((B,), 2.5, device=dev)
        model = ClassifierFreeSampleModel(model)
    kw = dict(noise=x, clip_denoised=False, model_kwargs={"y": y}, philox_seed=10)

    def sequential(skip):
        return df.p_sample_loop(model, (B, J, 1, T), skip_timesteps=skip, rng="philox", **kw)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def stats(v):
        return dict(ms=round(statistics.median(v), 2), min_max=[round(min(v), 2), round(max(v), 2)])

    own = os.path.abspath(a.tree) == os.path.abspath(os.path.join(HERE, ".."))
    rec = dict(tool="parallel_loop", tree="this checkout" if own else "parent", config=a.config, label=p["label"], arch=p["arch"], B=B,
               T=T, J=J, d=p["d"], L=p["L"], dtype="fp32", scale=2.5 if guided else None, sampler="p", steps=steps, repeats=a.repeats,
               device=torch.cuda.get_device_name(0))
    sequential(max(0, n - 20))
    ms, want = [], None
    for _ in range(a.repeats):
        t, want = wall(lambda: sequential(n - steps))
        ms.append(t)
    assert torch.isfinite(want).all()
    rec["sequential"] = dict(stats(ms), iterations=steps, forward_samples=steps * B * (2 if guided else 1))
    top = float(want.abs().max())
    if not a.baseline:
        for W in a.windows:
            try:                                                # warm-up; a window x batch the library cannot run is recorded as that
                df.parallel_sample_loop(model, (B, J, 1, T), skip_timesteps=max(0, n - 20), window=W, tolerance=0.1, **kw)
            except _lib.GdxError as e:
                rec[f"w{W}"] = dict(refused=str(e))
                continue
            for tol in a.tols:
                ms, rep, r = [], {}, None
                for _ in range(a.repeats):
                    t, r = wall(lambda: df.parallel_sample_loop(model, (B, J, 1, T), skip_timesteps=n - steps, window=W, tolerance=tol,
                                                                report=rep, **kw))
                    ms.append(t)
                row = dict(stats(ms), iterations=rep["iterations"], forward_samples=rep["forward_samples"],
                           deviation=float(f"{float((r - want).abs().max()) / top:.3e}"),
                           ratio_to_sequential=round(statistics.median(ms) / rec["sequential"]["ms"], 3))
                assert sum(rep["strides"]) == steps
                rec[f"w{W}t{tol:g}"] = row
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
