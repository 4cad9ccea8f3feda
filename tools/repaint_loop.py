#!/usr/bin/env python3
"""Wall time of one chunk's resampled loop (repaint_sample_loop) against its denoiser-call count, and the forward hop's share:
    python tools/repaint_loop.py [--config 1|genea] [--batch N] [--pairs 1,1 10,5 10,10] [--respacing 50] [--sampler p]
                                 [--repeats 3] [--out profiles/FILE.txt]
Rows: "jJrR" = repaint_sample_loop(jump=J, repeats=R) with in-kernel Philox noise on an in-betweening mask (the middle half of the
frames is generated); "j1r1" is the plain loop (repeats = 1 runs p_sample_loop / ddim_sample_loop itself).  Per row: the wall time of
the whole loop in ms (host clock around a synchronised loop; median and min / max of `repeats` runs after one warm run), its hops and
denoiser calls, ms per denoiser call, and its ratio to the plain loop next to the ratio of the call counts.  "forward_hop_us": the
forward hop alone, timed as a block of gdx_sample_loop that holds nothing else -- the hops of a (N - 1, 2) walk are N descents, one
forward hop, N - 1 descents, so a block of one hop at k_base = N is the renoise kernel -- over 200 such calls between two
synchronisations, and as a share of the row's ms per call.  The GENEA chunk runs guided at scale 2.5, config 1 unguided.  One JSON
line per run.  Weights are random: nothing about motion quality on a trained checkpoint follows."""
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
    ap.add_argument("--pairs", nargs="+", default=["1,1", "10,5", "10,10"], help="JUMP,REPEATS per row")
    ap.add_argument("--respacing", default="50", help="timestep respacing of the 1000-step cosine schedule")
    ap.add_argument("--sampler", default="p", choices=["p", "ddim"])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(HERE, ".."))
    import torch
    from gesturediffusion_amd._lib import GDX_SAMPLER_DDIM, GDX_SAMPLER_P
    from gesturediffusion_amd.diffusion import gaussian_diffusion as gd
    from gesturediffusion_amd.diffusion.respace import SpacedDiffusion, space_timesteps
    from gesturediffusion_amd.model import mdm_old  # noqa: F401
    from gesturediffusion_amd.model.cfg_sampler import ClassifierFreeSampleModel
    from gesturediffusion_amd.utils.init import synthetic_inputs
    from bench import PRESETS, build_model
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    p = PRESETS[a.config]
    dev = torch.device("cuda:0")
    model, cfg, _ = build_model(p["arch"], p["J"], p["d"], p["L"], dev)
    B, T, J = a.batch or p["batch"], p["T"], p["J"]
    df = SpacedDiffusion(use_timesteps=space_timesteps(1000, a.respacing), betas=gd.get_named_beta_schedule("cosine", 1000),
                         model_mean_type=gd.ModelMeanType.START_X, model_var_type=gd.ModelVarType.FIXED_SMALL,
                         loss_type=gd.LossType.MSE)
    n = df.num_timesteps
    x, seedp, mfcc = synthetic_inputs(cfg, B, T, seed=10)
    x = x.to(dev)
    mask = torch.ones(B, J, 1, T, dtype=torch.bool, device=dev)
    mask[..., T // 4:3 * T // 4] = False
    y = {"seed": seedp.to(dev), "mfcc": mfcc.to(dev), "inpainting_mask": mask, "inpainted_motion": torch.randn_like(x)}
    guided = a.config == "genea"
    if guided:
        y["scale"] = torch.full((B,), 2.5, device=dev)
        model = ClassifierFreeSampleModel(model)
    kw = dict(noise=x, clip_denoised=False, model_kwargs={"y": y}, rng="philox", philox_seed=10, sampler=a.sampler)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    rec = dict(tool="repaint_loop", config=a.config, label=p["label"], arch=p["arch"], B=B, T=T, J=J, d=p["d"], L=p["L"], dtype="fp32",
               scale=2.5 if guided else None, sampler=a.sampler, steps=n, repeats=a.repeats, device=torch.cuda.get_device_name(0))
    rows = {}
    for pair in a.pairs:
        jump, reps = (int(v) for v in pair.split(","))
        plan = df.resample_plan(jump, reps)
        calls = sum(h[0] == "r" for h in plan)
        run = lambda: df.repaint_sample_loop(model, (B, J, 1, T), jump=jump, repeats=reps, **kw)   # noqa: E731
        run()
        ms = []
        for _ in range(a.repeats):
            t, r = wall(run)
            ms.append(t)
        assert torch.isfinite(r).all()
        med = statistics.median(ms)
        rows[f"j{jump}r{reps}"] = dict(ms=round(med, 2), min_max=[round(min(ms), 2), round(max(ms), 2)], hops=len(plan), calls=calls,
                                       ms_per_call=round(med / calls, 4))
    plain = rows.get("j1r1")
    for row in rows.values():
        if plain is not None:
            row["ratio_to_plain"] = round(row["ms"] / plain["ms"], 3)
            row["calls_ratio"] = round(row["calls"] / plain["calls"], 3)
    rec.update(rows)
    # the forward hop alone: hop number n of a (n - 1, 2) walk, issued as a block of one hop
    state = x.clone()
    eng, mode, scale, m, motion = df._native_loop_setup(model, state, {"y": y})
    kind = GDX_SAMPLER_P if a.sampler == "p" else GDX_SAMPLER_DDIM
    coef, tmap = df.coef_table(kind, dev), df._timestep_map()
    assert df.resample_plan(n - 1, 2)[n] == ("f", 0, n - 1)
    eng.set_resample(n - 1, 2, df.alphas_cumprod)
    try:
        hop = lambda: eng.sample_loop(state, kind, mode, coef, tmap, n - 1, scale=scale, inpaint_mask=m, inpaint_motion=motion,   # noqa: E731
                                      philox_seed=10, run_steps=1, k_base=n)
        hop()
        t, _ = wall(lambda: [hop() for _ in range(200)])
    finally:
        eng.set_resample(1, 1)
    rec["forward_hop_us"] = round(t * 1e3 / 200, 2)
    for row in rows.values():
        row["forward_hop_share_of_a_call"] = round(rec["forward_hop_us"] * 1e-3 / row["ms_per_call"], 4)
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
