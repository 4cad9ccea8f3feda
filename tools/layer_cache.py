#!/usr/bin/env python3
"""ms/step of the fused ancestral loop under the layer cache (y['layer_cache']), and how far its result moves:
    python tools/layer_cache.py [--config genea|3] [--dtype fp32|fp16] [--cache 2,2 2,4 4,2] [--steps N] [--repeats 3]
                                [--baseline] [--tree DIR] [--deviation] [--out profiles/FILE.txt]
Rows: "nokey" = the guided model without the key (today's loop), "off" = the key at (1, 0) (the same launches), "eEkK" = every
E-th denoiser call in full, K layers on the calls in between.  --baseline times ONLY "nokey" and touches nothing a tree without
the feature lacks; with --tree DIR the package (and its library) are taken from that checkout -- the parent commit's, whose
library this package cannot load through GDX_LIBGDX because it lacks the new exports -- so both sides run in one job on one
box, alternating processes; repeating the parent's process gives the run-to-run spread the off path is held against.
The loop is p_sample_loop on the 1000-step schedule with in-kernel Philox noise (--steps N: only its last N steps, for the large
shapes), guided at scale 2.5: gdx_sample_loop's token-major path with and without the key.  Every process first warms a short
loop per row, then times each row `repeats` times between two events on the stream, rows alternating inside each repeat; median
and min / max per step.  Beside each measured ratio to "off" stands the prediction share * (1 + (E-1) K/L) / E + (1 - share),
share = the encoder's part of the step, itself measured in the same process from two loops that differ only in their layers:
share = 1 - t(E = 10^6, K = 1 extrapolated to K = 0) / t(off), i.e. from t(K = 1) and t(K = 2) of a loop whose calls after the
first are all partial.  Full calls pay the store pass, partial calls the apply pass; neither is in the prediction.
One JSON line per run.
--deviation (instead of timing): the ancestral loop on ddim10, ddim50 and the full 1000-step schedule (--steps ignored) with a
recorded x_T and Philox step noise; the final sample's max-abs deviation from the uncached loop relative to max|uncached|, for
every (E, K), beside "dropped": the distance of a model WITHOUT the deep layers (the same weights, layers K .. L-1 removed) --
what ignoring those layers altogether would cost.  Random weights: nothing about motion quality on a trained checkpoint follows."""
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


def pair(text):
    e, k = text.split(",")
    return int(e), int(k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="genea", choices=["3", "genea"])
    ap.add_argument("--dtype", default="fp32", choices=["fp32", "fp16"])
    ap.add_argument("--cache", type=pair, nargs="+", default=[(2, 2), (2, 4), (4, 2)], metavar="E,K")
    ap.add_argument("--steps", type=int, default=0, help="time only the last N steps of the schedule (0 = all 1000)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--baseline", action="store_true", help="time only the loop without the key (runs on a tree without the feature)")
    ap.add_argument("--tree", default=os.path.join(HERE, ".."), help="checkout whose package and library are measured")
    ap.add_argument("--deviation", action="store_true", help="deviation from the uncached loop instead of timing")
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
    B, T, J, L = p["batch"], p["T"], p["J"], p["L"]
    betas = gd.get_named_beta_schedule("cosine", 1000)

    def diffusion(respacing):
        return SpacedDiffusion(use_timesteps=space_timesteps(1000, respacing), betas=betas, model_mean_type=gd.ModelMeanType.START_X,
                               model_var_type=gd.ModelVarType.FIXED_SMALL, loss_type=gd.LossType.MSE)

    x, seedp, mfcc = synthetic_inputs(cfg, B, T, seed=10)
    x = x.to(dev)
    y_cfg = {"seed": seedp.to(dev), "mfcc": mfcc.to(dev), "scale": torch.full((B,), 2.5, device=dev)}
    guided = ClassifierFreeSampleModel(model)
    own = os.path.abspath(a.tree) == os.path.abspath(os.path.join(HERE, ".."))
    rec = dict(tool="layer_cache", tree="this checkout" if own else "parent", config=a.config, label=p["label"], arch=p["arch"],
               B=B, T=T, J=J, d=p["d"], L=L, dtype=a.dtype, scale=2.5, device=torch.cuda.get_device_name(0))
    name = lambda e, k: f"e{e}k{k}"      # noqa: E731

    if a.deviation:
        rec["measure"] = "max|x - uncached| / max|uncached| of the final sample, ancestral loop, random weights"
        for respacing in ("ddim10", "ddim50", [1000]):
            df = diffusion(respacing)
            kw = dict(noise=x, clip_denoised=False, rng="philox", philox_seed=10)
            full = df.p_sample_loop(guided, (B, J, 1, T), model_kwargs={"y": y_cfg}, **kw)
            top = float(full.abs().max())
            row = {}
            for e, k in a.cache:
                r = df.p_sample_loop(guided, (B, J, 1, T), model_kwargs={"y": dict(y_cfg, layer_cache=(e, k))}, **kw)
                assert torch.isfinite(r).all(), (e, k)
                row[name(e, k)] = float(f"{float((r - full).abs().max()) / top:.3e}")
            for k in sorted({k for _, k in a.cache}):           # the same weights (each tensor is seeded by its name) without layers k .. L-1
                small, _, _ = build_model(p["arch"], J, p["d"], k, dev)
                small.compute_dtype = a.dtype
                r = df.p_sample_loop(ClassifierFreeSampleModel(small), (B, J, 1, T), model_kwargs={"y": y_cfg}, **kw)
                row[f"dropped_k{k}"] = float(f"{float((r - full).abs().max()) / top:.3e}")
            rec["full1000" if respacing == [1000] else respacing] = row
    else:
        df = diffusion([1000])
        n = df.num_timesteps
        steps = min(n, a.steps) if a.steps > 0 else n

        def loop(y, skip):
            return df.p_sample_loop(guided, (B, J, 1, T), noise=x, clip_denoised=False, model_kwargs={"y": y}, skip_timesteps=skip,
                                    rng="philox", philox_seed=10)

        rows = {"nokey": y_cfg}
        if not a.baseline:
            rows["off"] = dict(y_cfg, layer_cache=(1, 0))
            for e, k in a.cache:
                rows[name(e, k)] = dict(y_cfg, layer_cache=(e, k))
            rows["shallow1"] = dict(y_cfg, layer_cache=(10**6, 1))     # one full call, then 1 / 2 layers: the encoder's share
            rows["shallow2"] = dict(y_cfg, layer_cache=(10**6, 2))
        for y in rows.values():                                 # warm-up: every row's kernels at the timed size
            loop(y, max(0, n - 20))
        torch.cuda.synchronize()
        ms = {k: [] for k in rows}
        for _ in range(a.repeats):
            for k, y in rows.items():                           # alternate the rows inside each repeat
                t, r = timed(torch, lambda y=y: loop(y, n - steps))
                assert torch.isfinite(r).all(), k
                ms[k].append(t / steps)
        rec.update(sampler="p", steps=steps, repeats=a.repeats)
        for k, v in ms.items():
            rec[k] = dict(ms_per_step=round(statistics.median(v), 5), min_max=[round(min(v), 5), round(max(v), 5)])
        if not a.baseline:
            base = rec["off"]["ms_per_step"]
            t1, t2 = rec["shallow1"]["ms_per_step"], rec["shallow2"]["ms_per_step"]
            per_layer = t2 - t1                                 # one layer of a partial call (the one full call: 1 / steps of the loop)
            share = L * per_layer / base
            rec["encoder"] = dict(ms_per_layer=round(per_layer, 5), share_of_step=round(share, 4),
                                  rest_with_apply_ms=round(t1 - per_layer, 5), rest_ms=round(base - L * per_layer, 5))
            for e, k in a.cache:
                pred = share * (1 + (e - 1) * k / L) / e + (1 - share)
                rec[name(e, k)].update(ratio_to_off=round(rec[name(e, k)]["ms_per_step"] / base, 4), prediction=round(pred, 4),
                                       encoder_factor=round((1 + (e - 1) * k / L) / e, 4))
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
