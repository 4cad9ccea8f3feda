#!/usr/bin/env python3
"""ms/step of the fused ancestral loop under perturbed-attention guidance (y['pag_scale'], y['pag_layers']):
    python tools/guidance_pag.py [--config genea|3] [--dtype fp32|fp16] [--steps N] [--repeats 3] [--baseline] [--tree DIR]
                                 [--check] [--copy] [--out profiles/FILE.txt]
Rows: "cond"    = the inner model alone (one pass per step),
      "joint"   = ClassifierFreeSampleModel, today's cond / uncond pair (2 passes),
      "pag"     = PerturbedAttentionSampleModel (GDX_PAG_ONLY: conditional and perturbed pass, 2 passes),
      "pag_cfg" = ClassifierFreeSampleModel with y['pag_scale'] (GDX_PAG_CFG: 3 passes).
--baseline times ONLY "cond" and "joint" and touches nothing a tree without the feature lacks; with --tree DIR the package (and
its library) are taken from that checkout -- the parent commit's -- so both sides run in one job on one box, alternating
processes; repeating the parent's process gives the run-to-run spread "joint" is held against.
The model is MDM at the preset's width, depth and batch with random weights: "genea" is sample.generate's chunk (B = 41, T = 120),
"3" is BASELINE config 3's shape with T = 200 in place of 196 (the local attention needs a multiple of its window).  The perturbed
layer is the default, the middle one.  The loop is p_sample_loop on the 1000-step schedule with in-kernel Philox noise, its last N
steps (--steps): "joint" and "pag" take gdx_sample_loop's token-major path, "pag_cfg" the pose-layout path (two transposes per
step more) plus the compose launch.  Every process first warms a short loop per row, then times each row `repeats` times between
two events on the stream, rows alternating inside each repeat, each timed loop behind one untimed step of the same row (a switch
between two and three row groups re-allocates the workspace, which is a cost per switch, not per step); median and min / max per
step, and each row's ratio to "joint".  "moved": max |sample - the unguided loop's sample| / max |that sample| at the end of the timed
loop, at w = 1 and w = 3 under "pag" (random weights: how far the guidance moves a sample, nothing about motion quality).
--check asserts that group F of a GDX_PAG_ONLY forward (an empty guidance interval returns it) has the bits of a GDX_COND forward.
--copy times gdx_attention_identity alone on a buffer large enough to hide the entry's synchronisation, and prices the step's copy
(B * (T + 1) rows of d elements) at that rate.  One JSON line per run."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = {"genea": dict(J=498, d=256, L=8, T=120, batch=41, label="GENEA chunk (sample.generate's workload)"),
          "3": dict(J=263, d=512, L=8, T=200, batch=256, label="BASELINE config 3's shape on MDM, T = 200")}


def timed(torch, fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    r = fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop), r


def copy_rate(torch, E, dev, dtype, rows, d, calls=10):
    """GB/s of gdx_attention_identity (bytes read + bytes written) over `calls` synchronous calls, after two warm-up calls."""
    qkv = torch.randn(rows, 3 * d, device=dev).to(dtype)
    ctx = torch.empty(rows, d, device=dev, dtype=dtype)
    for _ in range(2):
        E.attention_identity(qkv, ctx)
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        E.attention_identity(qkv, ctx)
        ts.append(time.perf_counter() - t0)
    assert torch.equal(ctx, qkv[:, 2 * d:])
    moved = 2 * rows * d * ctx.element_size()
    return moved, moved / statistics.median(ts) / 1e9, moved / max(ts) / 1e9, moved / min(ts) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="genea", choices=sorted(SHAPES))
    ap.add_argument("--dtype", default="fp32", choices=["fp32", "fp16"])
    ap.add_argument("--steps", type=int, default=50, help="time only the last N steps of the 1000-step schedule")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--baseline", action="store_true", help="time only the rows a tree without the feature has")
    ap.add_argument("--tree", default=os.path.join(HERE, ".."), help="checkout whose package and library are measured")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--copy", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch
    from gesturediffusion_amd import _lib
    from gesturediffusion_amd import engine as E
    from gesturediffusion_amd.diffusion import gaussian_diffusion as gd
    from gesturediffusion_amd.diffusion.respace import SpacedDiffusion, space_timesteps
    from gesturediffusion_amd.model.cfg_sampler import ClassifierFreeSampleModel
    from gesturediffusion_amd.model.mdm import MDM
    from gesturediffusion_amd.utils.init import init_state_dict, synthetic_inputs
    assert os.path.abspath(_lib.__file__).startswith(os.path.abspath(a.tree) + os.sep), _lib.__file__
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    p = SHAPES[a.config]
    dev = torch.device("cuda:0")
    B, T, J = p["batch"], p["T"], p["J"]
    cfg = dict(arch="mdm", njoints=J, nfeats=1, latent_dim=p["d"], ff_size=1024, num_layers=p["L"], num_heads=4, seed_poses=10)
    model = MDM(njoints=J, nfeats=1, translation=True, pose_rep="rot6d", glob=True, glob_rot=True, latent_dim=p["d"], ff_size=1024,
                num_layers=p["L"], num_heads=4, dropout=0.1, activation="gelu", data_rep="genea_vec", cond_mask_prob=0.1,
                dataset="genea2023", use_text=False, mfcc_input=True, use_wav_enc=False, seed_poses=10, use_audio=False)
    model.load_state_dict(init_state_dict(cfg, seed=0), strict=False)
    model.to(dev).eval()
    model.compute_dtype = a.dtype
    df = SpacedDiffusion(use_timesteps=space_timesteps(1000, [1000]), betas=gd.get_named_beta_schedule("cosine", 1000),
                         model_mean_type=gd.ModelMeanType.START_X, model_var_type=gd.ModelVarType.FIXED_SMALL,
                         loss_type=gd.LossType.MSE)
    n = df.num_timesteps
    steps = min(n, a.steps) if a.steps > 0 else n
    x, seedp, mfcc = (v.to(dev) for v in synthetic_inputs(cfg, B, T, seed=10))
    y_in = {"seed": seedp, "mfcc": mfcc}
    y_cfg = dict(y_in, scale=torch.full((B,), 2.5, device=dev))
    guided = ClassifierFreeSampleModel(model)

    def loop(m, y, skip):
        return df.p_sample_loop(m, (B, J, 1, T), noise=x, clip_denoised=False, model_kwargs={"y": y}, skip_timesteps=skip,
                                rng="philox", philox_seed=10)

    rows = {"cond": (model, y_in), "joint": (guided, y_cfg)}
    if not a.baseline:
        from gesturediffusion_amd.model.pag_sampler import PerturbedAttentionSampleModel
        pag = PerturbedAttentionSampleModel(model)
        w3 = torch.full((B,), 3.0, device=dev)
        rows["pag"] = (pag, dict(y_in, pag_scale=w3))
        rows["pag_cfg"] = (guided, dict(y_cfg, pag_scale=w3))
    for m, y in rows.values():                                  # warm-up: every row's kernels at the timed size
        loop(m, y, max(0, n - 10))
    torch.cuda.synchronize()
    ms = {k: [] for k in rows}
    last = {}
    for _ in range(a.repeats):
        for k, (m, y) in rows.items():                          # alternate the rows inside each repeat
            # one untimed step first: a row with another number of row groups than the row before it re-prepares the workspace
            # (gdx_set_attention_guidance allocates), once per switch and not per step
            loop(m, y, n - 1)
            t, r = timed(torch, lambda m=m, y=y: loop(m, y, n - steps))
            assert torch.isfinite(r).all(), k
            ms[k].append(t / steps)
            last[k] = r.clone()
    own = os.path.abspath(a.tree) == os.path.abspath(os.path.join(HERE, ".."))
    rec = dict(tool="guidance_pag", tree="this checkout" if own else "parent", config=a.config, label=p["label"], B=B, T=T, J=J,
               d=p["d"], L=p["L"], dtype=a.dtype, scale=2.5, pag_scale=3.0, pag_layers=[p["L"] // 2], sampler="p", steps=steps,
               repeats=a.repeats, device=torch.cuda.get_device_name(0))
    for k, v in ms.items():
        rec[k] = dict(ms_per_step=round(statistics.median(v), 5), min_max=[round(min(v), 5), round(max(v), 5)])
    joint = rec["joint"]["ms_per_step"]
    rec["ratio_to_joint"] = {k: round(rec[k]["ms_per_step"] / joint, 4) for k in ms}
    if not a.baseline:
        def moved(r):
            return round(float((r - last["cond"]).abs().max() / last["cond"].abs().max()), 4)
        w1 = loop(pag, dict(y_in, pag_scale=torch.full((B,), 1.0, device=dev)), n - steps)
        rec["moved"] = {"pag_w1": moved(w1), "pag_w3": moved(last["pag"]), "joint_s2.5": moved(last["joint"])}
    if a.check and not a.baseline:
        t = torch.full((B,), 500, device=dev, dtype=torch.long)
        want = model(x, t, y_in).clone()
        got = pag(x, t, dict(y_in, pag_scale=w3, guidance_interval=(1, 0)))          # lo > hi: no sample is guided, each is F
        assert torch.equal(got, want), "group F of a GDX_PAG_ONLY forward differs from the GDX_COND forward"
        assert not torch.equal(pag(x, t, dict(y_in, pag_scale=w3)), want)
        rec["check"] = "group F under GDX_PAG_ONLY == GDX_COND forward, bit for bit"
    if a.copy and not a.baseline:
        dt = torch.float32 if a.dtype == "fp32" else torch.float16
        big = (1 << 31) // (p["d"] * 4)                                               # 2 GiB of ctx at 4-byte elements
        moved_b, med, lo, hi = copy_rate(torch, E, dev, dt, big, p["d"])
        step_bytes = 2 * B * (T + 1) * p["d"] * (4 if a.dtype == "fp32" else 2)
        rec["copy"] = dict(rows=big, d=p["d"], bytes_moved=moved_b, GBps=round(med, 1), GBps_min_max=[round(lo, 1), round(hi, 1)],
                           step_copy_bytes=step_bytes, step_copy_us_at_that_rate=round(step_bytes / med / 1e3, 3),
                           share_of_pag_step=round(step_bytes / med / 1e6 / rec["pag"]["ms_per_step"], 5))
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
