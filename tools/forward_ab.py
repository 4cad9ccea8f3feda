#!/usr/bin/env python3
"""The denoiser's forward and the in-library loops of two builds of libgdx.so, bit for bit (needs an MI355X).

    python tools/forward_ab.py OLD_LIBGDX_SO NEW_LIBGDX_SO

Each library runs, in a fresh child process of its own (GDX_LIBGDX), one after the other, the per-step kernel sequence on the
same seeded inputs through every branch of its host code and reports a SHA-256 per output:

  * compute dtype fp32, fp16 (16-bit residual stream) and bf16 (fp32 residual stream);
  * V1 tiny (d=128, head width 32: the general attention kernel), V2 d=512 (d / cl_head = 64: the 16-bit front end in the 16-bit
    modes) and V2 d=256 (d / cl_head = 32: the fp32 front end, proj_pose writes fp32), B=3, T=20; in fp32 also V2 d=512 at T=30
    (attention3) and T=260 (S=261 > 256: the general attention kernel);
  * gdx_forward as COND, UNCOND and CFG: the output with keep_taps off, the output and every tap with keep_taps on;
  * loops with CFG + clip and Philox noise: a 6-step gdx_sample_loop (token-major path), the same with an inpainting mask (eager
    path), the same with graph replay on at 6 steps and at 12 (from 9 steps on the step is captured and replayed), one
    gdx_plms_loop and one gdx_bpd_loop.

Prints one line per output and a summary line; exit status 1 on any difference.

    GDX_LIBGDX=LIBGDX_SO rocprofv3 --kernel-trace --stats -- python tools/forward_ab.py --child OUT.json --brief

is the workload for comparing the launches of two builds: one CFG forward and the token-major loop of V2 d=512 in each dtype."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = ("fp32", "fp16", "bf16")
# name: (arch, latent_dim, ff_size, frames, dtypes, loops too)
CONFIGS = {
    "v1": ("mdm_old", 128, 256, 20, ALL, True),
    "v2d512": ("mdm", 512, 1024, 20, ALL, True),
    "v2d256": ("mdm", 256, 512, 20, ALL, True),
    "v2d512T30": ("mdm", 512, 1024, 30, ("fp32",), False),
    "v2d512T260": ("mdm", 512, 1024, 260, ("fp32",), False),
}
B, J, L, H = 3, 16, 2, 4


def child(out_path):
    sys.path.insert(0, REPO)
    import torch
    from gesturediffusion_amd.diffusion import gaussian_diffusion as gd
    from gesturediffusion_amd.diffusion.respace import SpacedDiffusion, space_timesteps
    from gesturediffusion_amd.engine import GDX_CFG, GDX_COND, GDX_UNCOND
    from gesturediffusion_amd.model.cfg_sampler import ClassifierFreeSampleModel
    from gesturediffusion_amd.model.mdm import MDM
    from gesturediffusion_amd.model.mdm_old import MDM_Old
    from gesturediffusion_amd.utils.init import init_state_dict, synthetic_inputs
    dev = torch.device("cuda:0")
    brief = "--brief" in sys.argv
    report = {}

    def put(name, *tensors):
        for i, t in enumerate(tensors):
            report[f"{name}.{i}"] = hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()

    def diffusion(steps, var="FIXED_SMALL"):
        return SpacedDiffusion(use_timesteps=space_timesteps(1000, [steps]), betas=gd.get_named_beta_schedule("cosine", 1000),
                               model_mean_type=gd.ModelMeanType.START_X, model_var_type=getattr(gd.ModelVarType, var),
                               loss_type=gd.LossType.MSE)

    for name, (arch, d, ff, T, dtypes, loops) in CONFIGS.items():
        if brief and name != "v2d512":
            continue
        cfg = dict(arch=arch, njoints=J, nfeats=1, latent_dim=d, ff_size=ff, num_layers=L, num_heads=H, seed_poses=10)
        sd = init_state_dict(cfg, seed=31, perturb=True)
        x, seedp, mfcc = (v.to(dev) for v in synthetic_inputs(cfg, B, T, seed=5))
        t = torch.tensor([17, 803, 0], device=dev)
        scale = torch.tensor([2.5, 1.0, 0.5], device=dev)
        for dtype in dtypes:
            m = (MDM if arch == "mdm" else MDM_Old)(
                njoints=J, nfeats=1, translation=True, pose_rep="rot6d", glob=True, glob_rot=True, latent_dim=d, ff_size=ff,
                num_layers=L, num_heads=H, data_rep="genea_vec", cond_mask_prob=0.1, dataset="genea2023", mfcc_input=True,
                seed_poses=10, compute_dtype=dtype)
            m.load_state_dict(sd, strict=False)
            m.to(dev).eval()
            eng = m._get_engine(dev)
            eng.prepare(B, T)
            for taps in (False,) if brief else (False, True):
                eng.keep_taps(taps)
                eng.set_condition(seedp, mfcc, cache=False)
                for mode, mname in ((GDX_COND, "cond"), (GDX_UNCOND, "uncond"), (GDX_CFG, "cfg"))[2 if brief else 0:]:
                    tag = f"forward.{name}.{dtype}.{mname}.taps{taps:d}"
                    put(tag, eng.forward(x, t, mode, scale if mode == GDX_CFG else None))
                    rows = (2 * B if mode == GDX_CFG else B) * (T + 1)
                    if taps:
                        put(tag + ".tap", *[eng.tap(i, rows, d, dev) for i in range(L + 1)])
            eng.keep_taps(False)
            if not loops:
                continue
            guided = ClassifierFreeSampleModel(m)
            y = {"seed": seedp, "mfcc": mfcc, "scale": scale}
            g = torch.Generator().manual_seed(T)
            y_inp = dict(y, inpainting_mask=(torch.rand(x.shape, generator=g) < 0.3).to(dev),
                         inpainted_motion=torch.randn(x.shape, generator=g).to(dev))
            kw = dict(clip_denoised=True, rng="philox", philox_seed=9)
            tag = f"loop.{name}.{dtype}"
            put(tag + ".token_major", diffusion(6).p_sample_loop(guided, x.shape, model_kwargs={"y": y}, **kw))
            if brief:
                continue
            put(tag + ".inpaint", diffusion(6).p_sample_loop(guided, x.shape, model_kwargs={"y": y_inp}, **kw))
            eng.set_graph_replay(True)
            for steps in (6, 12):
                put(f"{tag}.graph{steps}", diffusion(steps).p_sample_loop(guided, x.shape, model_kwargs={"y": y}, **kw))
            eng.set_graph_replay(False)
            put(tag + ".plms", diffusion(6).plms_sample_loop(guided, x.shape, model_kwargs={"y": y}, **kw))
            r = diffusion(6, "FIXED_LARGE").calc_bpd_loop(guided, 0.6 * x, model_kwargs={"y": y}, **kw)
            put(tag + ".bpd", *[r[k] for k in sorted(r)])
    torch.cuda.synchronize()
    json.dump(report, open(out_path, "w"))


def main():
    if sys.argv[1] == "--child":
        return child(sys.argv[2])
    libs = [os.path.abspath(p) for p in sys.argv[1:3]]
    reports = []
    with tempfile.TemporaryDirectory() as tmp:
        for i, lib in enumerate(libs):
            path = os.path.join(tmp, f"report{i}.json")
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], check=True, timeout=240,
                           env=dict(os.environ, GDX_LIBGDX=lib))
            reports.append(json.load(open(path)))
    old, new = reports
    bad = 0
    for name in sorted(set(old) | set(new)):
        same = old.get(name) == new.get(name)
        bad += not same
        print("%-50s old %s  new %s  %s" % (name, old.get(name, "-")[:16], new.get(name, "-")[:16], "identical" if same else "DIFFERENT"))
    print("# %d outputs compared, %d differences" % (len(set(old) | set(new)), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
