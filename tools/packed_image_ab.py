#!/usr/bin/env python3
"""Packed weight images of two builds of libgdx.so, byte for byte (needs an MI355X).

    python tools/packed_image_ab.py OLD_LIBGDX_SO NEW_LIBGDX_SO

Each library exports, in a child process of its own (GDX_LIBGDX), the packed image of the same seeded state dicts: both
topologies x fp32 / fp16 / bf16 at the tests' tiny configuration, and each topology once at a real size.  The new
library's child then uploads every image the OLD library wrote into a fresh model whose own parameters are other weights
and compares its forward, with torch.equal, against the forward either library computes from the state dict.  Prints one line
per case (SHA-256 of both images) and a summary line; exit status 1 on any difference."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(njoints=16, nfeats=1, latent_dim=128, ff_size=256, num_layers=2, num_heads=4, seed_poses=10)
REAL = dict(njoints=263, nfeats=1, latent_dim=512, ff_size=1024, num_layers=8, num_heads=4, seed_poses=10)
CASES = [("tiny", arch, dtype) for arch in ("mdm", "mdm_old") for dtype in ("fp32", "fp16", "bf16")] + \
        [("real", "mdm", "fp16"), ("real", "mdm_old", "fp32")]


def child(out, old):
    sys.path.insert(0, REPO)
    import torch
    from gesturediffusion_amd.model.mdm import MDM
    from gesturediffusion_amd.model.mdm_old import MDM_Old
    from gesturediffusion_amd.utils.init import init_state_dict, synthetic_inputs
    dev = torch.device("cuda:0")

    def model(arch, cfg, dtype, seed):
        m = (MDM if arch == "mdm" else MDM_Old)(njoints=cfg["njoints"], nfeats=1, translation=True, pose_rep="rot6d", glob=True,
                                                 glob_rot=True, latent_dim=cfg["latent_dim"], ff_size=cfg["ff_size"],
                                                 num_layers=cfg["num_layers"], num_heads=cfg["num_heads"], data_rep="genea_vec",
                                                 cond_mask_prob=0.1, dataset="genea2023", mfcc_input=True,
                                                 seed_poses=cfg["seed_poses"], compute_dtype=dtype)
        m.load_state_dict(init_state_dict(cfg, seed=seed, perturb=True), strict=False)
        return m.to(dev).eval()

    def forward(m, cfg):
        x, seedp, mfcc = synthetic_inputs(cfg, 3, 20, seed=5)
        return m(x.to(dev), torch.tensor([3, 500, 999], device=dev), y={"seed": seedp.to(dev), "mfcc": mfcc.to(dev)}).cpu()

    report = {}
    for size, arch, dtype in CASES:
        name = f"{size}_{arch}_{dtype}"
        cfg = dict(TINY if size == "tiny" else REAL, arch=arch)
        m = model(arch, cfg, dtype, seed=31)
        y = forward(m, cfg)
        blob = m.export_packed(dev)
        report[name] = {"sha256": hashlib.sha256(blob).hexdigest(), "bytes": len(blob)}
        if old is None:                                  # the old library's child: leave the image and the forward behind
            open(os.path.join(out, name + ".gdxpack"), "wb").write(blob)
            torch.save(y, os.path.join(out, name + ".pt"))
            continue
        other = model(arch, cfg, dtype, seed=32)
        assert not torch.equal(forward(other, cfg), y)
        other.load_packed(open(os.path.join(old, name + ".gdxpack"), "rb").read(), dev)
        got = forward(other, cfg)
        report[name]["old_image_forward_equal"] = bool(torch.equal(got, y) and torch.equal(got, torch.load(os.path.join(old, name + ".pt"))))
    json.dump(report, open(os.path.join(out, "report.json"), "w"))


def main():
    if sys.argv[1] == "--child":
        return child(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
    old_lib, new_lib = (os.path.abspath(p) for p in sys.argv[1:3])
    with tempfile.TemporaryDirectory() as tmp:
        dirs = [os.path.join(tmp, "old"), os.path.join(tmp, "new")]
        for d, lib, extra in ((dirs[0], old_lib, []), (dirs[1], new_lib, [dirs[0]])):
            os.mkdir(d)
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", d, *extra], check=True, timeout=240,
                           env=dict(os.environ, GDX_LIBGDX=lib))
        old, new = (json.load(open(os.path.join(d, "report.json"))) for d in dirs)
    bad = 0
    for name in old:
        same = old[name] == {k: new[name][k] for k in ("sha256", "bytes")}
        ok = same and new[name]["old_image_forward_equal"]
        bad += not ok
        print("%-22s %10d bytes  old %s  new %s  %s, the old image in the new handle: forward %s" %
              (name, old[name]["bytes"], old[name]["sha256"], new[name]["sha256"], "identical" if same else "DIFFERENT",
               "equal" if new[name]["old_image_forward_equal"] else "DIFFERENT"))
    print("# %d images compared, %d differences" % (len(old), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
