#!/usr/bin/env python3
"""Outputs of the 16-bit GEMM kernels (csrc/gemmh.hip) of two builds of libgdx.so, bit for bit (needs an MI355X).

    python tools/gemmh_ab.py OLD_LIBGDX_SO NEW_LIBGDX_SO

Each library runs, in a fresh child process of its own (GDX_LIBGDX), one after the other, gdx_linear_half on the same seeded
inputs and reports a SHA-256 per output, C32 and C16 apart, with the `launched` tuple in the output's name (a changed
dispatch shows as a difference): fp16 and bf16, every tile of tests/test_gpu_half_blocks.py's GH_TILES and the cost model
(0, 0), its GEMM_SHAPES x EPILOGUES; the shape of its eight-wave three-round test under both of that test's epilogues, tiles
(16, 4) and (8, 4); config 5's row-cut shape (66 688 x 1 024 x 1 024, + R into C32) under (0, 0) and (16, 4); and one forward
of the tiny V1 model and of the V2 model at d = 512 per 16-bit type.
Prints one line per output, one condensed line per (dtype, shape) and a summary line; exit status 1 on any difference."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = {"v1": ("mdm_old", 128, 256), "v2d512": ("mdm", 512, 1024)}     # arch, latent_dim, ff_size


def child(out_path):
    sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
    import torch
    import test_gpu_half_blocks as T
    from gesturediffusion_amd import _lib
    from gesturediffusion_amd.model.mdm import MDM
    from gesturediffusion_amd.model.mdm_old import MDM_Old
    from gesturediffusion_amd.utils.init import init_state_dict, synthetic_inputs
    dev = torch.device("cuda:0")
    lib = _lib.load()
    report = {}

    def put(name, t):
        report[name] = hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()

    def problem(M, N, K, Tn, seed):
        g = torch.Generator(device=dev).manual_seed(seed)
        A = torch.randn(M, K, device=dev, generator=g)
        W = torch.randn(N, K, device=dev, generator=g) / K ** 0.5
        bias = torch.randn(N, device=dev, generator=g)
        R = torch.randn(M + (M - 1) // Tn + 1, N + 4, device=dev, generator=g)
        V = torch.randn((M + Tn - 1) // Tn, N + 8, device=dev, generator=g)
        return A, W, bias, R, V

    def linear(tag, prob, M, N, K, Tn, ename, dtype, tile):
        A, W, bias, R, V = prob
        ub, gelu, uR, uV, rowmap, w32, w16 = T.EPILOGUES[ename]
        rows = (R.shape[0] if rowmap else M) + 3
        c32 = torch.full((rows, N), float("nan"), device=dev) if w32 else None
        c16 = torch.full((rows, N), float("nan"), device=dev) if w16 else None
        la = T.run_linear_half(lib, A, W, bias if ub else None, R if uR else None, R.shape[1], V if uV else None, V.shape[1], c32,
                               c16, M, N, K, Tn, rowmap, gelu, dtype, tile)
        for buf, nm in ((c32, "C32"), (c16, "C16")):
            if buf is not None:
                put(f"{tag} {ename} tile={tile[0]},{tile[1]} ran={'/'.join(map(str, la))} {nm}", buf)

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for dtype in (T.F16, T.BF16):
        dname = T.NAME[dtype]
        for M, N, K, Tn in T.GEMM_SHAPES:
            prob = problem(M, N, K, Tn, M * 7 + N + dtype)
            for ename in T.EPILOGUES:
                for tile in T.GH_TILES + [(0, 0)]:
                    linear(f"{dname} {M}x{N}x{K} T={Tn}", prob, M, N, K, Tn, ename, dtype, tile)
        M, N, K, Tn = 256 * ((2 * cus + 2) // 2) - 100, 512, 320, 197
        prob = problem(M, N, K, Tn, M + dtype)
        for ename in ("bias", "res_rowmap"):
            for tile in ((16, 4), (8, 4)):
                linear(f"{dname} {M}x{N}x{K} T={Tn}", prob, M, N, K, Tn, ename, dtype, tile)
        M, N, K = 66688, 1024, 1024
        prob = problem(M, N, K, 1, 5)
        for tile in ((0, 0), (16, 4)):
            linear(f"{dname} {M}x{N}x{K} T=1", prob, M, N, K, 1, "res_c32", dtype, tile)
        del prob
        for mname, (arch, d, ff) in MODELS.items():
            cfg = dict(arch=arch, njoints=16, nfeats=1, latent_dim=d, ff_size=ff, num_layers=2, num_heads=4, seed_poses=10)
            m = (MDM if arch == "mdm" else MDM_Old)(
                njoints=16, nfeats=1, translation=True, pose_rep="rot6d", glob=True, glob_rot=True, latent_dim=d, ff_size=ff,
                num_layers=2, num_heads=4, data_rep="genea_vec", cond_mask_prob=0.1, dataset="genea2023", mfcc_input=True,
                seed_poses=10, compute_dtype=dname)
            m.load_state_dict(init_state_dict(cfg, seed=31, perturb=True), strict=False)
            m.to(dev).eval()
            x, seedp, mfcc = synthetic_inputs(cfg, 3, 20, seed=5)
            with torch.no_grad():
                out = m(x.to(dev), torch.tensor([17, 803, 0], device=dev), {"seed": seedp.to(dev), "mfcc": mfcc.to(dev)})
            put(f"{dname} forward {mname}", out)
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
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], check=True, timeout=420,
                           env=dict(os.environ, GDX_LIBGDX=lib))
            reports.append(json.load(open(path)))
    old, new = reports
    bad = 0
    groups = {}
    for name in sorted(set(old) | set(new)):
        same = old.get(name) == new.get(name)
        bad += not same
        print("%-86s old %s  new %s  %s" % (name, old.get(name, "-")[:16], new.get(name, "-")[:16], "identical" if same else "DIFFERENT"))
        g = groups.setdefault(" ".join(name.split()[:3]), [0, 0, hashlib.sha256()])
        g[0] += 1
        g[1] += not same
        g[2].update((new.get(name) or "").encode())
    for key, (n, nd, h) in groups.items():
        print("## %-34s %3d outputs, %d different, sha256 of the new hashes %s" % (key, n, nd, h.hexdigest()[:16]))
    print("# %d outputs compared, %d differences" % (len(set(old) | set(new)), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
