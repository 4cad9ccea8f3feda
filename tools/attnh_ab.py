#!/usr/bin/env python3
"""Outputs of the 16-bit self-attention kernels (csrc/attentionh.hip) of two builds of libgdx.so, bit for bit (needs an MI355X).

    python tools/attnh_ab.py OLD_LIBGDX_SO NEW_LIBGDX_SO

Each library runs, in a fresh child process of its own (GDX_LIBGDX), one after the other, gdx_attention_half on the same seeded
inputs and reports a SHA-256 per output: fp16 and bf16, every head width 32 / 64 / 96 / 128 / 192 / 256 under every kernel that
exists for it (forced: 1 = h8, 2 = h8q, 3 = h8p) and under the forward's dispatch (0), at B = 2, H = 2 and S in SWEEP_S (partial
last query block, partial last key tile, one to four chunks and the chunk boundary at 17 blocks); the item-walk shapes of
tests/test_gpu_attention_half.py under h8p at grids 1, 3, 8, 9, 13, 64; one rescale ramp (scores rising by 9 per tile) at
S = 200; and one whole forward of the tiny model in fp16 and in bf16.
Prints one line per output, one condensed line per (dtype, head width, kernel) and a summary line; exit status 1 on any
difference."""
import ctypes as C
import hashlib
import json
import math
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(arch="mdm", njoints=16, nfeats=1, latent_dim=128, ff_size=256, num_layers=2, num_heads=4, seed_poses=10)
DTYPES = {"fp16": 1, "bf16": 2}                                       # GDX_DTYPE_*
SWEEP_S = [1, 13, 16, 17, 29, 45, 197, 257, 300, 521, 769]
WALK = [(3, 2, 300, 64), (2, 3, 521, 128), (1, 2, 769, 256), (5, 1, 45, 64), (2, 2, 13, 128)]   # B, H, S, hd
WALK_GRIDS = [1, 3, 8, 9, 13, 64]
PAD = 48                                                              # readable rows past B*S


def child(out_path):
    sys.path.insert(0, REPO)
    import torch
    from gesturediffusion_amd import _lib
    from gesturediffusion_amd.model.mdm import MDM
    from gesturediffusion_amd.utils.init import init_state_dict, synthetic_inputs
    dev = torch.device("cuda:0")
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    report = {}

    def put(name, t):
        report[name] = hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()

    def attention(name, qkv, B, S, H, d, dtype, kernel, grid=0):
        ctx = torch.full((B * S + 3, d), float("nan"), device=dev)
        rep = (C.c_int32 * 3)()
        _lib.check(lib.gdx_attention_half(C.c_void_p(qkv.data_ptr()), qkv.shape[0], C.c_void_p(ctx.data_ptr()), ctx.shape[0], B, S,
                                          H, d, dtype, kernel, grid, rep, stream), lib)
        assert kernel == 0 or rep[0] == kernel, (name, tuple(rep))
        put(f"{name} ran={rep[0]}/{rep[1]}/{rep[2]}", ctx)

    def random_qkv(B, S, d, seed):
        g = torch.Generator(device=dev).manual_seed(seed)
        qkv = torch.randn(B * S + PAD, 3 * d, device=dev, generator=g)
        qkv[:, :d] *= 2.0
        qkv[B * S:] = 0
        return qkv

    def ramp_qkv(B, S, H, hd, seed):                                 # log2-domain scores rise by 9 per 32-key tile
        g = torch.Generator(device=dev).manual_seed(seed)
        c = math.log2(math.e) / math.sqrt(hd)
        Q = torch.randn(B, S, H, hd, device=dev, generator=g) * 0.25
        K = torch.randn(B, S, H, hd, device=dev, generator=g) * 0.25
        j = torch.arange(S, device=dev).double()
        Q[..., 0] = 4.0 - 0.5 * (torch.arange(S, device=dev) % 4).float().view(1, S, 1)
        K[..., 0] = ((9.0 * torch.floor(j / 32) + 0.5 * (j % 32) / 32).float() / (4.0 * c)).view(1, S, 1)
        V = torch.randn(B, S, H, hd, device=dev, generator=g)
        rows = torch.cat([Q.reshape(B * S, H * hd), K.reshape(B * S, H * hd), V.reshape(B * S, H * hd)], dim=1)
        return torch.cat([rows, torch.zeros(PAD, 3 * H * hd, device=dev)])

    for dname, dtype in DTYPES.items():
        for hd in (32, 64, 96, 128, 192, 256):
            kernels = (0, 1, 2, 3) if hd in (64, 128, 256) else (0, 1)
            B, H = 2, 2
            for S in SWEEP_S:
                qkv = random_qkv(B, S, H * hd, seed=1000 * hd + S)
                for k in kernels:
                    attention(f"{dname} hd={hd} k={k} sweep S={S}", qkv, B, S, H, H * hd, dtype, k)
            qkv = ramp_qkv(B, 200, H, hd, seed=hd)
            for k in kernels:
                attention(f"{dname} hd={hd} k={k} ramp S=200", qkv, B, 200, H, H * hd, dtype, k)
        for B, H, S, hd in WALK:
            qkv = random_qkv(B, S, H * hd, seed=S + hd)
            for grid in WALK_GRIDS:
                attention(f"{dname} hd={hd} k=3 walk B={B} H={H} S={S} grid={grid}", qkv, B, S, H, H * hd, dtype, 3, grid)
        m = MDM(njoints=16, nfeats=1, translation=True, pose_rep="rot6d", glob=True, glob_rot=True, latent_dim=128, ff_size=256,
                num_layers=2, num_heads=4, data_rep="genea_vec", cond_mask_prob=0.1, dataset="genea2023", mfcc_input=True,
                seed_poses=10, compute_dtype=dname)
        m.load_state_dict(init_state_dict(TINY, seed=31, perturb=True), strict=False)
        m.to(dev).eval()
        x, seedp, mfcc = synthetic_inputs(TINY, 3, 20, seed=5)
        with torch.no_grad():
            out = m(x.to(dev), torch.tensor([17, 803, 0], device=dev), {"seed": seedp.to(dev), "mfcc": mfcc.to(dev)})
        put(f"{dname} forward tiny", out)
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
    groups = {}
    for name in sorted(set(old) | set(new)):
        same = old.get(name) == new.get(name)
        bad += not same
        print("%-66s old %s  new %s  %s" % (name, old.get(name), new.get(name), "identical" if same else "DIFFERENT"))
        key = " ".join(name.split()[:3]) if " hd=" in name else name
        g = groups.setdefault(key, [0, 0, hashlib.sha256()])
        g[0] += 1
        g[1] += not same
        g[2].update((new.get(name) or "").encode())
    for key, (n, nd, h) in groups.items():
        print("## %-24s %3d outputs, %d different, sha256 of the new hashes %s" % (key, n, nd, h.hexdigest()[:16]))
    print("# %d outputs compared, %d differences" % (len(set(old) | set(new)), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
