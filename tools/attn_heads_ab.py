#!/usr/bin/env python3
"""Head widths 96 / 192 against their zero-padded stand-ins 128 / 256 (profiles/attention_head96_192.txt):
python tools/attn_heads_ab.py TAG [time|timeh|err|both]
time:  gdx_bench_attention at (B, S, H) = (64, 197, 4) and (41, 121, 4) in fp32 (attention.hip alone, and with attention3 where it has
       an instantiation), fp16 and bf16 (the forward's dispatch), native and padded arms alternating; timeh: the 16-bit modes only
err:   attention.hip against fp64 attention on the inputs of tests/test_gpu_heads.py, every width
TAG labels the lines; GDX_LIBGDX names another build of the library (one library per process)."""
import ctypes as C, os, statistics, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from gesturediffusion_amd import _lib

tag = sys.argv[1]
what = sys.argv[2] if len(sys.argv) > 2 else "both"
lib = _lib.load(); torch.cuda.init()
s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
print(f"== [{tag}] library {_lib.LIB_PATH}", flush=True)


def bench(B, S, H, d, ver, iters):
    us = C.c_float()
    _lib.check(lib.gdx_bench_attention(B, S, H, d, ver, iters, C.byref(us), s), lib)
    return us.value


if what in ("time", "timeh", "both"):
    REP, ITERS = 7, 1000
    print(f"-- us per launch, gdx_bench_attention: 3 warm-up + {ITERS} timed launches between two events; {REP} such windows per arm,"
          " native and padded arms alternating; min / median / max", flush=True)
    for mode, ver, hdt in (("fp32 v1 (attention.hip)", 1, None), ("fp32 v4 (attention3 at 128, attention.hip elsewhere)", 4, None),
                           ("fp16 (dispatch)", 3, 1), ("bf16 (dispatch)", 3, 2)):
        if what == "timeh" and hdt is None:
            continue
        if hdt is not None:
            _lib.check(lib.gdx_set_test_half_dtype(hdt), lib)
        for B, S in ((64, 197), (41, 121)):
            for nat, pad in ((96, 128), (192, 256)):
                t = {nat: [], pad: []}
                for hd in (nat, pad):
                    bench(B, S, 4, 4 * hd, ver, 50)              # warm both shapes
                for _ in range(REP):
                    for hd in (nat, pad):
                        t[hd].append(bench(B, S, 4, 4 * hd, ver, ITERS))
                f = lambda v: f"{min(v):7.2f} {statistics.median(v):7.2f} {max(v):7.2f}"
                r = statistics.median(t[nat]) / statistics.median(t[pad])
                print(f"  {mode:52s} B={B} S={S} H=4  hd {nat:3d}: {f(t[nat])}   hd {pad:3d}: {f(t[pad])}   native/padded {r:.3f}", flush=True)

if what in ("err", "both"):
    rel_err = lambda a, b: float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))
    print("-- fp32 attention.hip (version 1) against fp64 attention, inputs of tests/test_gpu_heads.py (Q x 3), rel err of max|ref|", flush=True)
    d0 = torch.device("cuda:0")
    SEQ = [1, 16, 31, 33, 65, 128, 197]
    for H, dm in [(4, 384), (4, 768), (2, 192), (4, 512), (4, 1024)]:
        errs = []
        for S in SEQ:
            B = 2 + (S + H) % 2
            hd = dm // H
            g = torch.Generator(device=d0).manual_seed(S + dm)
            qkv = torch.randn(B * S, 3 * dm, device=d0, generator=g)
            qkv[:, :dm] *= 3.0
            ctx = torch.full((B * S, dm), float("nan"), device=d0)
            _lib.check(lib.gdx_attention_f32(C.c_void_p(qkv.data_ptr()), C.c_void_p(ctx.data_ptr()), B, S, H, dm, 1, s), lib)
            r = qkv.double().view(B, S, 3, H, hd)
            q, k, v = (r[:, :, i].permute(0, 2, 1, 3) for i in range(3))
            p = torch.softmax(q @ k.transpose(-1, -2) / hd ** 0.5, dim=-1)
            ref = (p @ v).permute(0, 2, 1, 3).reshape(B * S, dm)
            errs.append(rel_err(ctx.cpu().double(), ref.cpu()))
        print(f"  [{tag}] H={H} d={dm} (hd {dm // H}): " + "  ".join(f"S={S}:{e:.2e}" for S, e in zip(SEQ, errs)) + f"   max {max(errs):.2e}", flush=True)
