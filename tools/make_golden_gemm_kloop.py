#!/usr/bin/env python3
"""Record tests/golden/gemm_f32_kloop_parent.json: SHA-256 of the fp32 GEMM outputs of ONE build of libgdx.so.

The K loop of csrc/gemm2.hip may be rescheduled freely as long as every output element keeps its k-slab by k-slab fmaf
order, i.e. as long as the bits do not move.  This tool runs the cases of tests/test_gpu_gemm_f32_kloop.py (it is that
test's only statement of them: the test imports CASES / operands / run_case from here) on the library that GDX_LIBGDX
names -- the build of the commit BEFORE a K-loop change -- and writes one hash per case.  Needs an MI355X: the large M
of a case depends on the CU count, which is recorded next to the hashes.

Cases, per (tile, epilogue):
  M   1 row;  one tile + 5 rows;  (CUs + 1) tiles + 11 rows at N = one column tile (a workgroup walks two tiles);
  K   1 slab, NST slabs, NST + 1 slabs of the tile's depth (ring fill, wrap, the step after the wrap).
Inputs come from numpy.random.default_rng on the host, so they do not depend on the library or the torch version.

Usage:  GDX_LIBGDX=<parent's libgdx.so> python tools/make_golden_gemm_kloop.py [--out tests/golden]
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

FILE = "gemm_f32_kloop_parent.json"
# (mb, nbw, bk, nst) of gemm2.hip G4_CONFIGS, epilogue: (bias, gelu, R, rowmap) as forward_core launches them
TILES = [((5, 1, 64, 3), "bias_res"), ((5, 2, 64, 2), "bias"), ((5, 2, 64, 2), "bias_gelu"), ((5, 3, 64, 2), "bias"),
         ((9, 1, 32, 4), "res_rowmap"), ((8, 1, 32, 4), "bias"), ((1, 1, 64, 3), "bias"), ((2, 1, 64, 3), "bias")]
EPILOGUES = {"bias": (1, 0, 0, 0), "bias_gelu": (1, 1, 0, 0), "bias_res": (1, 0, 1, 0), "res_rowmap": (0, 0, 1, 1)}
T_ROWMAP = 17                   # frames per sample of the row-mapped case: sample boundaries inside 16-row blocks
M_CLASSES = ("one_row", "tile_plus_5", "cus_plus_1_tiles_plus_11")
K_CLASSES = ("one_slab", "nst_slabs", "nst_plus_1_slabs")


def rows_of(tile, mclass, cus):
    bm = 16 * tile[0]
    return {"one_row": 1, "tile_plus_5": bm + 5, "cus_plus_1_tiles_plus_11": (cus + 1) * bm + 11}[mclass]


def depth_of(tile, kclass):
    return tile[2] * {"one_slab": 1, "nst_slabs": tile[3], "nst_plus_1_slabs": tile[3] + 1}[kclass]


def cases(cus):
    """[(case id, tile, epilogue name, M, N, K)] -- N is one column tile."""
    out = []
    for tile, ename in TILES:
        for mc in M_CLASSES:
            for kc in K_CLASSES:
                name = f"{tile[0]}x{tile[1]}x{tile[2]}x{tile[3]}-{ename}-{mc}-{kc}"
                out.append((name, tile, ename, rows_of(tile, mc, cus), 64 * tile[1], depth_of(tile, kc)))
    return out


def operands(tile, ename, cus):
    """Host operands of one (tile, epilogue), sized for its largest case; a case uses the leading rows / columns."""
    seed = [1009, *tile, sorted(EPILOGUES).index(ename)]
    rng = np.random.default_rng(seed)
    Mmax, N, Kmax = rows_of(tile, M_CLASSES[-1], cus), 64 * tile[1], depth_of(tile, K_CLASSES[-1])
    rmax = Mmax + (Mmax - 1) // T_ROWMAP + 1
    f = lambda *s: rng.standard_normal(s, dtype=np.float32)                       # noqa: E731
    return {"A": f(Mmax, Kmax), "W": f(N, Kmax) / np.float32(Kmax ** 0.5), "bias": f(N), "R": f(rmax, N + 4)}


def run_case(lib, ops, tile, ename, M, N, K):
    """One gdx_linear_full call with the tile forced.  Returns (launched, SHA-256 of the rows the epilogue stores)."""
    import torch
    from gesturediffusion_amd import _lib
    ub, gelu, uR, rowmap = EPILOGUES[ename]
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)              # noqa: E731
    vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None            # noqa: E731
    rows_out = M + (M - 1) // T_ROWMAP + 1 if rowmap else M
    A, W = up(ops["A"][:M, :K]), up(ops["W"][:, :K])
    bias = up(ops["bias"]) if ub else None
    R = up(ops["R"][:rows_out]) if uR else None
    out = torch.zeros(rows_out, N, device=dev)                                    # token-0 rows of a row map stay zero
    la = (C.c_int32 * 6)()
    _lib.check(lib.gdx_linear_full(vp(A), vp(W), vp(bias), vp(R), N + 4, None, 0, vp(out), rows_out, M, N, K, T_ROWMAP,
                                   rowmap, gelu, 1, tile[0], tile[1], tile[2], la,
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)), lib)
    torch.cuda.synchronize()
    return tuple(la), hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()


def main():
    import torch
    from gesturediffusion_amd import _lib
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    args = ap.parse_args()
    lib = _lib.load()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    hashes, ops_of = {}, {}
    for name, tile, ename, M, N, K in cases(cus):
        key = (tile, ename)
        if key not in ops_of:
            ops_of.clear()                                                        # one operand set alive at a time
            ops_of[key] = operands(tile, ename, cus)
        la, h = run_case(lib, ops_of[key], tile, ename, M, N, K)
        assert la[:5] == (1, *tile), f"{name}: launched {la}, not the forced tile"
        hashes[name] = h
    path = os.path.join(args.out, FILE)
    with open(path, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "cus": cus, "sha256": hashes}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(path, len(hashes), "cases, library", _lib.LIB_PATH)


if __name__ == "__main__":
    main()
