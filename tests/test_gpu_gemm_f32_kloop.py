"""The K loop of the persistent fp32 GEMM (csrc/gemm2.hip) may be rescheduled, never re-associated: every output of
gdx_linear_full with a forced tile must equal, bit for bit, what the build before the K-loop work produced on an MI355X.

The cases, the host-side operands (numpy.random.default_rng) and the call live in tools/make_golden_gemm_kloop.py, which
recorded tests/golden/gemm_f32_kloop_parent.json (SHA-256 values only) from the parent commit's library:
  tiles   (5,1,64,3) bias_res [RESP], (5,2,64,2) bias and bias_gelu, (5,3,64,2) bias, (9,1,32,4) res_rowmap,
          (8,1,32,4) bias, (1,1,64,3) and (2,1,64,3) bias -- three-, four- and two-stage rings, 1 to 15 accumulators
  M       1 row; one tile + 5 rows; (CUs + 1) tiles + 11 rows at N = one column tile, so a workgroup walks two tiles
  K       1 slab, NST slabs, NST + 1 slabs: ring fill, wrap and the first step after it
Values against float64 are tests/test_gpu_gemm_f32.py's job; this file only pins the bits.  Needs an MI355X.
"""
import importlib.util
import json
import os

import pytest
import torch

from gesturediffusion_amd import _lib

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_golden_gemm_kloop", os.path.join(REPO, "tools", "make_golden_gemm_kloop.py"))
mk = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mk)

with open(os.path.join(REPO, "tests", "golden", mk.FILE)) as _f:
    GOLDEN = json.load(_f)


def test_golden_lists_exactly_the_cases():
    assert sorted(GOLDEN["sha256"]) == sorted(c[0] for c in mk.cases(GOLDEN["cus"]))
    assert len(GOLDEN["sha256"]) == len(mk.TILES) * 9


@pytest.mark.parametrize("tile,ename", mk.TILES, ids=[f"{t[0]}x{t[1]}x{t[2]}x{t[3]}-{e}" for t, e in mk.TILES])
def test_bits_equal_the_parent_build(tile, ename):
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus == GOLDEN["cus"], f"the hashes were recorded on {GOLDEN['cus']} CUs (the large M depends on it), this device has {cus}"
    lib = _lib.load()
    ops = mk.operands(tile, ename, cus)
    bad = []
    for name, t, e, M, N, K in mk.cases(cus):
        if (t, e) != (tile, ename):
            continue
        la, h = mk.run_case(lib, ops, tile, ename, M, N, K)
        assert la[:5] == (1, *tile), f"{name}: launched {la}, not the forced tile"
        assert la[5] == int(ename == "bias_res"), f"{name}: launched {la}: RESP runs under bias_res only"
        print(f"{name}: M={M} N={N} K={K} sha256 {h[:16]} want {GOLDEN['sha256'][name][:16]}")
        if h != GOLDEN["sha256"][name]:
            bad.append(name)
    assert not bad, f"outputs differ from the parent build's bits: {bad}"
