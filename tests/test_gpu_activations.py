"""The activation of every kernel that has one, per element against float64: the three GELU implementations (csrc/gemm.hip
gelu_erf, csrc/gemm2.hip gelu_fast2, csrc/gemmh.hip gelu2 in fp16 and bf16) and the SiLU of small_linear_kernel
(csrc/boundary.hip).  Need an MI355X.

The operands of tests/activation_grid.py make output element (m, n) = act(x_m + b_n) with an exact pre-activation: 16 384
different values at spacing 1/512 over [-16, 16) (SiLU: [-104, 104)), a second launch with the same rows times 2^-6, and special
rows (+-0, +-2^-14, +-32768, 16; fp32 kernels also +-1e-30, +-1e30) that make M odd and the last row tile partial.  The other
GELU checks of the suite are aggregates relative to max|ref| over N(0, 1)-scale GEMM outputs: a wrong coefficient, a wrong
sign beyond the 16-bit clamp, a misplaced lane or a badly handled 1 + erf cancellation at |x| > 3 stays below them.

Per element, in bands of |x|: [0,1) [1,2) [2,3) [3,4.2) [4.2,6) [6,16] and the special rows beyond.  Bounds (none taken from
the kernels' output) with the worst value measured on an MI355X beside each constant below.  Shape checks no tolerance
gives: out <= 0 for x < 0 and >= 0 for x >= 0; out >= min(ref) - bound; out <= x for x > 0; finite on every input; the 16-bit
kernels' clamp value for x < -4.24.  `launched` must name the kernel and tile that was asked for.

gemm2.hip applies gelu_fast2 at two places of its epilogue.  Only the plain one can be launched: the general epilogue runs
when R, V or the token-row map is set, and gemm() gives EPI_GELU none of them (forward.hip clears R and V for it, and
gdx_linear_full refuses the combination, as no forward launches it).  What stands in for "both store paths" here is every
tile shape: the lane -> column map of the stores depends on NBW (1, 2, 3 blocks per wave), so all 21 G4_CONFIGS shapes run, at
N = 64 (the eight one-block shapes) and N = 384 (all), and must agree bit for bit -- as
test_gpu_gemm_f32.py::test_tile_and_batch_independence_bitwise states for GELU without exception.
"""
import ctypes as C

import pytest
import torch

import activation_grid as AG
from gesturediffusion_amd import _lib
from test_gpu_gemm_f32 import COST_MODEL, G4, GEMM1, GEMM2, g4_valid, run as run_linear_full
from test_gpu_half_blocks import BF16, F16, NAME, assert_rounded, assert_rows, bits, dev, run_linear_half, stream, vp

pytestmark = pytest.mark.gpu

# ---- bounds.  |err| against float64 GELU / SiLU of the exact pre-activation x.
# gemm2.hip: its stated erf error 1.5e-7 (halved by the 0.5 x in front) plus four fp32 roundings; an fp32 emulation of the
# formula on the CPU gives at worst 2.5e-7 |x|.
# measured err / |x| per band: 2.68e-7 [0,1) (near-zero launch; 2.11e-7 on the wide grid), 1.43e-7 [1,2), 1.48e-7 [2,3),
# 1.50e-7 [3,4.2), 9.7e-8 [4.2,6), 9.9e-10 [6,16], 0 beyond; absolute: 4.54e-7 at worst, in [3,4.2)
G2_REL = 1.5e-7 / 2 + 2.0 ** -21
# gemm.hip (libm erff): four fp32 roundings; emulation 8e-8 |x|.
# measured err / |x| per band: 8.5e-8, 1.05e-7, 9.5e-8, 8.9e-8, 9.7e-8, 9.9e-10, 0 beyond
G1_REL = 2.0 ** -21
# gemmh.hip C32: the kernel's stated 2.5e-6 below |x| = 4.2 and 1.1e-5 |x| above, plus 20 % for multiply-add contraction the
# emulation (2.499e-6, 1.058e-5 |x|) cannot predict.
# measured (fp16 = bf16: C32 does not depend on the element type here), absolute: 1.3e-7 [0,1), 6.2e-7 [1,2), 1.35e-6 [2,3),
# 2.461e-6 [3,4.2); relative to |x|: 1.053e-5 [4.2,6), 1.055e-5 [6,16] and at +-32768
GH_ABS, GH_REL, GH_SPLIT = 3e-6, 1.32e-5, 4.2
# gemmh.hip beyond the clamp (z = x / sqrt(2) < -3, x < -4.2427): the kernel returns x / 2 (1 + P(-3)) where P(-3) is its fit of
# erf(-3), stated within 1.2e-6: |out - x erfc(3) / 2| <= |x| (1.2e-6 / 2 + 2^-22 for the cancelling add), plus 20 %.
# measured |out - x erfc(3) / 2| / |x|: 5.55e-7 (24 336 elements of the wide launch)
CLAMP_X = 4.2427
CLAMP_VALUE = 0.5 * 2.209049699858544e-05                   # erfc(3) / 2
CLAMP_REL = 1.2 * (1.2e-6 / 2 + 2.0 ** -22)
# SiLU s / (1 + expf(-s)): four fp32 roundings assumed (no emulation behind it); the floor covers the outputs the kernel
# flushes to -0 once expf(-s) overflows (s < -88.7, |ref| <= 2.6e-37).
# measured err / |ref| where |ref| >= 1e-30: 9.6e-8 - 1.17e-7 per band on [-104, 104), 1.43e-7 near zero; where the output is
# flushed (2 561 elements), |err| <= 1.55e-37
SILU_REL, SILU_FLOOR = 2.0 ** -21, 1e-36


def shape_checks(got, pre, ref, bound, what):
    """got, pre, ref, bound: float64 [M][N].  The per-element bound and the checks a tolerance does not give."""
    assert bool(torch.isfinite(got).all()), f"{what}: a non-finite output"
    err = (got - ref).abs()
    bad = err > bound
    if bool(bad.any()):
        i = int(torch.argmax((err - bound).flatten()))
        raise AssertionError(f"{what}: {int(bad.sum())} elements past the bound; worst at x = {float(pre.flatten()[i])!r}: got "
                             f"{float(got.flatten()[i])!r}, ref {float(ref.flatten()[i])!r}, bound {float(bound.flatten()[i]):.3e}")
    neg, pos = pre < 0, pre > 0
    assert bool((got[neg] <= 0).all()), f"{what}: a positive output for a negative input"
    assert bool((got[~neg] >= 0).all()), f"{what}: a negative output for a non-negative input"
    assert bool((got >= ref.min() - bound).all()), f"{what}: an output below the activation's minimum"
    assert bool((got[pos] <= pre[pos]).all()), f"{what}: an output above x"
    return err


def report(tag, err, pre, rel_to=None, unit="|err|"):
    print(f"\n[{tag}] worst {unit} per band of |x|: " + AG.fmt(AG.worst_per_band(err, pre, rel_to)))


# ---------------------------------------------------------------------------------------------------------------------
# fp32: gemm.hip and every tile of gemm2.hip
@pytest.mark.parametrize("grid", ["wide", "near"])
def test_gelu_f32_kernels_per_element(grid):
    """gemm.hip (kernel = 2) and gemm2.hip under every G4_CONFIGS shape g4_valid admits (forced, kernel = 1) and the
    dispatcher's choice, at N = 64 and N = 384 (b_n repeated six times), K = 64, M = 265 (no tile height divides it: 16, 32,
    64, 80, 96, 128, 144).  gemm2.hip: every shape gives the same bits, and the six copies of a column are bit-equal."""
    lib = _lib.load()
    d = dev()
    K = 64
    first2 = None
    for tile_n in (1, 6):
        A, W, b, pre = AG.operands("f32", grid, d, K=K, tile_n=tile_n)
        M, N = pre.shape
        ref = AG.gelu64(pre)
        assert M == 265
        runs = [(2, COST_MODEL)] if tile_n == 1 else []
        runs += [(1, t) for t in G4 if g4_valid(t, N, K)] + [(1, COST_MODEL), (0, COST_MODEL)]
        assert len(runs) == (1 + 8 + 2 if tile_n == 1 else 21 + 2)
        for kernel, tile in runs:
            out = torch.full((M, N), float("nan"), device=d)
            la = run_linear_full(lib, A, W, b, None, N, None, N, out, M, N, K, 1, 0, 1, kernel, tile)
            what = f"gelu {grid} N={N} kernel={kernel} tile={tile[:3]} launched={la}"
            if kernel == 2:
                assert la == (GEMM1, 0, 0, 0, 0, 0), f"{what}: gemm.hip was asked for"
            else:
                assert la[0] == GEMM2 and la[5] == 0 and g4_valid(la[1:5], N, K), what
                assert tile == COST_MODEL or la[1:5] == tile, f"{what}: the forced tile did not run"
            got = out.double()
            bound = pre.abs() * (G1_REL if kernel == 2 else G2_REL)
            err = shape_checks(got, pre, ref, bound, what)
            if kernel == 2:
                report(f"gemm.hip gelu_erf {grid}", err, pre, pre.abs(), "|err| / |x|")
                continue
            if first2 is None:
                first2 = out
                report(f"gemm2.hip gelu_fast2 {grid}", err, pre, pre.abs(), "|err| / |x|")
                report(f"gemm2.hip gelu_fast2 {grid}", err, pre)
            for c in range(tile_n):
                assert torch.equal(bits(out[:, c * AG.N:(c + 1) * AG.N]), bits(first2)), \
                    f"{what}: bits of column copy {c} differ from the first gemm2.hip launch"


# ---------------------------------------------------------------------------------------------------------------------
# 16-bit: gemmh_kernel tiles and the eight-wave gemmh8b_kernel
# (16, 4) is gemmh8b_kernel (256 x 256 tiles): it needs N % 256 == 0 and K >= 256, so N = 256 (b_n repeated four times: the
# smallest width it takes) and K = 256 (columns 1 .. 255 of A and W zero: still no summation error).  (8, 4) and (4, 4) are
# gemmh_kernel's 256-column tiles, (8, 2) its 128-column one, (4, 1) its 64-column one (the f16x4 store); (0, 0) the cost model.
GH_WIDE_TILES = [(16, 4), (8, 4), (4, 4), (8, 2), (4, 1), (0, 0)]
GH_NARROW_TILES = [(4, 1), (2, 1), (0, 0)]                  # the issue's own shape: N = 64, K = 64


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("grid", ["wide", "near"])
def test_gelu_half_kernels_per_element(grid, dtype):
    """gelu2 through gemmh8b_kernel (16, 4) and gemmh_kernel (8, 4), (4, 4), (8, 2), (4, 1), (2, 1) and the cost model's choice;
    M = 263.  C32 per element; C16 = C32 rounded; every tile, both widths and every column copy give the same C32 and C16
    bits; beyond the clamp (x < -4.2427) the output is x erfc(3) / 2 (about 1.1e-5 x, not 0: documented and accepted)."""
    lib = _lib.load()
    d = dev()
    first = None
    for K, tile_n, tiles in ((256, 4, GH_WIDE_TILES), (64, 1, GH_NARROW_TILES)):
        A, W, b, pre = AG.operands("half", grid, d, K=K, tile_n=tile_n)
        M, N = pre.shape
        assert M == 263
        ref = AG.gelu64(pre)
        written = torch.zeros(M + 3, dtype=torch.bool, device=d)
        written[:M] = True
        for tile in tiles:
            c32 = torch.full((M + 3, N), float("nan"), device=d)
            c16 = torch.full((M + 3, N), float("nan"), device=d)
            la = run_linear_half(lib, A, W, b, None, N, None, N, c32, c16, M, N, K, 1, 0, 1, dtype, tile)
            what = f"{NAME[dtype]} gelu {grid} N={N} K={K} tile={tile} launched={la}"
            if tile != (0, 0):
                assert la == (tile[0], tile[1], 0, 0, 0), f"{what}: the forced tile did not run"
            assert_rows(c32, written, what + " C32")
            assert_rows(c16, written, what + " C16")
            assert_rounded(c16[:M], c32[:M], dtype, what)
            if first is None:
                first = (c32[:M, :AG.N], c16[:M, :AG.N])
                got = c32[:M].double()
                a = pre.abs()
                bound = torch.where(a < GH_SPLIT, torch.full_like(a, GH_ABS), GH_REL * a)
                err = shape_checks(got, pre, ref, bound, what)
                report(f"gemmh.hip gelu2 {NAME[dtype]} {grid}", err, pre)
                report(f"gemmh.hip gelu2 {NAME[dtype]} {grid}", err, pre, a, "|err| / |x|")
                cl = pre < -CLAMP_X
                if grid == "wide":
                    assert int(cl.sum()) > 5000 * tile_n
                dev_cl = (got[cl] - pre[cl] * CLAMP_VALUE).abs() / pre[cl].abs()
                if bool(cl.any()):
                    print(f"[gemmh.hip gelu2 {NAME[dtype]} {grid}] clamp: worst |out - x erfc(3) / 2| / |x| {float(dev_cl.max()):.3e} "
                          f"over {int(cl.sum())} elements (bound {CLAMP_REL:.3e})")
                    assert bool((dev_cl <= CLAMP_REL).all()), f"{what}: not the documented clamp value below -{CLAMP_X}"
                    assert bool((got[cl] < 0).all()), f"{what}: the clamp value of a negative input is not negative"
            for c in range(tile_n):
                sl = slice(c * AG.N, (c + 1) * AG.N)
                assert torch.equal(bits(c32[:M, sl]), bits(first[0])), f"{what}: C32 bits of column copy {c} differ from tile (16, 4)"
                assert torch.equal(bits(c16[:M, sl]), bits(first[1])), f"{what}: C16 bits of column copy {c} differ from tile (16, 4)"


# ---------------------------------------------------------------------------------------------------------------------
# SiLU
@pytest.mark.parametrize("grid", ["silu", "near"])
def test_silu_small_linear_per_element(grid):
    """small_linear_kernel with act = 1 at K = 1 (one term: the argument is exact), M = 265 (67 blocks of four rows, the last
    with one), N = 64: x over [-104, 104) -- past s = -88.7, where expf(-s) overflows and the kernel returns -0 for a true
    value of at most 2.6e-37 -- and the near-zero rows; special rows +-0, +-2^-14, +-32768, +-1e30 / +-1e-30."""
    lib = _lib.load()
    d = dev()
    A, W, b, pre = AG.operands("f32", grid, d, K=1)
    M, N = pre.shape
    assert M == 265
    out = torch.full((M + 2, N), float("nan"), device=d)
    _lib.check(lib.gdx_small_linear(vp(A), 1, vp(W), 1, vp(b), vp(out), M + 2, N, M, N, 1, 1, stream()), lib)
    assert bool(torch.isnan(out[M:]).all()), "rows past M were written"
    got, ref = out[:M].double(), AG.silu64(pre)
    bound = SILU_REL * ref.abs() + SILU_FLOOR
    err = shape_checks(got, pre, ref, bound, f"silu {grid}")
    normal = ref.abs() >= 1e-30
    report(f"small_linear SiLU {grid}", torch.where(normal, err, torch.zeros_like(err)), pre, ref.abs(), "|err| / |ref| (|ref| >= 1e-30)")
    flushed = ~normal & (pre != 0)
    if bool(flushed.any()):
        print(f"[small_linear SiLU {grid}] {int(flushed.sum())} outputs with |ref| < 1e-30: worst |err| {float(err[flushed].max()):.3e} "
              f"(floor {SILU_FLOOR:.0e})")
