"""Kernel-level tests of the 16-bit encoder self-attention (csrc/attentionh.hip, fp16 and bf16 builds) through the test entry
point gdx_attention_half, which forces one kernel -- attentionh8_kernel (h8: 8 waves x 1 query block), attentionh8q_kernel (h8q:
8 x 2) or attentionh8p_kernel (h8p: persistent, one workgroup walking items) -- and reports what ran.  Need an MI355X.

Every case runs in fp16 and bf16 against a float64 softmax attention on the same rounded q / k / v, for every kernel that is
instantiated for its head dim (h8q / h8p: 64, 128, 256).  Besides the max-normalised bound of the whole-output tests, every
element is held to

    |ctx - ref| <= A u w + u |ref| + T max|v|,        w = sum_j p_j |v_j| / sum_j p_j   (float64, per row, head, column)

u = half an ulp (EPS_REL): the 16-bit rounding of the probabilities (A u w) and of the output (u |ref|); T covers fp16's
underflow of p < 2^-24 and fp32 round-off.  Structured probes (uniform, peaked, rescale ramps) check what random data cannot,
and the edge tests hold every kernel to per-sample bit-independence from its neighbours in the batch and from the pad rows.
h8, h8q and h8p run the same arithmetic per query block (same tile order, same online-softmax state), so all three must give
identical bits.
"""
import ctypes as C
import importlib.util
import math
import os

import pytest
import torch

from gesturediffusion_amd import _lib

pytestmark = pytest.mark.gpu

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
F16, BF16 = 1, 2                               # GDX_DTYPE_*
TDT = {F16: torch.float16, BF16: torch.bfloat16}
NAME = {F16: "fp16", BF16: "bf16"}
EPS_REL = {F16: 2.0 ** -11, BF16: 2.0 ** -8}    # half an ulp, relative, of a normal 16-bit number
TINY = {F16: 2.0 ** -25, BF16: 0.0}             # half the fp16 subnormal step
H8, H8Q, H8P = 1, 2, 3
KNAME = {H8: "h8", H8Q: "h8q", H8P: "h8p"}
# existing whole-output bounds (tests/test_gpu_parity.py, tests/test_gpu_round2.py), kept beside the per-element one
TOL_MAX = {F16: 2e-3, BF16: 1.6e-2}
# per-element bound, from the worst values measured on an MI355X over every case of this file (the "[attnh-measure]" lines):
#   A (with T = 0) fp16 0.85, bf16 0.78 -- except fp16's "first" ramp, 3.9, where the other keys' p underflow: that is T's part;
#   T (with A = 1) fp16 1.0e-7 of max|v| (that ramp), bf16 0 (measured nothing; kept as fp32 round-off room)
A_P = {F16: 2.0, BF16: 2.0}
T_ABS = {F16: 4e-7, BF16: 1e-7}
PAD = 48                                        # readable rows past B*S (a workgroup reads < S + 32 rows from its base)
JUNK = 3.0e4                                    # large finite pad values (fp16 max 65 504)


def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


def vp(t):
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(t):
    return t.contiguous().view(torch.int32)


def kernels(hd):
    return [H8] if hd == 32 else [H8, H8Q, H8P]


def run(qkv, B, S, H, d, dtype, kernel, grid=0):
    """One gdx_attention_half call on qkv (fp32 device [qkv_rows][3d], qkv_rows >= B*S) into a NaN-filled ctx with three sentinel
    rows past B*S.  Every row below B*S must come back finite, every sentinel row NaN, and the report must name the forced
    kernel / grid.  Returns the B*S rows and the report (kernel, grid, items)."""
    lib = _lib.load()
    rows = B * S
    ctx = torch.full((rows + 3, d), float("nan"), device=qkv.device)
    rep = (C.c_int32 * 3)()
    _lib.check(lib.gdx_attention_half(vp(qkv), qkv.shape[0], vp(ctx), ctx.shape[0], B, S, H, d, dtype, kernel, grid, rep,
                                      stream()), lib)
    what = f"{NAME[dtype]} {KNAME.get(kernel, 'dispatch')} B={B} S={S} H={H} d={d} grid={grid}"
    if kernel:
        assert rep[0] == kernel, f"{what}: kernel {rep[0]} ran"
    if grid:
        assert rep[1] == grid, f"{what}: grid {rep[1]}"
    assert bool(torch.isfinite(ctx[:rows]).all()), f"{what}: a row below B*S holds a non-finite value"
    assert bool(torch.isnan(ctx[rows:]).all()), f"{what}: a sentinel row past B*S was written"
    return ctx[:rows], tuple(rep)


def reference(qkv, B, S, H, d, dtype):
    """float64 softmax attention on the dtype-rounded q / k / v: (ref, w) as [B*S][d]."""
    hd = d // H
    r = qkv[:B * S].to(TDT[dtype]).double().view(B, S, 3, H, hd)
    q, k, v = (r[:, :, i].transpose(1, 2) for i in range(3))
    p = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(hd), dim=-1)
    ref = (p @ v).transpose(1, 2).reshape(B * S, d)
    w = (p @ v.abs()).transpose(1, 2).reshape(B * S, d)
    return ref, w, float(v.abs().max())


def check(got, refw, dtype, what):
    """Per-element bound and the max-normalised one; returns the measured (A, T) of this output for the log."""
    ref, w, vmax = refw
    u = EPS_REL[dtype]
    err = (got.double() - ref).abs()
    lim = A_P[dtype] * u * w + u * ref.abs() + T_ABS[dtype] * vmax
    bad = err > lim
    if bool(bad.any()):
        i = int(bad.view(-1).nonzero()[0])
        raise AssertionError(f"{what}: |ctx - ref| {float(err.view(-1)[i]):.3e} > bound {float(lim.view(-1)[i]):.3e} at element {i} "
                             f"(ref {float(ref.view(-1)[i]):.4e}, w {float(w.view(-1)[i]):.3e}; {int(bad.sum())} elements)")
    m = float(ref.abs().max())
    if m > 0:
        e = float(err.max()) / m
        assert e < TOL_MAX[dtype], f"{what}: rel err {e:.2e}"
    a_meas = float(((err - u * ref.abs()) / (u * w).clamp_min(1e-30)).max())
    t_meas = float((err - u * w - u * ref.abs()).clamp_min(0).max()) / max(vmax, 1e-30)
    print(f"[attnh-measure] {what}: A {a_meas:.3f} T {t_meas:.2e}")
    return a_meas, t_meas


def random_qkv(B, S, d, seed, rows=None, qscale=2.0):
    g = torch.Generator(device=dev()).manual_seed(seed)
    qkv = torch.randn(rows or B * S, 3 * d, device=dev(), generator=g)
    qkv[:, :d] *= qscale                         # sharper softmax than unit-variance scores
    if rows:
        qkv[B * S:] = 0
    return qkv


def run_all(qkv, B, S, H, d, dtype, what, refw=None, grids=()):
    """Every instantiated kernel: each within the bounds, all three bit-identical (h8p also at each grid of `grids`)."""
    refw = refw or reference(qkv, B, S, H, d, dtype)
    outs = {}
    for k in kernels(d // H):
        got, _ = run(qkv, B, S, H, d, dtype, k)
        check(got, refw, dtype, f"{what} {KNAME[k]}")
        outs[k] = bits(got)
    for k in outs:
        assert torch.equal(outs[k], outs[H8]), f"{what}: {KNAME[k]} and h8 differ in bits"
    for gr in grids:
        got, _ = run(qkv, B, S, H, d, dtype, H8P, gr)
        assert torch.equal(bits(got), outs[H8Q]), f"{what}: h8p at grid {gr} and h8q differ in bits"
    return outs


# ---------------------------------------------------------------------------------------------------------------------
# geometry: query-block counts 1..17 in one chunk (S = 16k - 15: a last block of one row, 16k - 3: of 13 rows; key-tile tails
# of 1, 13 and 31 keys and exact multiples of 32), S = 1, and several chunks (h8q / h8p: 2 chunks at 257 .. 300 -- 17 to 19
# blocks --, 3 at 521, 4 at 769; h8: chunks of 8 blocks, 2 to 7 of them)
SWEEP_S = sorted({16 * k - 15 for k in range(1, 18)} | {16 * k - 3 for k in range(1, 18)} | {257, 300, 521, 769})


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("hd", [32, 64, 128, 256])
def test_attention_half_geometry_sweep(hd, dtype):
    """Every kernel at every S of SWEEP_S (B = 2, H = 2): per-element bound, NaN sentinels, all kernels bit-identical."""
    B, H = 2, 2
    d = H * hd
    for S in SWEEP_S:
        qkv = random_qkv(B, S, d, seed=S * 10 + hd + dtype)
        run_all(qkv, B, S, H, d, dtype, f"{NAME[dtype]} sweep hd={hd} S={S}")


# ---------------------------------------------------------------------------------------------------------------------
# persistent item walk: (B, H, S, hd) -> items (sample, head, chunk): 12 (two chunks of 9 / 10 blocks), 18 (three chunks),
# 8 (four chunks of 12 / 13 blocks), 5 and 4 (one chunk); grids 1..13 chain 1 to 18 items per workgroup across samples,
# heads and chunks of different sizes, with grids that are not a multiple of the 8 XCDs and grids above the item count
WALK = [(3, 2, 300, 64), (2, 3, 521, 128), (1, 2, 769, 256), (5, 1, 45, 64), (2, 2, 13, 128)]
WALK_GRIDS = [1, 3, 7, 8, 9, 13, 21, 64]


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("B,H,S,hd", WALK)
def test_attention_half_persistent_item_walk(B, H, S, hd, dtype):
    """h8p forced at grids 1, 3, 7, 8, 9, 13, 21 and 64 gives h8q's bits at every grid (attentionh8p_kernel's comment: per item
    the arithmetic of attentionh8q_kernel, statement for statement), and h8q is within the bounds; h8 gives the same bits."""
    d = H * hd
    qkv = random_qkv(B, S, d, seed=B * 1000 + S + hd + dtype, rows=B * S + PAD)
    nqb = (S + 15) // 16
    nitems = B * H * ((nqb + 15) // 16)
    _, rep = run(qkv, B, S, H, d, dtype, H8P)
    assert rep[2] == nitems and rep[1] == min(nitems, torch.cuda.get_device_properties(0).multi_processor_count), rep
    run_all(qkv, B, S, H, d, dtype, f"{NAME[dtype]} walk B={B} H={H} S={S} hd={hd}", grids=WALK_GRIDS)


# ---------------------------------------------------------------------------------------------------------------------
# structured probes
PROBE_S = [1, 29, 64, 77, 197, 300, 769]


def junk_pad(qkv, rows, g):
    """Large finite values (+-JUNK) in every column of the readable rows past B*S."""
    n = qkv.shape[0] - rows
    qkv[rows:] = (torch.rand(n, qkv.shape[1], device=qkv.device, generator=g) * 2 - 1) * JUNK


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("hd", [32, 64, 128, 256])
def test_attention_half_uniform_probe(hd, dtype):
    """Q = 0: every valid key has p = 1 and l = S, so the output is the mean of V over exactly the sample's S keys.  V holds
    nonzero integers in [-8, 8] (exact in both types, exact fp32 sums), different per sample, head, key and column; K is
    random and the pad rows hold +-3e4 junk.  The output must be within one 16-bit rounding of the exact mean (plus the fp32
    1/l product): a key counted twice or missed, or a key of another sample, head, column or of the pad, moves the mean by
    at least 1/S of a value whose mean is mostly << 1 -- many roundings."""
    B, H = 3, 2
    d = H * hd
    for S in PROBE_S:
        g = torch.Generator(device=dev()).manual_seed(S + hd)
        rows = B * S
        qkv = torch.zeros(rows + PAD, 3 * d, device=dev())
        qkv[:rows, d:2 * d] = torch.randn(rows, d, device=dev(), generator=g)
        mag = torch.randint(1, 9, (rows, d), device=dev(), generator=g).float()
        sgn = torch.randint(0, 2, (rows, d), device=dev(), generator=g).float() * 2 - 1
        qkv[:rows, 2 * d:] = mag * sgn
        junk_pad(qkv, rows, g)
        mean = qkv[:rows, 2 * d:].double().view(B, S, d).mean(dim=1, keepdim=True).expand(B, S, d).reshape(rows, d)
        outs = {}
        for k in kernels(hd):
            got, _ = run(qkv, B, S, H, d, dtype, k)
            what = f"{NAME[dtype]} uniform probe hd={hd} S={S} {KNAME[k]}"
            ok = within_one_rounding(got, mean, dtype, mean.abs() * 2.0 ** -22)
            assert ok, f"{what}: not within one rounding of the mean of V (max |err| {float((got.double() - mean).abs().max()):.3e})"
            outs[k] = bits(got)
        for k in outs:
            assert torch.equal(outs[k], outs[H8]), f"{NAME[dtype]} uniform probe hd={hd} S={S}: {KNAME[k]} and h8 differ"


def within_one_rounding(c16, ref, dtype, abs_tol):
    """|c16 - ref| <= half an ulp of ref + abs_tol: one rounding of a value that is abs_tol from ref."""
    err = (c16.double() - ref).abs()
    lim = ref.abs() * EPS_REL[dtype] * 1.0001 + abs_tol + TINY[dtype]
    return bool((err <= lim).all())


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("hd", [32, 64, 128, 256])
def test_attention_half_peaked_probe(hd, dtype):
    """K rows are random +-1 vectors and query i of (sample b, head h) is 12 K[t] for its target key t = (a i + b + h) mod S,
    a prime that does not divide S: the targets of a (sample, head) are a permutation of its keys -- key 0, key S - 1, every
    key of the last partial tile and every position class of the permuted k-slot order (k slot 8g + j <-> key 16 (j >> 2) +
    4g + (j & 3)).  The target's score exceeds every other by ~12 (sqrt(hd) - 4), so the output is essentially V[t]: a
    mis-paired key slot or swizzle row returns another key's V."""
    B, H = 2, 2
    d = H * hd
    for S in [1, 13, 61, 96, 197, 521]:
        g = torch.Generator(device=dev()).manual_seed(S * 3 + hd)
        a = next(p for p in (7, 11, 13, 17) if S % p)
        K = (torch.randint(0, 2, (B, S, H, hd), device=dev(), generator=g).float() * 2 - 1)
        i = torch.arange(S, device=dev())
        Q = torch.empty_like(K)
        for b in range(B):
            for h in range(H):
                Q[b, :, h] = 12.0 * K[b, (a * i + b + h) % S, h]
        V = torch.randn(B, S, H, hd, device=dev(), generator=g)
        qkv = torch.cat([Q.reshape(B * S, d), K.reshape(B * S, d), V.reshape(B * S, d)], dim=1)
        run_all(qkv, B, S, H, d, dtype, f"{NAME[dtype]} peaked probe hd={hd} S={S}")


def ramp_qkv(B, S, H, hd, L, seed):
    """Scores (log2 domain, as the kernels see them) L(key) + small noise: Q[:, 0] = alpha in {4, 3.5, 3, 2.5} by query (so the
    lanes of a block cross the rescale threshold at different tiles), K[:, 0] = L / (4 c), c = log2(e) / sqrt(hd); the other
    dimensions hold noise of 0.25."""
    d = H * hd
    g = torch.Generator(device=dev()).manual_seed(seed)
    c = math.log2(math.e) / math.sqrt(hd)
    Q = torch.randn(B, S, H, hd, device=dev(), generator=g) * 0.25
    K = torch.randn(B, S, H, hd, device=dev(), generator=g) * 0.25
    Q[..., 0] = 4.0 - 0.5 * (torch.arange(S, device=dev()) % 4).float().view(1, S, 1)
    K[..., 0] = (L(torch.arange(S, device=dev()).double()).float() / (4.0 * c)).view(1, S, 1)
    V = torch.randn(B, S, H, hd, device=dev(), generator=g)
    return torch.cat([Q.reshape(B * S, d), K.reshape(B * S, d), V.reshape(B * S, d)], dim=1)


RAMPS = {
    "over": lambda j: 9.0 * torch.floor(j / 32) + 0.5 * (j % 32) / 32,        # every tile raises the maximum by > 8
    "under": lambda j: 7.875 * torch.floor(j / 32),                          # by just under 8: p up to ~2^7.9, then a rescale
    "first": lambda j: torch.where(j == 0, 30.0, 0.0) + 0 * j,              # the maximum in key 0
    "last": lambda j: torch.where(j == j.max(), 30.0, 0.0) + 0 * j,         # the maximum in key S - 1 (the partial last tile)
}


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("hd", [32, 64, 128, 256])
@pytest.mark.parametrize("ramp", sorted(RAMPS))
def test_attention_half_rescale_probes(ramp, hd, dtype):
    """The deferred-max rescale (threshold 8 in the log2 domain) under score ramps: forced at every tile, just avoided with p
    approaching 2^8, and a single maximum in the first or in the last, partial tile.  Per-element bound, all kernels
    bit-identical."""
    B, H = 2, 2
    d = H * hd
    for S in [45, 200, 521]:
        qkv = ramp_qkv(B, S, H, hd, RAMPS[ramp], seed=S + hd + len(ramp))
        run_all(qkv, B, S, H, d, dtype, f"{NAME[dtype]} ramp {ramp} hd={hd} S={S}")


# ---------------------------------------------------------------------------------------------------------------------
# edges and independence: S with a partial last query block (45: 13 rows, 197: 5, 300: 12, 29: 13, 521: 9)
IND = [(3, 45, 2, 64), (3, 197, 2, 128), (3, 300, 1, 256), (3, 29, 2, 32), (3, 521, 1, 128), (2, 197, 1, 256)]


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("B,S,H,hd", IND)
def test_attention_half_sample_independence(B, S, H, hd, dtype):
    """With each kernel forced, every sample's rows are bit-equal (a) with +-3e4 junk instead of zeros in the readable pad rows
    past B*S (q, k and v), (b) to a B = 1 call on that sample alone (nothing readable past it), and (c) with every other
    sample replaced by different data with 40x larger queries.  A query row past S in a partial last block is never stored,
    but it takes part in its block's rescale vote: if it came from the next sample or the pad (h8q / h8p before the Q rows
    were clamped to S - 1, as h8 does) it could move a valid query's reference maximum and change its bits."""
    d = H * hd
    rows = B * S
    g = torch.Generator(device=dev()).manual_seed(S * 7 + hd + dtype)
    qkv = random_qkv(B, S, d, seed=S + 5 * hd + dtype, rows=rows + PAD)
    loud = random_qkv(B, S, d, seed=S + 5 * hd + dtype + 1, qscale=80.0)
    refw = reference(qkv, B, S, H, d, dtype)
    for k in kernels(hd):
        what = f"{NAME[dtype]} {KNAME[k]} B={B} S={S} H={H} hd={hd}"
        base, _ = run(qkv, B, S, H, d, dtype, k)
        check(base, refw, dtype, what)
        base = bits(base)
        qj = qkv.clone()
        junk_pad(qj, rows, g)
        got, _ = run(qj, B, S, H, d, dtype, k)
        assert torch.equal(bits(got), base), f"{what}: the junk in the pad rows changed the output"
        for b in range(B):
            sl = slice(b * S, (b + 1) * S)
            alone, _ = run(qkv[sl].contiguous(), 1, S, H, d, dtype, k)
            assert torch.equal(bits(alone), base[sl]), f"{what}: sample {b} alone differs from sample {b} in the batch"
            mix = loud.clone()
            mix[sl] = qkv[sl]
            got, _ = run(mix, B, S, H, d, dtype, k)
            assert torch.equal(bits(got)[sl], base[sl]), f"{what}: sample {b} changes with its neighbours"


# ---------------------------------------------------------------------------------------------------------------------
# dispatch at the bench presets' attention shapes
def preset_shapes():
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(REPO, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    out = []
    for name, p in sorted(bench.PRESETS.items()):
        B = p["sub"] or p["batch"]
        out.append((name, B * (2 if p["cfg"] else 1), p["T"] + 1, 4, p["d"]))
    p = bench.PRESETS["5"]
    out.append(("5 (one rank of 8)", p["batch"] // 8, p["T"] + 1, 4, p["d"]))
    return out


def expected_dispatch(B, S, H, d, num_cus):
    """The documented rule (launch_attentionh_kernel): persistent once every CU has two items, 8 x 2 blocks from 128 items,
    else 8 x 1 block; items counted in chunks of 16 query blocks."""
    hd = d // H
    nqb = (S + 15) // 16
    items = B * H * ((nqb + 15) // 16)
    if hd >= 64 and items >= 2 * num_cus:
        return H8P, min(items, num_cus), items
    if hd >= 64 and items >= 128:
        return H8Q, items, items
    n8 = B * H * ((nqb + 7) // 8)
    return H8, n8, n8


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_attention_half_dispatch_at_bench_shapes(dtype):
    """kernel = 0 at each preset's attention shape (S = T + 1, H = 4, the CFG double batch where the preset guides, config 4's
    sub-batch, config 5's one-rank share of 16) reports the kernel, grid and item count of the rule for this device's CU
    count; the first, a middle and the last sample are checked against the reference."""
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    for name, B, S, H, d in preset_shapes():
        qkv = random_qkv(B, S, d, seed=S + B)
        got, rep = run(qkv, B, S, H, d, dtype, 0)
        want = expected_dispatch(B, S, H, d, num_cus)
        assert rep == want, f"preset {name} B={B} S={S} d={d}: dispatch ran {rep}, the rule says {want} ({num_cus} CUs)"
        for b in sorted({0, B // 2, B - 1}):
            sl = slice(b * S, (b + 1) * S)
            check(got[sl], reference(qkv[sl], 1, S, H, d, dtype), dtype, f"{NAME[dtype]} preset {name} sample {b}")
        del qkv, got
