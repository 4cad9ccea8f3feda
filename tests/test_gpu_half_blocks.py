"""Kernel-level tests of the 16-bit building blocks (fp16 and bf16 builds): every tile of the reduced-precision GEMM
(csrc/gemmh.hip) under every epilogue the forwards use, the LayerNorm kernels (csrc/norm.hip) and the V2 front end
(RoPE -> causal local attention -> RoPE at t+1, csrc/frontend.hip), each through its C-ABI test entry point against a plain
float64 reference of the same operation on the same (rounded) inputs.  Need an MI355X.

Every output buffer is prefilled with NaN and carries sentinel rows past its end: rows the kernel must write have to come
back finite, every other row (token-0 rows of a token-row map or a compacted LayerNorm, encoder row 0, rows past the
output) has to stay NaN.  A 16-bit output written next to an fp32 one has to equal the fp32 one rounded, bit for bit.

Bounds are relative to max|reference| and were set from the worst error measured on an MI355X (stated per bound) with a
margin of at least 2x; none is looser than the existing kernel tests of the same precision (GEMM 2e-6, GELU 3e-5,
attention-like 16-bit 2e-3 fp16 / 1.6e-2 bf16).
"""
import ctypes as C
import math

import pytest
import torch

from gesturediffusion_amd import _lib

pytestmark = pytest.mark.gpu

F32, F16, BF16 = 0, 1, 2                       # GDX_DTYPE_*
TDT = {F16: torch.float16, BF16: torch.bfloat16}
NAME = {F32: "fp32", F16: "fp16", BF16: "bf16"}
EPS_REL = {F16: 2.0 ** -11, BF16: 2.0 ** -8}    # half an ulp, relative, of a normal 16-bit number
TINY = {F16: 2.0 ** -25, BF16: 0.0}             # half the fp16 subnormal step

# gemmh.hip GH_CONFIGS (mb, nbw) and the 256 x 256 eight-wave kernel (16, 4); (0, 0) = the cost model
GH_TILES = [(8, 4), (7, 4), (6, 4), (5, 4), (4, 4), (12, 2), (10, 2), (9, 2), (8, 2), (6, 2), (5, 2), (4, 2), (8, 1), (4, 1),
            (2, 1), (16, 4)]


def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


def vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def rel(got, ref):
    return float(((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item())


def bits(t):
    return t.contiguous().view(torch.int32)


def assert_rows(buf, written, what):
    """Rows in `written` (bool [rows]) all finite, every other row all NaN."""
    fin = torch.isfinite(buf)
    assert bool(fin[written].all()), f"{what}: a row that must be written holds a non-finite value"
    assert bool(torch.isnan(buf[~written]).all()), f"{what}: a row that must stay untouched was written"


def assert_rounded(c16, c32, dtype, what):
    """The 16-bit output equals the fp32 output rounded to the element type, bit for bit (both come from one value)."""
    assert torch.equal(bits(c16), bits(c32.to(TDT[dtype]).float())), f"{what}: 16-bit output is not the fp32 output rounded"


def within_one_rounding(c16, ref, dtype, abs_tol):
    """|c16 - ref| <= half an ulp of ref + abs_tol: one rounding of a value that is abs_tol from ref."""
    err = (c16.double() - ref).abs()
    lim = ref.abs() * EPS_REL[dtype] * 1.0001 + abs_tol + TINY[dtype]
    return bool((err <= lim).all())


# ---------------------------------------------------------------------------------------------------------------------
# 16-bit GEMM: every tile x every epilogue of the forwards
#   (M, N, K, T): one row; fewer rows than any tile with T = 7 (the 16-row blocks cross sample boundaries); a ragged last
#   tile with T = 37; at M = 20 000, more tiles than CUs for every tile but the eight-wave kernel (which gets several
#   rounds in test_half_gemm_row_cut_config5 and test_half_gemm_eight_wave_three_rounds_odd_slabs), with T = 197 (config 5's
#   S); the same M at K = 320: an odd number (five) of 64-deep K slabs with several tiles per workgroup, so the three slab
#   slots do not come back to slot 0 at a tile's first slab
GEMM_SHAPES = [(1, 256, 256, 1), (50, 256, 320, 7), (333, 512, 256, 37), (3000, 256, 256, 120), (20000, 512, 256, 197),
               (20000, 512, 320, 197)]
# C32: fp32 round-off of a K <= 320 sum; measured worst 2.1e-7 (GELU 1.3e-5 -- the polynomial erf), bounds as
# test_fp16_gemm_vs_torch
GEMM_TOL32, GEMM_TOL32_GELU = 2e-6, 3e-5

# name: (bias, gelu, R, V, rowmap, C32, C16) -- the forwards' launches (csrc/forward.hip forward_core)
EPILOGUES = {
    "bias": (1, 0, 0, 0, 0, 1, 1),              # QKV, out-proj / FFN-2 of the 16-bit stream, output linear
    "bias_gelu": (1, 1, 0, 0, 0, 1, 1),         # FFN-1
    "res_c32": (1, 0, 1, 0, 0, 1, 0),           # out-proj / FFN-2 of bf16's fp32 stream: + fp32 residual into C32
    "res_rowmap": (0, 0, 1, 0, 1, 1, 1),        # V1 input linear: + addend rows, frames into [B, T+1] rows
    "res_vec_c16": (0, 0, 1, 1, 0, 0, 1),       # V2 proj_pose: + addend + per-sample coarse vector, 16-bit xseq
}


def run_linear_half(lib, A, W, bias, R, ldr, V, ldv, c32, c16, M, N, K, T, rowmap, gelu, dtype, tile):
    launched = (C.c_int32 * 5)()
    c_rows = (c32 if c32 is not None else c16).shape[0]
    _lib.check(lib.gdx_linear_half(vp(A), vp(W), vp(bias), vp(R), ldr, vp(V), ldv, vp(c32), vp(c16), c_rows, M, N, K, T,
                                   rowmap, gelu, dtype, tile[0], tile[1], launched, stream()), lib)
    return tuple(launched)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("M,N,K,T", GEMM_SHAPES)
def test_half_gemm_every_tile_every_epilogue(M, N, K, T, dtype):
    """Every gemmh.hip tile kernel (the 15 GH_CONFIGS shapes, the 256 x 256 eight-wave kernel) and the cost model's choice,
    under each epilogue the forwards launch, against float64 on the 16-bit-rounded A and W.  `launched` must name the forced
    tile (a silent fall-back fails); C32 within fp32 round-off, C16 = C32 rounded (or, C16 alone, one rounding of the
    reference); every tile gives the same bits (summation order does not depend on the tile)."""
    lib = _lib.load()
    d = dev()
    g = torch.Generator(device=d).manual_seed(M * 7 + N + dtype)
    A = torch.randn(M, K, device=d, generator=g)
    W = torch.randn(N, K, device=d, generator=g) / K ** 0.5
    bias = torch.randn(N, device=d, generator=g)
    nb = (M + T - 1) // T
    out_map = torch.arange(M, device=d) + torch.arange(M, device=d) // T + 1       # rowmap: m -> m + m/T + 1
    rows_map = M + (M - 1) // T + 1
    ldr, ldv = N + 4, N + 8                                                          # strides wider than N
    R = torch.randn(rows_map, ldr, device=d, generator=g)
    V = torch.randn(nb, ldv, device=d, generator=g)
    Ar, Wr = A.to(TDT[dtype]).double(), W.to(TDT[dtype]).double()
    prod = Ar @ Wr.t()                                                               # once per problem
    seen, worst = set(), {}
    for ename, (ub, gelu, uR, uV, rowmap, w32, w16) in EPILOGUES.items():
        rows_out = rows_map if rowmap else M
        rsel = out_map if rowmap else torch.arange(M, device=d)
        ref = prod.clone()
        if ub:
            ref += bias.double()
        if uR:
            ref += R[rsel, :N].double()
        if uV:
            ref += V[torch.arange(M, device=d) // T, :N].double()
        if gelu:
            ref = torch.nn.functional.gelu(ref)
        written = torch.zeros(rows_out + 3, dtype=torch.bool, device=d)
        written[rsel] = True
        first = None
        for tile in GH_TILES + [(0, 0)]:
            c32 = torch.full((rows_out + 3, N), float("nan"), device=d) if w32 else None
            c16 = torch.full((rows_out + 3, N), float("nan"), device=d) if w16 else None
            la = run_linear_half(lib, A, W, bias if ub else None, R if uR else None, ldr, V if uV else None, ldv, c32, c16,
                                 M, N, K, T, rowmap, gelu, dtype, tile)
            what = f"{NAME[dtype]} {ename} tile {tile} launched {la}"
            if tile != (0, 0):
                assert la == (tile[0], tile[1], 0, 0, 0), f"{what}: the forced tile did not run"
                seen.add(la[:2])
            else:
                assert (la[0], la[1]) in GH_TILES, what
                if rowmap or uV:
                    assert la[2] == 0, f"{what}: a row cut under a row map / per-sample vector"
            for buf, nm in ((c32, "C32"), (c16, "C16")):
                if buf is not None:
                    assert_rows(buf, written, f"{what} {nm}")
            if c32 is not None:
                e = rel(c32[rsel], ref)
                worst[ename] = max(worst.get(ename, 0.0), e)
                assert e < (GEMM_TOL32_GELU if gelu else GEMM_TOL32), f"{what}: C32 rel err {e:.2e}"
                if c16 is not None:
                    assert_rounded(c16[rsel], c32[rsel], dtype, what)
            else:
                assert within_one_rounding(c16[rsel], ref, dtype, GEMM_TOL32 * float(ref.abs().max())), \
                    f"{what}: C16 is more than one rounding from the reference"
            out = c32 if c32 is not None else c16
            if first is None:
                first = out
            else:
                assert torch.equal(bits(out), bits(first)), f"{what}: output bits differ from tile {GH_TILES[0]}"
    assert seen == set(GH_TILES), f"tile kernels that did not run: {set(GH_TILES) - seen}"
    print(f"\n[gemmh {NAME[dtype]} M={M} N={N} K={K} T={T}] 16 forced tiles ran; worst C32 rel err "
          + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


def test_half_gemm_row_cut_config5():
    """Config 5's bf16 fp32-stream out-projection (M = 66 688, N = K = 1 024, + fp32 residual into C32): on a 256-CU part the
    cost model cuts the rows (eight-wave kernel for whole rounds, another tile for the tail, R / C32 offset for the tail
    launch).  The result must be bit-equal to the forced eight-wave kernel over all rows, and sampled rows (both sides of
    the cut, the last rows) within the fp32 round-off bound of the other GEMM cases."""
    lib = _lib.load()
    d = dev()
    M, N, K = 66688, 1024, 1024
    g = torch.Generator(device=d).manual_seed(5)
    A = torch.randn(M, K, device=d, generator=g)
    W = torch.randn(N, K, device=d, generator=g) / K ** 0.5
    bias = torch.randn(N, device=d, generator=g)
    R = torch.randn(M, N, device=d, generator=g)
    outs = {}
    for tile in [(0, 0), (16, 4)]:
        c32 = torch.full((M + 2, N), float("nan"), device=d)
        outs[tile] = (c32, run_linear_half(lib, A, W, bias, R, N, None, N, c32, None, M, N, K, 1, 0, 0, BF16, tile))
    c32, la = outs[(0, 0)]
    print(f"\n[gemmh bf16 config-5 out-proj] cost model launched {la}")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus == 256:
        assert la[0] == 16 and 0 < la[2] < M and (la[3], la[4]) in GH_TILES, f"no row cut on a 256-CU part: {la}"
    assert outs[(16, 4)][1] == (16, 4, 0, 0, 0)
    written = torch.zeros(M + 2, dtype=torch.bool, device=d)
    written[:M] = True
    assert_rows(c32, written, "row cut C32")
    assert torch.equal(bits(c32), bits(outs[(16, 4)][0])), "the row cut changed bits"
    cut = la[2] if la[2] else M // 2
    rows = torch.cat([torch.arange(0, 64), torch.arange(cut - 64, min(cut + 64, M)), torch.arange(M - 64, M),
                      torch.randint(0, M, (256,), generator=torch.Generator().manual_seed(1))]).to(d)
    ref = A[rows].bfloat16().double() @ W.bfloat16().double().t() + bias.double() + R[rows].double()
    assert rel(c32[rows], ref) < GEMM_TOL32


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_half_gemm_eight_wave_three_rounds_odd_slabs(dtype):
    """The eight-wave kernel with three tiles on a workgroup (2 cus + 1 tiles of 256 x 256 at N = 512), an odd number (five) of
    64-deep K slabs per tile, a ragged last row panel, under the plain epilogue and under the row-indexed one (token-row map
    + addend rows, T = 197): its DMA streams cross every tile boundary two slabs ahead of the MFMAs, and the five-unit ring
    meets a tile's first slab in a different slot every time.  C32 against float64 on 2 048 sampled rows and the last 256,
    C16 = C32 rounded, and the same bits as the forced 128 x 256 tile over every row."""
    lib = _lib.load()
    d = dev()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    ntm = (2 * cus + 1 + 1) // 2
    M, N, K, T = 256 * ntm - 100, 512, 320, 197
    g = torch.Generator(device=d).manual_seed(M + dtype)
    A = torch.randn(M, K, device=d, generator=g)
    W = torch.randn(N, K, device=d, generator=g) / K ** 0.5
    bias = torch.randn(N, device=d, generator=g)
    out_map = torch.arange(M, device=d) + torch.arange(M, device=d) // T + 1
    rows_map = M + (M - 1) // T + 1
    ldr = N + 4
    R = torch.randn(rows_map, ldr, device=d, generator=g)
    rows = torch.cat([torch.randint(0, M, (2048,), generator=torch.Generator().manual_seed(2)), torch.arange(M - 256, M)]).to(d)
    prod = A[rows].to(TDT[dtype]).double() @ W.to(TDT[dtype]).double().t()
    for ename in ("bias", "res_rowmap"):
        ub, gelu, uR, uV, rowmap, w32, w16 = EPILOGUES[ename]
        rows_out = rows_map if rowmap else M
        rsel = out_map if rowmap else torch.arange(M, device=d)
        ref = prod + (bias.double() if ub else 0.0) + (R[rsel[rows], :N].double() if uR else 0.0)
        written = torch.zeros(rows_out + 3, dtype=torch.bool, device=d)
        written[rsel] = True
        outs = {}
        for tile in [(16, 4), (8, 4)]:
            c32 = torch.full((rows_out + 3, N), float("nan"), device=d)
            c16 = torch.full((rows_out + 3, N), float("nan"), device=d)
            la = run_linear_half(lib, A, W, bias if ub else None, R if uR else None, ldr, None, N, c32, c16, M, N, K, T, rowmap,
                                 gelu, dtype, tile)
            what = f"{NAME[dtype]} {ename} M={M} tile {tile} launched {la}"
            assert la == (tile[0], tile[1], 0, 0, 0), f"{what}: the forced tile did not run"
            assert_rows(c32, written, what + " C32")
            assert_rows(c16, written, what + " C16")
            outs[tile] = (c32, c16, what)
        c32, c16, what = outs[(16, 4)]
        e = rel(c32[rsel[rows]], ref)
        print(f"\n[gemmh {what}] C32 rel err {e:.2e} on {rows.numel()} rows")
        assert e < GEMM_TOL32, f"{what}: C32 rel err {e:.2e}"
        assert_rounded(c16[rsel], c32[rsel], dtype, what)
        assert torch.equal(bits(c32), bits(outs[(8, 4)][0])), f"{what}: C32 bits differ from tile (8, 4)"
        assert torch.equal(bits(c16), bits(outs[(8, 4)][1])), f"{what}: C16 bits differ from tile (8, 4)"


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm
LN_D =[256, 512, 1024, 96, 128, 384, 768, 2048]      # vec kernels (fp32: all three; 16-bit: 512, 1 024), then generic
# fp32 statistics over rows of up to 2 048: measured worst 1.0e-6 (out32, d = 256, both input kinds; 7e-7 - 9e-7 at the
# other widths), so a margin of 2x; the offset rows lose log10(offset / spread) digits of the mean to fp32, which stays
# inside this bound at offset 20
LN_TOL32 = 2e-6


def ln_inputs(rows, d, seed, device):
    """Rows cycle through: N(0, 1); 20 + N(0, 1) (large common offset); N(0, 1e-3) (spread so small that eps = 1e-5
    dominates the variance); 3 N(0, 1) - 1."""
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.randn(rows, d, device=device, generator=g)
    kind = torch.arange(rows, device=device) % 4
    x[kind == 1] += 20.0
    x[kind == 2] *= 1e-3
    x[kind == 3] = 3.0 * x[kind == 3] - 1.0
    res = torch.randn(rows, d, device=device, generator=g) * 0.5
    res[kind == 2] *= 1e-3
    return x, res


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("d", LN_D)
def test_layernorm_kernels(d, dtype):
    """launch_layernorm (fp32 input: layernorm_vec_kernel<1,2,4>, layernorm_gen_kernel, 16-bit copy) and launch_layernorm_f16
    (16-bit input: layernorm_h_vec_kernel<1,2>, layernorm_h_gen_kernel) against float64 layer_norm (eps 1e-5, biased
    variance) of the same (rounded) inputs: rows 1, 3, 5, 2 999; with and without the residual; compact_S 2, 197, 521
    (token 0 of every sample dropped, nothing stored past B (S - 1) rows)."""
    lib = _lib.load()
    dv = dev()
    g = torch.Generator(device=dv).manual_seed(d)
    gamma = 1.0 + 0.5 * torch.randn(d, device=dv, generator=g)
    beta = 0.5 * torch.randn(d, device=dv, generator=g)
    cases = [(r, 0) for r in (1, 3, 5, 2999)] + [(3 * 2, 2), (4 * 197, 197), (5 * 521, 521)]
    worst = 0.0
    for rows, cs in cases:
        x, res = ln_inputs(rows, d, rows + d, dv)
        keep = torch.ones(rows, dtype=torch.bool, device=dv)
        if cs:
            keep[::cs] = False
        n_out = int(keep.sum())
        for half_input in (0, 1):
            for use_res in (0, 1):
                xr, rr = (x.to(TDT[dtype]).double(), res.to(TDT[dtype]).double()) if half_input else (x.double(), res.double())
                v = xr + rr if use_res else xr
                ref = torch.nn.functional.layer_norm(v, (d,), gamma.double(), beta.double(), 1e-5)[keep]
                o32 = torch.full((n_out + 2, d), float("nan"), device=dv)
                o16 = torch.full((n_out + 2, d), float("nan"), device=dv)
                _lib.check(lib.gdx_layernorm(vp(x), vp(res) if use_res else None, vp(gamma), vp(beta), vp(o32), vp(o16),
                                             n_out + 2, rows, d, cs, half_input, dtype, stream()), lib)
                what = f"{NAME[dtype]} LN d={d} rows={rows} compact_S={cs} half_input={half_input} res={use_res}"
                written = torch.zeros(n_out + 2, dtype=torch.bool, device=dv)
                written[:n_out] = True
                assert_rows(o32, written, what + " out32")
                assert_rows(o16, written, what + " out16")
                e = rel(o32[:n_out], ref)
                worst = max(worst, e)
                assert e < LN_TOL32, f"{what}: out32 rel err {e:.2e}"
                assert_rounded(o16[:n_out], o32[:n_out], dtype, what)
                if half_input:          # the forwards' usual call: no fp32 copy; the same 16-bit bits
                    o16b = torch.full_like(o16, float("nan"))
                    _lib.check(lib.gdx_layernorm(vp(x), vp(res) if use_res else None, vp(gamma), vp(beta), None, vp(o16b),
                                                 n_out + 2, rows, d, cs, half_input, dtype, stream()), lib)
                    assert torch.equal(bits(o16b), bits(o16)), what + ": out16 differs without out32"
    print(f"\n[layernorm {NAME[dtype]} d={d}] worst out32 rel err {worst:.2e}")


# ---------------------------------------------------------------------------------------------------------------------
# V2 front end.  (E, heads, window, T, B): E = d / heads.  heads = 8 as the model; the other head counts make the
# (sample, head, window) count not a multiple of the four waves of an MFMA kernel's block (surplus waves).
LA_CASES = [
    (16, 8, 10, 20, 2),        # scalar kernel (E = 16)
    (48, 8, 10, 10, 3),        # scalar kernel (E = 48), T = window
    (32, 8, 10, 520, 1),       # fp32 MFMA <32>; the 16-bit dtypes take the fp32 kernel + 16-bit copy
    (64, 8, 10, 520, 2),       # config 5: d = 512, window 10, T = 520
    (128, 8, 16, 32, 3),       # window 16: all 32 key slots, T = 2 window
    (64, 8, 1, 7, 2),          # window 1
    (64, 3, 10, 30, 3),        # 27 work items
    (128, 5, 10, 20, 1),       # 10 work items
    (32, 3, 16, 16, 1),        # 3 work items, window 16
    (64, 3, 16, 32, 1),        # 6 work items, window 16
    (16, 8, 20, 40, 2),        # window 20: the scalar fallback
    (64, 8, 20, 60, 1),        # window 20 at E = 64: the scalar fallback for every dtype
]
# measured worst (rel to max|ref|): fp32 kernels 2.3e-7 (the 16-bit dtypes' fp32 kernel included); 16-bit kernel
# fp16 4.0e-4, bf16 3.5e-3 -- bounds 4x, 2.5x and 2.3x those
LA_TOL32 = 1e-6
LA_TOL16 = {F16: 1e-3, BF16: 8e-3}


def expected_kernel(E, window, dtype):
    if dtype != F32 and E in (64, 128) and window <= 16:
        return 2
    return 1 if E in (32, 64, 128) and window <= 16 else 0


def local_attention_ref(x, ang, B, T, heads, window):
    """float64 through the oracle: head split, RoPE at positions 0..T-1, causal local attention, RoPE at 1..T."""
    from oracle import mdm_forward as omf
    d = x.shape[-1]
    xs = omf._heads_split(x.permute(1, 0, 2), B, T, heads)
    xs = omf.apply_rotary(xs, torch.cat([ang[:T], ang[:T]], dim=-1))
    xs = omf.local_attention(xs, window=window)
    xs = omf.apply_rotary(xs, torch.cat([ang[1:T + 1], ang[1:T + 1]], dim=-1))
    return omf._heads_merge(xs, B, T, heads).permute(1, 0, 2).reshape(B, T, d)


def run_local_attention(E, heads, window, T, B, dtype, real_rope=False):
    lib = _lib.load()
    dv = dev()
    d = E * heads
    g = torch.Generator().manual_seed(E * 1000 + T * 10 + window + dtype)
    xseq = torch.randn(B, T, d, generator=g) * 1.5
    if real_rope:               # the model's own tables (model/mdm.py SinusoidalEmbeddings -> rope.cos / rope.sin)
        from gesturediffusion_amd.model.mdm import SinusoidalEmbeddings
        from oracle import mdm_forward as omf
        cos, sin = SinusoidalEmbeddings(E).tables(T + 1)
        ang = omf.rotary_freqs(T + 1, E)[:, :E // 2].double()
    else:                       # random angles: a wrong position / frequency index cannot hide behind cos = 1, sin = 0
        ang = (torch.rand(T + 1, E // 2, generator=g, dtype=torch.float64) * 2 - 1) * math.pi
        cos, sin = ang.cos().float(), ang.sin().float()
    kern = expected_kernel(E, window, dtype)
    x_in = xseq.to(TDT[dtype]).double() if kern == 2 else xseq.double()
    ref = local_attention_ref(x_in, ang, B, T, heads, window)
    rows = B * (T + 1) + 2
    enc = torch.full((rows, d), float("nan"), device=dv)
    enc16 = torch.full((rows, d), float("nan"), device=dv) if dtype != F32 else None
    k = C.c_int32(-1)
    xd, cd, sd = xseq.to(dv), cos.to(dv), sin.to(dv)      # named: a temporary's memory could be reused before the call
    _lib.check(lib.gdx_local_attention(vp(xd), vp(cd), vp(sd), vp(enc), vp(enc16), rows, B, T, d, heads, window, dtype,
                                       C.byref(k), stream()), lib)
    what = f"{NAME[dtype]} local attention E={E} heads={heads} window={window} T={T} B={B}"
    assert k.value == kern, f"{what}: kernel {k.value}, expected {kern}"
    written = torch.zeros(rows, dtype=torch.bool)
    for b in range(B):
        written[b * (T + 1) + 1:(b + 1) * (T + 1)] = True
    written = written.to(dv)
    assert_rows(enc, written, what + " enc")
    got = enc[written].view(B, T, d).cpu()
    e = rel(got, ref)
    if kern == 2:
        assert_rows(enc16, written, what + " enc16")
        assert e < LA_TOL16[dtype], f"{what}: rel err {e:.2e}"
    else:
        assert e < LA_TOL32, f"{what}: rel err {e:.2e}"
    if enc16 is not None:
        assert_rows(enc16, written, what + " enc16")
        assert_rounded(enc16[written], enc[written], dtype, what)
    return e


@pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("E,heads,window,T,B", LA_CASES)
def test_local_attention_kernels(E, heads, window, T, B, dtype):
    """The V2 front end through the forwards' dispatch (local_attention_mfma_kernel<32,64,128>, the scalar
    local_attention_kernel, local_attention_h_kernel<64,128> in fp16 / bf16, or the fp32 kernel with a 16-bit copy)
    against the oracle's float64 RoPE / local attention on random-angle tables (the 16-bit kernel: on the rounded xseq).
    Encoder row 0 of every sample and the sentinel rows stay untouched."""
    e = run_local_attention(E, heads, window, T, B, dtype)
    print(f"\n[local attention {NAME[dtype]} E={E} heads={heads} window={window} T={T} B={B}] rel err {e:.2e}")


@pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=["fp32", "fp16", "bf16"])
def test_local_attention_model_rope(dtype):
    """The same at config 5's front end with the model's own RoPE tables."""
    run_local_attention(64, 8, 10, 520, 2, dtype, real_rope=True)
