"""Kernel-level tests of the boundary kernels of the denoiser step (csrc/boundary.hip and csrc/boundaryh.hip: the two pose <-> token-major transposes,
small_linear, gather_rows, mfcc_project, token0) and of masked_l2 (csrc/bound.hip), each through its C-ABI entry point against
a plain reference of the same operation: torch indexing / torch fp32 in the reference's order where the kernel must be
bit-exact, float64 elsewhere.  Need an MI355X.

Every output buffer is prefilled with NaN and carries at least two sentinel rows past its end, plus sentinel columns where
rows are strided: elements the kernel must write have to come back finite, every other element has to stay NaN.  Inputs
carry NaN wherever the kernel must not read: behind a row's K / C / J columns, in the rows behind a buffer and in the source
sample behind the last one (which `b` in place of `b % Bsrc` would reach).

Integer-valued inputs make every partial sum an exact fp32 integer, so those results must equal float64 exactly, whatever
the summation order: a dropped, doubled or mis-strided term cannot hide.  Normal-random inputs get a per-element bound that
holds for any order, with or without FMA; the worst ratio to each bound is printed.  Measured on an MI355X, as a fraction of
the bound: small_linear <= 0.044 (at K = 1; 1e-3 at K = 512), mfcc_project <= 0.17, masked_l2 <= 0.085 (one element; 6e-5
at the model's pose shape).

The one measured tolerance is SILU_TOL (see there).
"""
import ctypes as C

import pytest
import torch

from gesturediffusion_amd import _lib

pytestmark = pytest.mark.gpu

F32, F16, BF16 = 0, 1, 2                       # GDX_DTYPE_*
TDT = {F16: torch.float16, BF16: torch.bfloat16}
NAME = {F32: "fp32", F16: "fp16", BF16: "bf16"}
U = 2.0 ** -24                                  # fp32 unit round-off
NAN = float("nan")


def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


def vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(t):
    return t.contiguous().view(torch.int32)


def gen(seed):
    return torch.Generator(device=dev()).manual_seed(seed)


def nans(*shape):
    return torch.full(shape, NAN, device=dev())


def randint(g, lo, hi, *shape):
    """Integer-valued fp32 in [lo, hi]."""
    return torch.randint(lo, hi + 1, shape, device=dev(), generator=g).float()


def assert_written(buf, written, what):
    """Elements in `written` (bool, broadcastable to buf: [rows, 1] or [rows, cols]) all finite, every other one NaN."""
    written = written.expand_as(buf)
    assert bool(torch.isfinite(buf[written]).all()), f"{what}: an element that must be written holds a non-finite value"
    assert bool(torch.isnan(buf[~written]).all()), f"{what}: an element that must stay untouched was written"


def assert_rows(buf, written, what):
    """Rows in `written` (bool [rows]) all finite, every other row all NaN."""
    assert_written(buf, written[:, None], what)


def assert_rounded(c16, c32, dtype, what):
    """The 16-bit output equals the fp32 output rounded to the element type, bit for bit (both come from one value)."""
    assert torch.equal(bits(c16), bits(c32.to(TDT[dtype]).float())), f"{what}: 16-bit output is not the fp32 output rounded"


def row_mask(n, rows):
    m = torch.zeros(n, dtype=torch.bool, device=dev())
    m[rows] = True
    return m


# ---------------------------------------------------------------------------------------------------------------------
# transposes: bit-exact against torch indexing
#   (J, T, ldx): smaller than a 32 x 32 tile; one past / one short of a tile; several tiles, ragged on both axes, with the
#   padding columns all in the last J tile (150 -> 160, 263 -> 288) next to 22 / 7 source rows; no ragged edge at all
TR_SHAPES = [(7, 9, 32), (33, 31, 64), (150, 60, 160), (263, 196, 288), (64, 64, 64)]
TR_BATCH = [(1, 1), (3, 3), (4, 2)]            # (B, Bsrc); (4, 2) is CFG: both halves read the same source

# Values a float -> 16-bit conversion gets wrong first: exact round-to-nearest-even ties of fp16 (11-bit significand) and
# bf16 (8-bit), fp16's subnormal range with its ties (step 2^-24; 2^-25 ties to zero), the fp16 overflow threshold (65504 is
# the largest finite, 65520 ties to inf, just below it rounds to 65504), both zeros
SPECIALS = [
    1 + 2.0 ** -11, -(1 + 2.0 ** -11), 1 + 3 * 2.0 ** -11, 2049.0, 2051.0, -2049.0, 0.5 + 2.0 ** -12,
    1 + 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 3 * 2.0 ** -8, 257.0, 259.0, 3.0 + 2.0 ** -7,
    2.0 ** -24, 2.0 ** -25, -(2.0 ** -25), 3 * 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -20), 2.0 ** -20 + 2.0 ** -25, 1e-5, -1e-6, 6e-8,
    3e-8, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, -(2.0 ** -14) + 2.0 ** -25, 6.0e-5,
    65504.0, -65504.0, 65520.0, -65520.0, 65519.996, -65519.996, 65505.0, 0.0, -0.0,
    1e-3, -1.234e-3, 0.999e-3, 1e3, -999.7, 1000.25,
]


def pose_tensor(g, Bsrc, J, T):
    """[Bsrc + 1, J, T]: normal values at magnitudes 1e-3, 1 and 1e3 with SPECIALS scattered over every source sample;
    the sample behind the last is NaN (no kernel may read it)."""
    x = torch.randn(Bsrc, J, T, device=dev(), generator=g)
    x *= torch.tensor([1e-3, 1.0, 1e3], device=dev())[torch.randint(0, 3, (Bsrc, J, T), device=dev(), generator=g)]
    sp = torch.tensor(SPECIALS, device=dev())
    assert J * T >= len(SPECIALS)
    for b in range(Bsrc):
        pos = torch.randperm(J * T, device=dev(), generator=g)[:len(SPECIALS)]
        x[b].view(-1)[pos] = sp
    return torch.cat([x, nans(1, J, T)])


def run_transpose_in(lib, x, B, Bsrc, J, T, ldx, dtype):
    xt = nans(B * T + 2, ldx)
    _lib.check(lib.gdx_transpose_in(vp(x), vp(xt), xt.shape[0], B, Bsrc, J, T, ldx, dtype, stream()), lib)
    return xt


@pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("B,Bsrc", TR_BATCH)
@pytest.mark.parametrize("J,T,ldx", TR_SHAPES)
def test_transpose_in_bit_exact(J, T, ldx, B, Bsrc, dtype):
    """xt[b*T + t][j] = x[b % Bsrc][j][t] bit for bit (fp32), or x.to(dtype) bit for bit (the 16-bit kernels: ties, fp16
    subnormals, +-65504 / +-65520, both zeros); columns J..ldx-1 of every written row are +0.0 exactly; rows >= B*T stay NaN."""
    lib = _lib.load()
    x = pose_tensor(gen(J * 1000 + T + B), Bsrc, J, T)
    xt = run_transpose_in(lib, x, B, Bsrc, J, T, ldx, dtype)
    what = f"transpose_in {NAME[dtype]} J={J} T={T} ldx={ldx} B={B} Bsrc={Bsrc}"
    src = x[torch.arange(B, device=x.device) % Bsrc]                     # [B, J, T]
    ref = src.permute(0, 2, 1).reshape(B * T, J)
    if dtype != F32:
        ref = ref.to(TDT[dtype]).float()
        if dtype == F16:
            assert bool(torch.isinf(ref).any()) and bool(((ref != 0) & (ref.abs() < 2.0 ** -14)).any()), "specials missing"
    assert bool(torch.isnan(xt[B * T:]).all()), f"{what}: a row past B*T was written"
    assert torch.equal(bits(xt[:B * T, :J]), bits(ref)), f"{what}: values differ from the source"
    assert bool((bits(xt[:B * T, J:]) == 0).all()), f"{what}: a padding column is not +0.0"
    if B > Bsrc:
        assert torch.equal(bits(xt[:Bsrc * T]), bits(xt[Bsrc * T:B * T])), f"{what}: the two CFG halves differ"


@pytest.mark.parametrize("B", [1, 3, 4])
@pytest.mark.parametrize("J,T,ldx", TR_SHAPES)
def test_transpose_out_bit_exact(J, T, ldx, B):
    """y[b*J + j][t] = yt[b*T + t][j] bit for bit with ldy > J and NaN in the unread columns J..ldy-1 and in the rows behind
    yt; rows >= B*J of y stay NaN."""
    lib = _lib.load()
    ldy = ldx + 3
    g = gen(J + T + B)
    yt = nans(B * T + 2, ldy)
    yt[:B * T, :J] = torch.randn(B * T, J, device=dev(), generator=g)
    y = nans(B * J + 2, T)
    _lib.check(lib.gdx_transpose_out(vp(yt), vp(y), y.shape[0], B, J, T, ldy, stream()), lib)
    what = f"transpose_out J={J} T={T} ldy={ldy} B={B}"
    assert_rows(y, row_mask(B * J + 2, slice(0, B * J)), what)
    ref = yt[:B * T, :J].reshape(B, T, J).permute(0, 2, 1).reshape(B * J, T)
    assert torch.equal(bits(y[:B * J]), bits(ref)), f"{what}: values differ from the source"


@pytest.mark.parametrize("J,T,ldx", TR_SHAPES)
def test_transpose_round_trip(J, T, ldx):
    """out(in(x)) == x bit for bit (fp32, three samples, the padded stride of the forwards on both sides)."""
    lib = _lib.load()
    B = 3
    x = pose_tensor(gen(J + T), B, J, T)
    xt = run_transpose_in(lib, x, B, B, J, T, ldx, F32)
    y = nans(B * J + 2, T)
    _lib.check(lib.gdx_transpose_out(vp(xt), vp(y), y.shape[0], B, J, T, ldx, stream()), lib)
    assert torch.equal(bits(y[:B * J]), bits(x[:B].reshape(B * J, T))), f"round trip J={J} T={T} ldx={ldx}"
    assert bool(torch.isnan(y[B * J:]).all())


# ---------------------------------------------------------------------------------------------------------------------
# gather_rows: d below, between and above multiples of the 256-thread block
@pytest.mark.parametrize("M", [1, 5])
@pytest.mark.parametrize("d", [32, 384, 512])
def test_gather_rows_bit_exact_and_clamped(d, M):
    """out[m] = table[clamp(idx[m], 0, max_rows - 1)] bit for bit: indices 0, max_rows - 1, -3 (-> first row) and
    max_rows + 7 (-> last row).  The table is followed by NaN rows that must never reach the output."""
    lib = _lib.load()
    max_rows = 11
    table = torch.cat([torch.randn(max_rows, d, device=dev(), generator=gen(d)), nans(8, d)])
    picks = [0, max_rows - 1, -3, max_rows + 7, 4]
    for idx_list in ([picks] if M == 5 else [[i] for i in picks]):
        idx = torch.tensor(idx_list, dtype=torch.int64, device=dev())
        out = nans(M + 2, d)
        _lib.check(lib.gdx_gather_rows(vp(table), vp(idx), vp(out), out.shape[0], M, d, max_rows, stream()), lib)
        what = f"gather_rows d={d} idx={idx_list}"
        assert_rows(out, row_mask(M + 2, slice(0, M)), what)
        assert torch.equal(bits(out[:M]), bits(table[idx.clamp(0, max_rows - 1)])), f"{what}: wrong row"


# ---------------------------------------------------------------------------------------------------------------------
# small_linear
#   (M, N, K, lda, ldw, ldo): one term; K one short of the 64 lanes; K one past them (a lane with two terms, the others
#   with one) and M one past the four rows of a block; the seed-encoder class K = 263 * 8 (32-33 terms per lane); the
#   timestep MLP at d = 512 with three row blocks
SL_SHAPES = [(1, 1, 1, 1, 32, 1), (3, 5, 63, 63, 64, 8), (5, 384, 65, 70, 96, 384), (2, 64, 2104, 2104, 2112, 64),
             (9, 512, 512, 512, 512, 512)]

# SiLU s / (1 + expf(-s)) on an exact argument against float64 s * sigmoid(s), relative to max(|ref|, 2^-126), over the
# elements where expf(-s) is finite (-s <= log(FLT_MAX)): measured worst on an MI355X 9.992e-8 (integer-valued arguments of
# the five shapes, dense weights with |s| up to 3.5e3 and sparse ones with |s| up to 272); the bound is 4x that, which leaves room for a different expf code path in another
# compiler release.  Where expf(-s) overflows (s <= -89 for an integer s) the kernel divides by inf and returns -0 while the
# true value (|.| <= 2.7e-37) is still a normal number, so a relative measure is 1 there by construction: those elements
# are held to "zero or a tiny negative, never NaN" instead: ref * (1 + SILU_TOL) <= got <= 0.
SILU_MEASURED = 9.992e-8
SILU_TOL = 4 * SILU_MEASURED
LOG_FLT_MAX = 88.72283905206835


def sl_operands(g, M, N, K, lda, ldw, integer, sparse=False):
    """A [M + 2][lda], W [N][ldw] (NaN in A[:, K:], W[:, K:] and the two rows behind A) and bias [N]."""
    A, W = nans(M + 2, lda), nans(N, ldw)
    if integer:
        A[:M, :K], W[:, :K], bias = randint(g, -8, 8, M, K), randint(g, -8, 8, N, K), randint(g, -64, 64, N)
        if sparse:      # ~6 non-zero weights per row: pre-activations spread over the whole SiLU range, not saturated
            W[:, :K] *= (torch.rand(N, K, device=dev(), generator=g) < 6.0 / K).float()
    else:
        A[:M, :K] = torch.randn(M, K, device=dev(), generator=g)
        W[:, :K] = torch.randn(N, K, device=dev(), generator=g) / K ** 0.5
        bias = torch.randn(N, device=dev(), generator=g)
    return A, W, bias


def run_small_linear(lib, A, lda, W, ldw, bias, M, N, K, ldo, act, what):
    out = nans(M + 2, ldo)
    _lib.check(lib.gdx_small_linear(vp(A), lda, vp(W), ldw, vp(bias), vp(out), out.shape[0], ldo, M, N, K, act, stream()), lib)
    written = torch.zeros(M + 2, ldo, dtype=torch.bool, device=dev())
    written[:M, :N] = True
    assert_written(out, written, what)                      # columns N..ldo-1 and the rows behind stay NaN
    return out[:M, :N]


def sl_reference(A, W, bias, M, K):
    """float64 pre-activation and the magnitude sum of its terms, sum_k |a_k w_k| + |bias_n|."""
    a, w = A[:M, :K].double(), W[:, :K].double()
    pre, mag = a @ w.t(), a.abs() @ w.abs().t()
    if bias is not None:
        pre, mag = pre + bias.double(), mag + bias.double().abs()
    return pre, mag


def silu64(s):
    return s * torch.sigmoid(s)


@pytest.mark.parametrize("use_bias", [1, 0], ids=["bias", "nobias"])
@pytest.mark.parametrize("M,N,K,lda,ldw,ldo", SL_SHAPES)
def test_small_linear(M, N, K, lda, ldw, ldo, use_bias):
    """Integer-valued inputs (|a|, |w| <= 8, |bias| <= 64; sum |a||w| + |bias| < 2^24, asserted): act = 0 equals float64
    exactly; SiLU on the exact argument within SILU_TOL, with arguments below -90 (expf(-s) overflows: zero or a tiny
    negative, never NaN) and above +90.  Normal-random inputs: |got - ref| <= (K + 2) 2^-24 (sum_k |a_k w_k| + |bias_n|), any
    summation order, FMA or not; through SiLU (derivative at most 1.0999) 1.1 times that plus SILU_TOL |ref|."""
    lib = _lib.load()
    g = gen(M * 31 + N * 7 + K + use_bias)
    tag = f"small_linear M={M} N={N} K={K} lda={lda} ldw={ldw} ldo={ldo} bias={use_bias}"
    # integer-valued, act = 0: exact
    A, W, bias = sl_operands(g, M, N, K, lda, ldw, integer=True)
    bias = bias if use_bias else None
    pre, mag = sl_reference(A, W, bias, M, K)
    assert float(mag.max()) < 2 ** 24
    got = run_small_linear(lib, A, lda, W, ldw, bias, M, N, K, ldo, 0, f"{tag} int")
    assert torch.equal(got.double(), pre), f"{tag}: integer inputs are not exact, worst |diff| {float((got.double() - pre).abs().max())}"
    # integer-valued, SiLU: dense operands (mostly saturated arguments) and sparse weights (arguments across the range)
    worst_silu = 0.0
    for sparse in (False, True):
        if sparse:
            A, W, b2 = sl_operands(g, M, N, K, lda, ldw, integer=True, sparse=True)
            bias = b2 if use_bias else None
            if M >= 2 and K >= 2:        # arguments +-128 at (0, 0) and (1, 0)
                W[0, :K] = 0.0
                W[0, :2] = 8.0
                A[0, :2], A[1, :2] = 8.0, -8.0
                if bias is not None:
                    bias[0] = 0.0
        pre, mag = sl_reference(A, W, bias, M, K)
        assert float(mag.max()) < 2 ** 24
        if sparse and M >= 2 and K >= 2:
            assert float(pre.min()) < -90 and float(pre.max()) > 90
        got = run_small_linear(lib, A, lda, W, ldw, bias, M, N, K, ldo, 1, f"{tag} int silu").double()
        ref = silu64(pre)
        ovf = -pre > LOG_FLT_MAX                                           # expf(-s) = inf
        ratio = (got - ref).abs() / ref.abs().clamp_min(2.0 ** -126)
        r = float(ratio[~ovf].max()) if bool((~ovf).any()) else 0.0
        worst_silu = max(worst_silu, r)
        print(f"\n[{tag} silu{' sparse' if sparse else ''}] worst |got - ref| / max(|ref|, 2^-126) {r:.3e} where expf(-s) is finite "
              f"(tolerance {SILU_TOL:.3e}); arguments in [{float(pre.min()):.0f}, {float(pre.max()):.0f}], {int(ovf.sum())} in the "
              f"overflow range, ratio there {float(ratio[ovf].max()) if bool(ovf.any()) else 0.0:.3e}")
        assert r <= SILU_TOL, f"{tag}: SiLU off by {r:.3e} relative"
        assert bool(((got[ovf] <= 0) & (got[ovf] >= ref[ovf] * (1 + SILU_TOL) - 2.0 ** -149)).all()), \
            f"{tag}: SiLU of an argument below -{LOG_FLT_MAX:.1f} is not zero or a tiny negative"
    # normal-random: the order-independent bound
    A, W, bias = sl_operands(g, M, N, K, lda, ldw, integer=False)
    bias = bias if use_bias else None
    pre, mag = sl_reference(A, W, bias, M, K)
    lim = (K + 2) * U * mag
    got = run_small_linear(lib, A, lda, W, ldw, bias, M, N, K, ldo, 0, f"{tag} randn").double()
    r0 = float(((got - pre).abs() / lim).max())
    assert float(pre.min()) > -80                                          # nowhere near the overflow range
    ref = silu64(pre)
    lim1 = 1.1 * lim + SILU_TOL * ref.abs().clamp_min(2.0 ** -126)
    got1 = run_small_linear(lib, A, lda, W, ldw, bias, M, N, K, ldo, 1, f"{tag} randn silu").double()
    r1 = float(((got1 - ref).abs() / lim1).max())
    print(f"[{tag} randn] worst |got - ref| / bound: act 0 {r0:.3e}, SiLU {r1:.3e}")
    assert r0 <= 1.0, f"{tag}: {r0:.3e} of the bound"
    assert r1 <= 1.0, f"{tag} SiLU: {r1:.3e} of the bound"


# ---------------------------------------------------------------------------------------------------------------------
# mfcc_project
#   (B, Bsrc, C, T, d, rps, off, pe): one row, one channel; V2 layout, 63 rows (one short of a 64-row block); V1 layout
#   with CFG, 260 rows (a last block of 4), row 0 of every sample untouched; C at the cap and n over three 256-thread
#   blocks; rps > T + off (unwritten rows inside every sample)
MP_SHAPES = [(1, 1, 1, 1, 32, 1, 0, 0), (3, 3, 26, 21, 384, 21, 0, 0), (4, 2, 26, 65, 512, 66, 1, 1),
             (2, 2, 32, 64, 768, 64, 0, 0), (2, 1, 13, 33, 96, 40, 3, 1)]


@pytest.mark.parametrize("B,Bsrc,C,T,d,rps,off,use_pe", MP_SHAPES)
def test_mfcc_project(B, Bsrc, C, T, d, rps, off, use_pe):
    """out[b*rps + t + off][n] = sum_c mfcc[b % Bsrc][c][t] W[n][c] + bias[n] (+ pe[t + 1][n]); every other row stays NaN.
    Integer-valued inputs equal float64 exactly; normal-random inputs within (C + 4) 2^-24 (sum_c |m_c w_c| + |bias| + |pe|)
    (bias and pe are two more terms: K = C + 2 in small_linear's bound).  ldw > C with NaN behind column C; NaN in the source
    sample behind the last, in pe row 0 and in the pe rows behind T."""
    lib = _lib.load()
    g = gen(B * 100 + C * 10 + T)
    ldw = 32 if C < 32 else 40
    rows = B * rps + 2
    tag = f"mfcc_project B={B} Bsrc={Bsrc} C={C} T={T} d={d} rps={rps} off={off} pe={use_pe}"
    bsel = torch.arange(B, device=dev()) % Bsrc
    orow = (torch.arange(B, device=dev())[:, None] * rps + torch.arange(T, device=dev())[None, :] + off).reshape(-1)
    for integer in (True, False):
        mf, W, pe = nans(Bsrc + 1, C, T), nans(d, ldw), nans(T + 3, d)
        if integer:
            mf[:Bsrc], W[:, :C] = randint(g, -8, 8, Bsrc, C, T), randint(g, -8, 8, d, C)
            bias, pe[1:T + 1] = randint(g, -64, 64, d), randint(g, -64, 64, T, d)
        else:
            mf[:Bsrc], W[:, :C] = torch.randn(Bsrc, C, T, device=dev(), generator=g), torch.randn(d, C, device=dev(), generator=g)
            bias, pe[1:T + 1] = torch.randn(d, device=dev(), generator=g), torch.randn(T, d, device=dev(), generator=g)
        m, w = mf[bsel].double().permute(0, 2, 1), W[:, :C].double()                   # [B, T, C], [d, C]
        ref, mag = m @ w.t() + bias.double(), m.abs() @ w.abs().t() + bias.double().abs()   # [B, T, d]
        if use_pe:
            ref, mag = ref + pe[1:T + 1].double(), mag + pe[1:T + 1].double().abs()
        ref, mag = ref.reshape(B * T, d), mag.reshape(B * T, d)
        out = nans(rows, d)
        _lib.check(lib.gdx_mfcc_project(vp(mf), vp(W), ldw, vp(bias), vp(pe) if use_pe else None, vp(out), rows, B, Bsrc, C, T,
                                        d, rps, off, stream()), lib)
        assert_rows(out, row_mask(rows, orow), f"{tag} {'int' if integer else 'randn'}")
        got = out[orow].double()
        if integer:
            assert float(mag.max()) < 2 ** 24
            assert torch.equal(got, ref), f"{tag}: integer inputs are not exact, worst |diff| {float((got - ref).abs().max())}"
        else:
            r = float(((got - ref).abs() / ((C + 4) * U * mag)).max())
            print(f"\n[{tag}] worst |got - ref| / bound {r:.3e}")
            assert r <= 1.0, f"{tag}: {r:.3e} of the bound"
        if B > Bsrc:
            first = out[orow[:Bsrc * T]]
            for h in range(1, B // Bsrc):
                assert torch.equal(bits(out[orow[h * Bsrc * T:(h + 1) * Bsrc * T]]), bits(first)), f"{tag}: CFG halves differ"


# ---------------------------------------------------------------------------------------------------------------------
# token0: bit-exact against torch fp32 in the reference's order, (temb + seed_emb) + pe0 and c2 = c2t + c2_seed
T0_SHAPES = [(1, 1, 2, 32), (3, 3, 5, 384), (4, 2, 7, 512)]            # (B, Bsrc, S, d)
T0_OUTPUTS = [(F32, 0), (F16, 0), (F16, 1), (BF16, 0), (BF16, 1)]      # (dtype, enc16 given)


def run_token0(lib, temb, tstride, seed, pe0, c2t, c2s, state, B, Bsrc, S, d, dtype, want16, use_c2, what):
    rows = B * S + 2
    enc, enc16, c2 = nans(rows, d), nans(rows, d) if want16 else None, nans(B + 2, d) if use_c2 else None
    _lib.check(lib.gdx_token0(vp(temb), tstride, vp(seed), vp(pe0), vp(enc), vp(enc16), rows, vp(c2t) if use_c2 else None,
                              vp(c2s) if use_c2 else None, vp(c2), B + 2, vp(state), B, Bsrc, S, d, dtype, stream()), lib)
    tok = row_mask(rows, torch.arange(B, device=dev()) * S)               # only row 0 of each sample's S rows
    assert_rows(enc, tok, f"{what} enc")
    if want16:
        assert_rows(enc16, tok, f"{what} enc16")
        assert_rounded(enc16[tok], enc[tok], dtype, what)
    if use_c2:
        assert_rows(c2, row_mask(B + 2, slice(0, B)), f"{what} c2")
    return enc[tok], c2[:B] if use_c2 else None


@pytest.mark.parametrize("shared", [0, 1], ids=["tstride_d", "tstride_0"])
@pytest.mark.parametrize("B,Bsrc,S,d", T0_SHAPES)
def test_token0_bit_exact(B, Bsrc, S, d, shared):
    """enc[b*S] = (temb[(b % Bsrc) * tstride] + seed_emb[b]) + pe0 and c2[b] = c2t[(b % Bsrc) * tstride] + c2_seed[b], bit for
    bit, with tstride d (a row per source sample; the rows behind the last, up to row B, are NaN) or 0 (one row for the batch), with and
    without pe0, with and without the c2 triple, in fp32 and, for fp16 and bf16, with and without the 16-bit copy (= enc
    rounded, bit for bit).  Rows 1..S-1 of every sample stay NaN in enc and enc16."""
    lib = _lib.load()
    g = gen(B * 10 + S + d + shared)
    rnd = lambda *s: torch.randn(*s, device=dev(), generator=g)
    trows = 1 if shared else Bsrc
    temb, c2t = torch.cat([rnd(trows, d), nans(B, d)]), torch.cat([rnd(trows, d), nans(B, d)])    # NaN up to row B
    seed, c2s, pe0 = rnd(B, d), rnd(B, d), rnd(d)
    tsel = torch.zeros(B, dtype=torch.long, device=dev()) if shared else torch.arange(B, device=dev()) % Bsrc
    for use_pe in (1, 0):
        ref = temb[tsel] + seed
        if use_pe:
            ref = ref + pe0
        ref2 = c2t[tsel] + c2s
        for use_c2 in (1, 0):
            for dtype, want16 in T0_OUTPUTS:
                what = f"token0 B={B} Bsrc={Bsrc} S={S} d={d} tstride={0 if shared else d} pe0={use_pe} c2={use_c2} {NAME[dtype]} enc16={want16}"
                enc, c2 = run_token0(lib, temb, 0 if shared else d, seed, pe0 if use_pe else None, c2t, c2s, None, B, Bsrc, S, d,
                                     dtype, want16, use_c2, what)
                assert torch.equal(bits(enc), bits(ref)), f"{what}: enc differs"
                if use_c2:
                    assert torch.equal(bits(c2), bits(ref2)), f"{what}: c2 differs"


@pytest.mark.parametrize("k", [0, 5])
@pytest.mark.parametrize("B,Bsrc,S,d", T0_SHAPES)
def test_token0_row_from_device_state(B, Bsrc, S, d, k):
    """The graph-replay path as gdx_sample_loop launches it (denoise_step: the table bases with tstride 0, the row index in
    device memory): state = {k, step number} names row k of a 6-row temb / c2t table for the whole batch."""
    lib = _lib.load()
    g = gen(B + S + d + k)
    rnd = lambda *s: torch.randn(*s, device=dev(), generator=g)
    temb, c2t = torch.cat([rnd(6, d), nans(1, d)]), torch.cat([rnd(6, d), nans(1, d)])
    seed, c2s, pe0 = rnd(B, d), rnd(B, d), rnd(d)
    state = torch.tensor([k, 77], dtype=torch.int32, device=dev())
    for use_c2, pe in ((1, None), (0, pe0)):                               # V2 (c2, no pe0) and V1 (pe0, no c2)
        for dtype, want16 in T0_OUTPUTS:
            what = f"token0 state k={k} B={B} S={S} d={d} c2={use_c2} {NAME[dtype]} enc16={want16}"
            enc, c2 = run_token0(lib, temb, 0, seed, pe, c2t, c2s, state, B, Bsrc, S, d, dtype, want16, use_c2, what)
            ref = temb[k] + seed
            assert torch.equal(bits(enc), bits(ref + pe if pe is not None else ref)), f"{what}: enc differs"
            if use_c2:
                assert torch.equal(bits(c2), bits(c2t[k] + c2s)), f"{what}: c2 differs"


# ---------------------------------------------------------------------------------------------------------------------
# masked_l2 (gdx_masked_l2): out[b] = sum_{j,t} (a - b)^2 mask[b,t] / (J * sum_t mask[b,t])
#   (B, J, T): one element; small and odd; the model's pose shape (J*T far above the 256-thread block); T above the block
ML_SHAPES = [(1, 1, 1), (2, 7, 9), (3, 263, 196), (1, 498, 520)]
ML_MASKS = ["ones", "prefix", "scattered", "one_empty"]


def ml_mask(g, kind, B, T):
    m = torch.zeros(B, T, dtype=torch.uint8, device=dev())
    if kind == "ones":
        m[:] = 1
    elif kind == "prefix":                       # ragged: lengths 1, T/2, T-1 (at least one frame)
        for b in range(B):
            m[b, :max(1, [1, T // 2, T - 1][b % 3])] = 1
    else:
        m = (torch.rand(B, T, device=dev(), generator=g) < 0.5).to(torch.uint8)
        m[:, T // 2] = 1                         # never empty by accident
        if kind == "one_empty":
            m[0] = 0
    return m


def run_masked_l2(lib, a, b, mask, B, J, T):
    out = nans(B + 2)
    _lib.check(lib.gdx_masked_l2(vp(a), vp(b), vp(mask), vp(out), B, J, T, stream()), lib)
    assert bool(torch.isnan(out[B:]).all()), "masked_l2 wrote past out[B]"
    return out[:B]


@pytest.mark.parametrize("kind", ML_MASKS)
@pytest.mark.parametrize("B,J,T", ML_SHAPES)
def test_masked_l2(B, J, T, kind):
    """Integer-valued inputs with a - b in [-2, 2] (sum d^2 <= 4 J T < 2^24, asserted: the sum is exact): the result is one
    correctly rounded fp32 division and equals the float64 quotient rounded to fp32, bit for bit.  Normal-random inputs: within
    (J T + 3) 2^-24 ref of float64 (all terms non-negative: any summation order, plus the difference, the product and the
    division).  A sample with an empty mask is 0/0 = NaN, as in the reference, and only that sample.  A batch gives the same
    bits per sample as batches of one."""
    lib = _lib.load()
    g = gen(B * 1000 + J + T)
    mask = ml_mask(g, kind, B, T)
    empty = mask.sum(1) == 0
    assert bool(empty.any()) == (kind == "one_empty")
    tag = f"masked_l2 B={B} J={J} T={T} mask={kind}"
    assert 4 * J * T < 2 ** 24
    for integer in (True, False):
        if integer:
            a = randint(g, -50, 50, B, J, T)
            b = a - randint(g, -2, 2, B, J, T)
        else:
            a, b = torch.randn(B, J, T, device=dev(), generator=g), torch.randn(B, J, T, device=dev(), generator=g)
        m64 = mask.double()[:, None, :]
        dif = a.double() - b.double()
        num, den = (dif * dif * m64).sum((1, 2)), J * mask.double().sum(1)
        ref = num / den                                                                # NaN where the mask is empty
        got = run_masked_l2(lib, a, b, mask, B, J, T)
        assert torch.equal(torch.isnan(got), empty), f"{tag}: NaN exactly for the sample with an empty mask"
        ok = ~empty
        if integer:
            assert float(dif.abs().max()) <= 2 and float(num.max()) < 2 ** 24
            assert torch.equal(bits(got[ok]), bits(ref[ok].float())), f"{tag}: not the correctly rounded quotient: {got} vs {ref}"
        elif bool(ok.any()):
            r = float(((got[ok].double() - ref[ok]).abs() / ((J * T + 3) * U * ref[ok])).max())
            print(f"\n[{tag}] worst |got - ref| / bound {r:.3e}")
            assert r <= 1.0, f"{tag}: {r:.3e} of the bound"
        for s in range(B if B > 1 else 0):
            one = run_masked_l2(lib, a[s:s + 1].contiguous(), b[s:s + 1].contiguous(), mask[s:s + 1].contiguous(), 1, J, T)
            assert torch.equal(bits(one), bits(got[s:s + 1])), f"{tag}: sample {s} alone gives other bits"
