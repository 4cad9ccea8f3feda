"""Kernel-level tests of the fp32 encoder self-attention -- attention_kernel<HD> (csrc/attention.hip, every head width, any
S) and attention3_kernel<HD, PERSIST> (csrc/attention3.hip, widths 64 / 128 up to 256 tokens, item-resident and persistent)
-- through the test entry point gdx_attention_f32_rows, which forces one kernel on exactly the caller's rows (no hidden pad,
the whole ctx copied back) and reports what ran.  Need an MI355X.

Every case is compared with a float64 softmax attention on the same fp32 inputs, and every element is held to

    |ctx - ref| <= A_MAX u (D + sqrt(S) + 4) w,    u = 2^-24,
    w = sum_j p_j |v_j|  (per row, head, column),    D = max_j sum_e |q_e k_je| / sqrt(hd)  (per row, head)

u D: the rounding of an hd-term fp32 dot product as it passes through exp; u sqrt(S): the P V and row-sum accumulation; 4: exp,
the normalisation and the per-tile rescale.  A_MAX is not taken from the kernels: REF_A_WORST is the worst statistic
A = max err / (u (D + sqrt(S) + 4) w) of a plain one-pass torch-fp32 attention (reference32 below) over every case of this
file, computed on the CPU by `python tests/test_gpu_attention_f32.py` (no GPU needed), and A_MAX is twice that: the factor 2
is for the kernels' other summation order (hd-long chains of k = 2 / k = 4 MFMA steps, the tile-by-tile online softmax, the
four-way merge of the shared last block).

The whole-output bound max|err| / max|ref| < 2e-6 of the older tests (tests/test_gpu_parity.py, tests/test_gpu_heads.py) is
kept at every (head width, S) at which they assert it (STRICT below), on every case of this file with that pair, whatever its
batch, head count, seed or data kind; at width 32, width 256 and the other sequence lengths, where the plain fp32 reference
itself goes past 2e-6, the bound is twice the fp32 reference's own value on the same inputs, floored at 1e-6.  That reference
is torch on the host's CPU, so the second bound moves with the host's BLAS (on two hosts its value at hd 256, S = 255 was
9.2e-7 and 2.45e-6); the per-element bound and the 2e-6 do not.
What the 2e-6 found: attention3 at hd 128 with one 32-MFMA score chain measured 2.12e-6 at B = 3, S = 197, H = 2 on this
file's seed (the plain fp32 reference: 1.61e-6); it now accumulates the scores in two chains and measures 7.5e-7 there.

Every check prints "[attn32-measure] <case>: A ... rel ..." for the kernel and for the fp32 reference;
profiles/attention_f32_bounds.txt keeps the worst values per kernel and width.
"""
import ctypes as C
import functools
import math
import os
import sys

import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

from gesturediffusion_amd import _lib

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
# worst A of reference32 over every case of this file (python tests/test_gpu_attention_f32.py: the random sweep's 2.65 at
# hd = 192, S = 32; 2.29 at hd 256, 2.00 at 128, <= 1.5 at 32 / 64 / 96; block counts 1.63, edges 2.30, many-workgroup cases
# 2.09; ramps <= 0.36, uniform <= 0.25, peaked 0)
REF_A_WORST = 2.65
A_MAX = 2.0 * REF_A_WORST
GEN, A3, A3P = 1, 3, 5                       # gdx_attention_f32_rows kernels; 0 = the forward's choice
KNAME = {0: "dispatch", GEN: "attention", A3: "attention3", A3P: "attention3p"}
PAD = 64                                     # attention3 stages whole 64-key tiles: readable rows past B*S
JUNK = 1.0e18                                # large finite pad values: masked by select, and 0 x junk is 0
WIDTHS = [32, 64, 96, 128, 192, 256]
# every (hd, S) at which an older test holds the kernels to 2e-6 on Q x 3 data: test_fp32_attention_vs_torch (hd 128 and 64),
# test_fp32_attention_heads_vs_fp64 (96 / 192).  Every case of this file at one of these pairs keeps the 2e-6, whatever its
# batch, head count and seed.
STRICT = ({(128, S) for S in (1, 16, 61, 65, 129, 197, 201, 241, 256)} | {(64, 81), (64, 197)}
          | {(hd, S) for hd in (96, 192) for S in (1, 16, 31, 33, 65, 128, 197)})


def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


def vp(t):
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(t):
    return t.contiguous().view(torch.int32)


def a3_ok(S, hd):
    """attention3_supported (csrc/attention3.hip)"""
    return hd in (64, 128) and (S + 15) // 16 <= 16


def heads(qkv, B, S, H, d, dtype):
    r = qkv[:B * S].to(dtype).view(B, S, 3, H, d // H)
    return (r[:, :, i].transpose(1, 2) for i in range(3))


def reference(qkv, B, S, H, d):
    """float64 softmax attention on the fp32 inputs, on qkv's device: ref and the per-element unit u (D + sqrt(S) + 4) w of the
    bound, both [B*S][d]."""
    hd = d // H
    q, k, v = heads(qkv, B, S, H, d, torch.float64)
    p = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(hd), dim=-1)
    ref = (p @ v).transpose(1, 2).reshape(B * S, d)
    w = p @ v.abs()                                                             # [B][H][S][hd]
    D = (q.abs() @ k.abs().transpose(-1, -2)).amax(dim=-1, keepdim=True) / math.sqrt(hd)
    unit = (U * (D + math.sqrt(S) + 4.0) * w).transpose(1, 2).reshape(B * S, d)
    return ref, unit


def reference32(qkv, B, S, H, d):
    """The plain reference that A_MAX and the whole-output bound are taken from: one-pass torch-fp32 attention on the CPU."""
    hd = d // H
    q, k, v = heads(qkv.cpu(), B, S, H, d, torch.float32)
    p = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(hd), dim=-1)
    return (p @ v).transpose(1, 2).reshape(B * S, d)


def stats(got, ref, unit):
    """(A, max-normalised error, |got - ref|) of one output"""
    err = (got.double() - ref).abs()
    a = float((err / unit.clamp_min(1e-300)).max())
    rel = float(err.max()) / max(float(ref.abs().max()), 1e-300)
    return a, rel, err


class Case:
    """One input with its references, computed once and shared by every kernel run on it."""

    def __init__(self, what, qkv, B, S, H, d, device=None):
        self.what, self.B, self.S, self.H, self.d = what, B, S, H, d
        self.strict = (d // H, S) in STRICT                                      # the older tests' 2e-6 holds at this shape
        device = device or dev()
        on = qkv.to(device)
        self.ref, self.unit = reference(on, B, S, H, d)
        r32 = reference32(qkv, B, S, H, d).to(device)
        self.a32, self.rel32, _ = stats(r32, self.ref, self.unit)
        print(f"[attn32-measure] {what} fp32-reference: A {self.a32:.3f} rel {self.rel32:.2e}")
        g = torch.Generator().manual_seed(B * 7 + S)
        junk = (torch.rand(PAD, 3 * d, generator=g) * 2 - 1) * JUNK
        self.padded = torch.cat([qkv, junk]).to(device)                          # [B*S + 64][3d], junk behind the samples
        self.exact = on                                                          # [B*S][3d]


def run(qkv, B, S, H, d, kernel, grid=0):
    """One gdx_attention_f32_rows call on qkv (fp32 device [qkv_rows][3d]) into a ctx of NaN rows with three sentinel rows of small
    integers behind B*S.  Every row below B*S must come back finite, the sentinel rows unchanged, and the report must name the
    forced kernel, grid and the item count.  Returns the B*S rows and the report (kernel, grid, items)."""
    lib = _lib.load()
    rows = B * S
    ctx = torch.full((rows + 3, d), float("nan"), device=qkv.device)
    sent = (torch.arange(3 * d, device=qkv.device) % 7 + 1).float().view(3, d)
    ctx[rows:] = sent
    rep = (C.c_int32 * 3)()
    _lib.check(lib.gdx_attention_f32_rows(vp(qkv), qkv.shape[0], vp(ctx), ctx.shape[0], B, S, H, d, kernel, grid, rep, stream()),
               lib)
    what = f"{KNAME[kernel]} B={B} S={S} H={H} d={d} grid={grid}"
    if kernel:
        assert rep[0] == kernel, f"{what}: kernel {rep[0]} ran"
    if grid:
        assert rep[1] == grid, f"{what}: grid {rep[1]}"
    assert rep[2] == B * H, f"{what}: {rep[2]} items"
    assert bool(torch.isfinite(ctx[:rows]).all()), f"{what}: a row below B*S holds a non-finite value"
    assert torch.equal(ctx[rows:], sent), f"{what}: a sentinel row past B*S was written"
    return ctx[:rows], tuple(rep)


def check(got, ref, unit, rel32, what, strict=False):
    """The per-element bound on every element and the whole-output one; prints and returns the measured (A, rel)."""
    a, rel, err = stats(got, ref, unit)
    print(f"[attn32-measure] {what}: A {a:.3f} rel {rel:.2e}")
    bad = err > A_MAX * unit
    if bool(bad.any()):
        i = int(bad.view(-1).nonzero()[0])
        raise AssertionError(f"{what}: |ctx - ref| {float(err.view(-1)[i]):.3e} > bound {A_MAX * float(unit.view(-1)[i]):.3e} at "
                             f"element {i} (ref {float(ref.view(-1)[i]):.4e}; {int(bad.sum())} elements, A {a:.2f})")
    tol = 2e-6 if strict else max(2.0 * rel32, 1e-6)
    assert rel < tol, f"{what}: max|err| / max|ref| {rel:.2e}, bound {tol:.2e} (fp32 reference {rel32:.2e})"
    return a, rel


def kernels(S, hd, nitems):
    """(kernel, grid) pairs that take the shape: the general kernel, and attention3 item-resident, persistent (two grids) and as the
    forward's choice"""
    ks = [(GEN, 0)]
    if a3_ok(S, hd):
        ks += [(A3, 0), (0, 0)] + [(A3P, g) for g in sorted({1, nitems - 1}) if 0 < g < nitems]
    else:
        ks += [(0, 0)]
    return ks


def run_all(case, extra=None):
    """Every kernel that takes the case's shape, on the junk-padded rows: each within the bounds; the forward's choice gives the
    bits of the kernel it reports; attention3's forms all give identical bits.  extra(got, what) adds a probe's own check."""
    c = case
    outs = {}
    for k, grid in kernels(c.S, c.d // c.H, c.B * c.H):
        got, rep = run(c.padded, c.B, c.S, c.H, c.d, k, grid)
        what = f"{c.what} {KNAME[k]}" + (f" grid={grid}" if grid else "")
        if k == 0:
            assert rep[0] == (A3 if a3_ok(c.S, c.d // c.H) else GEN), f"{what}: the forward's choice ran kernel {rep[0]}"
            assert torch.equal(bits(got), outs[rep[0]]), f"{what}: differs in bits from kernel {rep[0]} forced"
            continue
        if k == A3P:
            assert torch.equal(bits(got), outs[A3]), f"{what}: differs in bits from the item-resident form"
            continue
        check(got, c.ref, c.unit, c.rel32, what, c.strict)
        if extra:
            extra(got, what)
        outs[k] = bits(got)
    return outs


# ---------------------------------------------------------------------------------------------------------------------
# case builders: data is made on the CPU from seeded generators, so that the fp32 reference's A can be taken without a GPU
def random_qkv(B, S, d, seed, qscale=3.0):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B * S, 3 * d, generator=g)
    qkv[:, :d] *= qscale                       # sharper softmax than unit-variance scores
    return qkv


# one to five workgroups per item, 1 to 17 K/V tiles, masked tails of 1 and 31 keys, a last workgroup with one, two and four
# active waves (129 / 257 / 385: one; 300: two; 127 / 255 / 521 ...)
SWEEP_S = [1, 16, 31, 32, 33, 127, 128, 129, 255, 256, 257, 300, 385, 521]


def sweep_cases(hd):
    for S in SWEEP_S:
        B, H = 2 + S % 2, 2
        yield f"sweep hd={hd} S={S}", random_qkv(B, S, H * hd, seed=S * 10 + hd), B, S, H, H * hd


def block_cases(hd):
    """the data of test_fp32_attention3_every_block_count (tests/test_gpu_parity.py): Q x 2, B = 3, H = 2"""
    for k in range(1, 17):
        for S in (16 * k - 15, 16 * k - 3):
            yield f"blocks hd={hd} S={S}", random_qkv(3, S, 2 * hd, seed=1000 * hd + S, qscale=2.0), 3, S, 2, 2 * hd


PROBE_S = [1, 33, 64, 77, 197, 256, 300, 521]


def uniform_cases(hd):
    """Q = 0: every key has the same score, so ctx is the column mean of V over exactly the sample's S keys (D = 0: only the
    additive terms of the bound act).  K is random."""
    B, H = 3, 2
    d = H * hd
    for S in PROBE_S:
        qkv = random_qkv(B, S, d, seed=S + hd, qscale=0.0)
        yield f"uniform hd={hd} S={S}", qkv, B, S, H, d


def peak_positions(S):
    """first key, last key, the last key of a full tile and the first key of the masked tail tile, for 32-key (attention.hip)
    and 64-key (attention3.hip) tiles"""
    pos = {0, S - 1}
    for T in (32, 64):
        t = T * ((S - 1) // T)                 # first key of the last tile
        if S % T and t > 0:
            pos |= {t - 1, t}
    return sorted(pos)


def peaked_qkv(B, S, H, hd, rot, seed):
    """K rows are random +-1 vectors; every query of item (b, h) is c K[t] for the item's target t = positions[(b H + h + rot) %
    n], with c such that the target's score leads every other key's by 40: p of every other key is below e^-40, so ctx is
    V[t].  |V| lies in [0.5, 2).  Returns qkv and the targets' V rows as [B*S][d]."""
    g = torch.Generator().manual_seed(seed)
    pos = peak_positions(S)
    K = torch.randint(0, 2, (B, S, H, hd), generator=g).float() * 2 - 1
    V = (torch.rand(B, S, H, hd, generator=g) * 1.5 + 0.5) * (torch.randint(0, 2, (B, S, H, hd), generator=g).float() * 2 - 1)
    Q = torch.empty_like(K)
    want = torch.empty_like(V)
    for b in range(B):
        for h in range(H):
            t = pos[(b * H + h + rot) % len(pos)]
            dots = K[b, :, h] @ K[b, t, h]
            dots[t] = -hd
            c = 40.0 * math.sqrt(hd) / (hd - float(dots.max())) * 1.02       # lead = c (hd - k_j . k_t) / sqrt(hd) >= 40.8
            Q[b, :, h] = c * K[b, t, h]
            want[b, :, h] = V[b, t, h]
    d = H * hd
    return torch.cat([Q.reshape(B * S, d), K.reshape(B * S, d), V.reshape(B * S, d)], dim=1), want.reshape(B * S, d)


def peaked_cases(hd):
    B, H = 2, 2
    for S in [1, 13, 45, 96, 197, 256, 300, 521]:
        for rot in range(len(peak_positions(S))):
            qkv, want = peaked_qkv(B, S, H, hd, rot, seed=S * 3 + hd + rot)
            yield f"peaked hd={hd} S={S} rot={rot}", qkv, B, S, H, H * hd, want


RAMP_STEPS = [3.0, 9.5, 10.5, 25.0]


def ramp_qkv(B, S, H, hd, step, descending, seed):
    """Q[:, 0] = sqrt(hd) and 0 elsewhere, K[:, 0] = step * (the key's 16-key block, counted from the other end if descending):
    the score is the block's level, the same for every query.  K's other columns and V are random."""
    g = torch.Generator().manual_seed(seed)
    nblk = (S + 15) // 16
    blk = torch.arange(S) // 16
    level = step * (nblk - 1 - blk if descending else blk).float()
    Q = torch.zeros(B, S, H, hd)
    K = torch.randn(B, S, H, hd, generator=g)
    Q[..., 0] = math.sqrt(hd)
    K[..., 0] = level.view(1, S, 1)
    V = torch.randn(B, S, H, hd, generator=g)
    d = H * hd
    return torch.cat([Q.reshape(B * S, d), K.reshape(B * S, d), V.reshape(B * S, d)], dim=1)


def ramp_cases(hd, step):
    B, H = 2, 2
    for S in [45, 200, 256, 521]:
        for desc in (False, True):
            yield (f"ramp {step:g} {'descending' if desc else 'ascending'} hd={hd} S={S}",
                   ramp_qkv(B, S, H, hd, step, desc, seed=S + hd + int(step)), B, S, H, H * hd)


# a partial last query block / wave / workgroup at every width: 45 (13 rows), 197 (5), 300, 29, 521 (9), 129 (1), 257 (1), 256;
# (197, 128), (197, 64) and (81, 64) are shapes of the older tests (STRICT)
EDGES = [(3, 45, 2, 64), (3, 197, 2, 128), (3, 300, 1, 256), (3, 29, 2, 32), (3, 521, 2, 128), (3, 129, 2, 96), (3, 257, 1, 192),
         (3, 256, 2, 64), (3, 197, 2, 64), (3, 81, 2, 64)]


def edge_cases():
    for B, S, H, hd in EDGES:
        yield f"edges B={B} S={S} H={H} hd={hd}", random_qkv(B, S, H * hd, seed=S + 5 * hd), B, S, H, H * hd


MANY = [(66, 197, 4, 128), (66, 197, 4, 256)]                 # more (sample, head) items than CUs


def dispatch_shape(cus, short):
    """width 128 at one head: B items; 2 CUs of them make launch_attention3 go persistent, one fewer does not"""
    return (2 * cus - (1 if short else 0), 17, 1, 128)


def many_cases(cus=256):
    for B, S, H, hd in MANY + [dispatch_shape(cus, False), dispatch_shape(cus, True)]:
        yield f"many B={B} S={S} H={H} hd={hd}", random_qkv(B, S, H * hd, seed=B + S + hd), B, S, H, H * hd


@functools.lru_cache(maxsize=None)
def num_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd", WIDTHS)
def test_attention_f32_general_sweep(hd):
    """attention_kernel at every width and every S of SWEEP_S on Q x 3 data (and attention3's three forms where they take the
    shape): per-element bound, whole-output bound (2e-6 at the shapes of the older tests), sentinels, the forward's choice."""
    for what, qkv, B, S, H, d in sweep_cases(hd):
        run_all(Case(what, qkv, B, S, H, d))


@pytest.mark.parametrize("hd", [64, 128])
def test_attention_f32_attention3_every_block_count(hd):
    """attention3 at every query-block count 1..16 (S = 16k - 15 and 16k - 3, the data of
    test_fp32_attention3_every_block_count) with the per-element bound and that test's 2e-6: item-resident, the forward's choice
    and the persistent form at grids 1, 2 and B H - 1 all give identical bits."""
    for what, qkv, B, S, H, d in block_cases(hd):
        c = Case(what, qkv, B, S, H, d)
        got, _ = run(c.padded, B, S, H, d, A3)
        check(got, c.ref, c.unit, c.rel32, f"{what} attention3", strict=True)
        base = bits(got)
        for k, grid in [(0, 0), (A3P, 1), (A3P, 2), (A3P, B * H - 1)]:
            got, rep = run(c.padded, B, S, H, d, k, grid)
            assert rep[0] == (k or A3), f"{what}: kernel {k} reported {rep}"
            assert torch.equal(bits(got), base), f"{what}: {KNAME[k]} at grid {grid} differs in bits from the item-resident form"
        got, _ = run(c.padded, B, S, H, d, GEN)
        check(got, c.ref, c.unit, c.rel32, f"{what} attention", c.strict)


@pytest.mark.parametrize("hd", WIDTHS)
def test_attention_f32_uniform_probe(hd):
    """Q = 0 on every kernel: ctx is the column mean of V (the float64 reference is checked to be that mean), within the bound's
    additive terms alone."""
    for what, qkv, B, S, H, d in uniform_cases(hd):
        c = Case(what, qkv, B, S, H, d)
        mean = qkv[:, 2 * d:].double().view(B, S, d).mean(dim=1, keepdim=True).expand(B, S, d).reshape(B * S, d).to(c.ref.device)
        assert float((c.ref - mean).abs().max()) < 1e-14, what
        run_all(c)


@pytest.mark.parametrize("hd", WIDTHS)
def test_attention_f32_peaked_probe(hd):
    """One key leads by 40 in score -- the first key, the last key, the last key of a full tile, the first key of the masked
    tail tile, rotated over the (sample, head) items: ctx equals that key's V row within 4 u |v|, besides the bound."""
    for what, qkv, B, S, H, d, want in peaked_cases(hd):
        c = Case(what, qkv, B, S, H, d)
        want = want.double().to(c.ref.device)

        def is_v_row(got, what):
            err = (got.double() - want).abs()
            assert bool((err <= 4 * U * want.abs()).all()), \
                f"{what}: not the target key's V row (max |err| / |v| {float((err / want.abs()).max()):.2e})"
        run_all(c, extra=is_v_row)


@pytest.mark.parametrize("hd", WIDTHS)
@pytest.mark.parametrize("step", RAMP_STEPS)
def test_attention_f32_ramp_probes(step, hd):
    """The score depends on the key's 16-key block only and rises (or falls) by `step` per block.  attention3 moves its running
    max only when a block exceeds it by more than 10: a rise of 3 crosses that every fourth block, 9.5 every second one (with p up
    to e^9.5 in between), 10.5 at every block and 25 by a wide margin; descending, the first block holds the max and no later
    one moves it.  attention_kernel rescales by alpha = exp(-32 step ...) per tile.  Scores reach 800: nothing may overflow."""
    for what, qkv, B, S, H, d in ramp_cases(hd, step):
        run_all(Case(what, qkv, B, S, H, d))


@pytest.mark.parametrize("B,S,H,hd", EDGES)
def test_attention_f32_edges_and_sample_independence(B, S, H, hd):
    """With each kernel forced: 1e18 junk in the 64 rows behind the samples gives the bits that zeros there give; every sample of
    the B = 3 call is bit-equal to a B = 1 call on that sample alone; attention_kernel, which clamps, takes qkv_rows = B*S exactly
    and gives the same bits again.  (run() holds the sentinel rows of ctx and the finiteness of every row below B*S.)"""
    d = H * hd
    what, qkv, *_ = next(c for c in edge_cases() if c[2:5] == (B, S, H) and c[5] == d)
    c = Case(what, qkv, B, S, H, d)
    zero = c.padded.clone()
    zero[B * S:] = 0
    for k, grid in kernels(S, hd, B * H):
        if k == 0:
            continue
        kw = f"{what} {KNAME[k]}"
        got, _ = run(c.padded, B, S, H, d, k, grid)
        check(got, c.ref, c.unit, c.rel32, kw, c.strict)
        base = bits(got)
        got, _ = run(zero, B, S, H, d, k, grid)
        assert torch.equal(bits(got), base), f"{kw}: the junk in the pad rows changed the output"
        if k == GEN:
            got, _ = run(c.exact, B, S, H, d, k)
            assert torch.equal(bits(got), base), f"{kw}: qkv_rows = B*S gives other bits"
        for b in range(B):
            sl = slice(b * S, (b + 1) * S)
            alone = c.exact[sl].contiguous() if k == GEN else torch.cat([c.exact[sl], c.padded[B * S:]])
            k1, g1 = (A3, 0) if k == A3P and H == 1 else (k, min(grid, H - 1))   # one item cannot be walked: item-resident
            got, _ = run(alone, 1, S, H, d, k1, g1)
            assert torch.equal(bits(got), base[sl]), f"{kw}: sample {b} alone differs from sample {b} in the batch"


@pytest.mark.parametrize("B,S,H,hd", MANY)
def test_attention_f32_more_items_than_cus(B, S, H, hd):
    """More (sample, head) items than CUs on each kernel: sample 0, a middle sample and the last one are checked against the
    reference and against the bits of a B = 1 call."""
    d = H * hd
    what, qkv, *_ = next(c for c in many_cases() if c[2:5] == (B, S, H) and c[5] == d)
    many_check(what, qkv, B, S, H, d, [(GEN, 0)] + ([(A3, 0), (0, 0), (A3P, 100)] if a3_ok(S, hd) else [(0, 0)]))


def many_check(what, qkv, B, S, H, d, ks, expect=None):
    on = qkv.to(dev())
    padded = torch.cat([on, torch.full((PAD, 3 * d), JUNK, device=on.device)])
    picks = sorted({0, B // 2, B - 1})
    subs = {b: Case(f"{what} sample {b}", qkv[b * S:(b + 1) * S], 1, S, H, d) for b in picks}
    for k, grid in ks:
        got, rep = run(padded, B, S, H, d, k, grid)
        if expect and k == 0:
            assert rep == expect, f"{what}: the forward's choice ran {rep}, the rule says {expect}"
        for b in picks:
            c = subs[b]
            sl = slice(b * S, (b + 1) * S)
            check(got[sl], c.ref, c.unit, c.rel32, f"{c.what} {KNAME[k]}", c.strict)
            alone, _ = run(c.padded, 1, S, H, d, GEN if rep[0] == GEN else A3)   # (attention3's forms give the same bits)
            assert torch.equal(bits(alone), bits(got[sl])), f"{c.what} {KNAME[k]}: differs in bits from the B = 1 call"


def test_attention_f32_dispatch_goes_persistent_at_two_items_per_cu():
    """kernel = 0 at width 128 and 2 CUs items (S = 17, one head) reports the persistent form on one workgroup per CU; at one
    item fewer the item-resident one.  First, middle and last sample against the reference and their B = 1 bits."""
    cus = num_cus()
    for short in (False, True):
        B, S, H, hd = dispatch_shape(cus, short)
        d = H * hd
        qkv = random_qkv(B, S, d, seed=B + S + hd)
        expect = (A3, B * H, B * H) if short else (A3P, cus, B * H)
        many_check(f"dispatch B={B} S={S} H={H} hd={hd}", qkv, B, S, H, d, [(0, 0)], expect)


# ---------------------------------------------------------------------------------------------------------------------
def reference_a_worst():
    """A of reference32 over every case of this file, on the CPU (the many-workgroup cases by the samples the tests check)."""
    cpu = torch.device("cpu")
    worst = {}

    def take(group, what, qkv, B, S, H, d):
        c = Case(what, qkv, B, S, H, d, device=cpu)
        key = (group, d // H)
        a, r = worst.get(key, (0.0, 0.0))
        worst[key] = (max(a, c.a32), max(r, c.rel32))

    for hd in WIDTHS:
        for args in sweep_cases(hd):
            take("sweep", *args)
        for args in uniform_cases(hd):
            take("uniform", *args)
        for args in peaked_cases(hd):
            take("peaked", *args[:6])
        for step in RAMP_STEPS:
            for args in ramp_cases(hd, step):
                take("ramp", *args)
    for hd in (64, 128):
        for args in block_cases(hd):
            take("blocks", *args)
    for args in edge_cases():
        take("edges", *args)
    for what, qkv, B, S, H, d in many_cases():
        for b in sorted({0, B // 2, B - 1}):
            take("many", f"{what} sample {b}", qkv[b * S:(b + 1) * S], 1, S, H, d)
    for (group, hd), (a, r) in sorted(worst.items()):
        print(f"[attn32-reference] {group:8s} hd={hd:3d}: worst A {a:.3f}, worst rel {r:.2e}")
    print(f"[attn32-reference] REF_A_WORST = {max(a for a, _ in worst.values()):.3f}")


if __name__ == "__main__":
    reference_a_worst()
