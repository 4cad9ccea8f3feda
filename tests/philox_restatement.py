"""The in-kernel noise generator (philox_normal4, csrc/gdx_pose_device.h) restated next to oracle/philox.py: the counter words with
the oracle's keying, Box-Muller with log / sqrt / cos / sin in float64, the per-element bound, the statistics and the key
sets that tests/test_philox_host.py (CPU) and tests/test_gpu_philox.py (GPU) share, and the mutants of the negative
controls.  No GPU code here.

  words()     counter = (group, step, sample lo, sample hi), key = (seed lo, seed hi), sample = sample_offset + b in 64 bits,
              through oracle.philox.philox4x32_10, which the Random123 known answers pin (test_philox_host.py).
  normal64()  u0 = ((w0 >> 8) + 1) 2^-24 and u1 = (w1 >> 8) 2^-24 are exact in float32 (24-bit integers times a power of two);
              the angle fl32(2pi_f32 u1) is the one float32 rounding the kernel performs before its libm calls.  From there on
              float64: r = sqrt(-2 log u0), z = (r cos a, r sin a); slots 2, 3 likewise from w2, w3.
  bound       |got - z| <= K 2^-24 max(r, 2^-12) per element.  Scaled by the radius, not by |z|: next to a zero of cos or sin
              an ulp of 1 times r is all a float32 path can promise.  Any wrong bit in the cipher changes every output word, so
              the bound loses nothing on the integer part; it has to see a wrong libm call or a missing + 1.

Which check catches which mutant (test_philox_host.py::test_the_checks_reject_the_mutant asserts exactly this column; the
other checks that also fail are printed):
  nine_rounds            known answers
  key_not_advanced       known answers
  w1_off_by_one          known answers
  hi_lo_exchanged        known answers
  group_step_exchanged   bound against normal64 (every key set whose step differs from the group index)
  sample_hi_dropped      bound, at sample_offset >= 2^32
  sample_wraps_32        bound, at sample_offset 2^32 - 3 with batch 8 (samples 3 .. 7 lie past the carry)
  shift_9                bound (every uniform halves); the statistics as well
  u0_plus_one_missing    the u0 = 2^-24 edge rows: log(0) -> a non-finite value; the u0 = 1 rows are no longer zero
  angle_from_u0          bound; statistics (z0, z1 are functions of one uniform: KS of the slots)
  sin_is_cos             bound; statistics (slots 0, 1 equal: correlation 1)
"""
import math

import numpy as np
import torch

from oracle import philox as op

U = 2.0 ** -24
R_FLOOR = 2.0 ** -12
TWO_PI_F32 = np.float32(6.28318530717958647692)
R_MAX = math.sqrt(48 * math.log(2))            # u = 2^-24: sqrt(-2 log 2^-24) = 5.76826...
Z_MAX = 5.7684

# Worst |z32 - z64| / (2^-24 max(r, 2^-12)) over SEEDS x OFFSETS x STEPS x SHAPES:
#   oracle/philox.py normal() (numpy float32 libm) on the CPU: 3.503 (the one-sample shape of 262157 elements; 2.41 and 2.93
#                                                              at the two small shapes; 3.197 at seed 123456789012345,
#                                                              sample_offset 2^32 - 3, step 0xfffffffe, 8 x 65536 elements)
#   randn_kernel on an MI355X:                                 3.205 (the same shape, seed 2^64 - 1; 2.53 and 2.94 at the small
#                                                              shapes; test_gpu_philox.py::test_randn_vs_normal64 prints them)
# K is four times the CPU figure, the margin the project gives an fp32 path against its float64 restatement; it was fixed from
# the CPU figure alone, before the device's was known.
K_CPU_MEASURED = 3.51
K_GPU_MEASURED = 3.205
K = 4 * K_CPU_MEASURED

# engine.randn is compared at every combination of these (2a of the issue)
SEEDS = [0, 2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1]
OFFSETS = [0, 2 ** 32 - 3, 2 ** 32, 2 ** 63]
STEPS = [0, 1, 2 ** 31, 2 ** 32 - 1]
BIG = 4 * (65536 + 3) + 1
SHAPES = [(5, 7, 1, 9), (3, 16, 1, 20), (1, BIG)]
CARRY_BATCH = 8                                  # sample_offset 2^32 - 3: batch 8, so that samples 3 .. 7 are past the carry

# The statistics' draws: (seed, sample_offset, first step); STAT_STEPS consecutive steps of STAT_BATCH samples of STAT_PER
# elements = 2^20 values.  Chosen once on the CPU so that normal64 of the oracle passes stat_failures with room
# (test_philox_host.py prints every figure), before anything ran on a GPU.
STAT_KEYS = [(10, 0, 0), (123456789012345, 2 ** 32 - 3, 0xfffffffe), (2 ** 64 - 1, 2 ** 63, 2 ** 31)]
STAT_STEPS, STAT_BATCH, STAT_PER = 2, 8, 65536

# Edge draws, all at seed 10, sample 0: (step, group, slot, word, meaning)
EDGE_SEED = 10
EDGES = [
    (252126, 4, 0, 0xffffff9f, "u0 = 1"),
    (568356, 24, 0, 0x000000f5, "u0 = 2^-24"),
    (918293, 19, 1, 0x00000075, "angle 0"),
    (590545, 16, 1, 0xffffffba, "angle below 2pi"),
    (147022, 9, 2, 0xffffffc0, "u0 = 1"),
    (780990, 6, 2, 0x00000018, "u0 = 2^-24"),
    (740278, 17, 3, 0x000000e4, "angle 0"),
    (686677, 25, 3, 0xffffffd1, "angle below 2pi"),
]
EDGE_PER = 128

CIPHER_MUTANTS = ["nine_rounds", "key_not_advanced", "w1_off_by_one", "hi_lo_exchanged"]
KEYING_MUTANTS = ["group_step_exchanged", "sample_hi_dropped", "sample_wraps_32"]
NORMAL_MUTANTS = ["shift_9", "u0_plus_one_missing", "angle_from_u0", "sin_is_cos"]
MUTANTS = CIPHER_MUTANTS + KEYING_MUTANTS + NORMAL_MUTANTS


def cipher(counter, key, mutant=None):
    """oracle.philox.philox4x32_10, or one of CIPHER_MUTANTS of it."""
    if mutant not in CIPHER_MUTANTS:
        return op.philox4x32_10(counter, key)
    c = [counter[..., i].astype(np.uint32) for i in range(4)]
    k0, k1 = np.uint32(key[0]), np.uint32(key[1])
    w1 = np.uint32(int(op.W1) + 1) if mutant == "w1_off_by_one" else op.W1
    with np.errstate(over="ignore"):
        for _ in range(9 if mutant == "nine_rounds" else 10):
            p0 = op.M0 * c[0].astype(np.uint64)
            p1 = op.M1 * c[2].astype(np.uint64)
            hi0, lo0 = (p0 >> np.uint64(32)).astype(np.uint32), p0.astype(np.uint32)
            hi1, lo1 = (p1 >> np.uint64(32)).astype(np.uint32), p1.astype(np.uint32)
            if mutant == "hi_lo_exchanged":
                hi0, lo0, hi1, lo1 = lo0, hi0, lo1, hi1
            c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
            if mutant != "key_not_advanced":
                k0 = np.uint32(k0 + op.W0)
                k1 = np.uint32(k1 + w1)
    return np.stack(c, axis=-1)


def words(batch, per_sample, seed, sample_offset, step, mutant=None):
    """uint32 [batch, groups, 4]: the cipher's output for every group of every sample, keyed as oracle.philox.normal keys it."""
    assert mutant is None or mutant in MUTANTS
    groups = (per_sample + 3) // 4
    sample = [(sample_offset + b) % 2 ** 64 for b in range(batch)]
    if mutant == "sample_wraps_32":
        sample = [(sample_offset & ~0xFFFFFFFF) | ((sample_offset + b) & 0xFFFFFFFF) for b in range(batch)]
    ctr = np.empty((batch, groups, 4), dtype=np.uint32)
    ctr[..., 0] = np.arange(groups, dtype=np.uint32)
    ctr[..., 1] = np.uint32(step & 0xFFFFFFFF)
    ctr[..., 2] = np.array([s & 0xFFFFFFFF for s in sample], dtype=np.uint32)[:, None]
    ctr[..., 3] = 0 if mutant == "sample_hi_dropped" else np.array([s >> 32 for s in sample], dtype=np.uint32)[:, None]
    if mutant == "group_step_exchanged":
        ctr = ctr[..., [1, 0, 2, 3]]
    return cipher(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF), mutant)


def normal64(w, mutant=None):
    """words [..., groups, 4] -> (z, r), float64 [..., 4 * groups]: the four normals of every group and each one's radius."""
    assert mutant is None or mutant in MUTANTS
    sh = np.uint32(9 if mutant == "shift_9" else 8)
    one = np.uint32(0 if mutant == "u0_plus_one_missing" else 1)
    inv24 = np.float32(U)
    u = [((w[..., 0] >> sh) + one).astype(np.float32) * inv24, (w[..., 1] >> sh).astype(np.float32) * inv24,
         ((w[..., 2] >> sh) + one).astype(np.float32) * inv24, (w[..., 3] >> sh).astype(np.float32) * inv24]
    assert all(v.dtype == np.float32 for v in u)
    out_z, out_r = [], []
    with np.errstate(divide="ignore"):
        for ur, ua in ((u[0], u[1]), (u[2], u[3])):
            r = np.sqrt(-2.0 * np.log(ur.astype(np.float64)))
            a = (TWO_PI_F32 * (ur if mutant == "angle_from_u0" else ua)).astype(np.float32).astype(np.float64)
            out_z += [r * np.cos(a), r * (np.cos(a) if mutant == "sin_is_cos" else np.sin(a))]
            out_r += [r, r]
    flat = w.shape[:-2] + (4 * w.shape[-2],)
    return np.stack(out_z, axis=-1).reshape(flat), np.stack(out_r, axis=-1).reshape(flat)


def reference(batch, per_sample, seed, sample_offset, step, mutant=None):
    """(z, r) float64 [batch, per_sample] of a randn call."""
    z, r = normal64(words(batch, per_sample, seed, sample_offset, step, mutant), mutant)
    return z[:, :per_sample], r[:, :per_sample]


def error_units(got, z, r):
    """|got - z| in units of 2^-24 max(r, 2^-12), per element; a non-finite `got` counts as infinitely far."""
    got = np.asarray(got, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        e = np.abs(got - z) / (U * np.maximum(r, R_FLOOR))
    return np.where(np.isfinite(got), e, np.inf)


def within_bound(got, z, r):
    return bool((error_units(got, z, r) <= K).all())


def batch_of(sample_offset, shape):
    """The batch of a SEEDS x OFFSETS x STEPS case: the shape's own, except CARRY_BATCH at the offset whose batch must cross 2^32."""
    return CARRY_BATCH if sample_offset == 2 ** 32 - 3 and shape[0] > 1 else shape[0]


# ------------------------------------------------------------------------------------------------------------ edge rows
def edge_expectation(step, group, slot):
    """What an edge row of EDGES pins at elements 4*group + 2*(slot // 2) + {0, 1}: ('zero', 'zero'), ('radius', 'zero'), or
    None where only the bound (and, at u = 2^-24, z0^2 + z1^2 = r^2) applies."""
    w = int(words(1, EDGE_PER, EDGE_SEED, 0, step)[0, group, slot])
    if slot % 2 == 0:
        return ("zero", "zero") if (w >> 8) + 1 == 2 ** 24 else None
    return ("radius", "zero") if w >> 8 == 0 else None


def edge_failures(got, step, group, slot):
    """The edge checks on one randn row `got` (float32 [>= 4*group + 4], seed EDGE_SEED, sample 0, draw `step`)."""
    got = np.asarray(got)
    bad = []
    if not np.isfinite(got).all():
        bad.append("non-finite value")
    z, r = reference(1, len(got), EDGE_SEED, 0, step)
    z, r = z[0], r[0]
    if not within_bound(got, z, r):
        bad.append(f"bound: {error_units(got, z, r).max():.3g} units")
    e = 4 * group + 2 * (slot // 2)
    g0, g1 = float(got[e]), float(got[e + 1])
    want = edge_expectation(step, group, slot)
    if want == ("zero", "zero") and not (g0 == 0.0 and g1 == 0.0):
        bad.append(f"radius 0 gives ({g0!r}, {g1!r}), not (+-0, +-0)")
    if want == ("radius", "zero"):
        if g1 != 0.0:
            bad.append(f"sin(0) element is {g1!r}")
        if abs(g0 - float(np.float32(r[e]))) > K * U * max(r[e], R_FLOOR):
            bad.append(f"cos(0) element {g0!r} is not the radius {r[e]!r}")
    if slot % 2 == 0 and r[e] > 5.76:                    # u = 2^-24: the largest radius, squared 48 ln 2
        if abs(r[e] - R_MAX) > 1e-12:
            bad.append("restatement radius")
        # d(z0^2 + z1^2) = 2 (z0 dz0 + z1 dz1) <= 2 r (|dz0| + |dz1|) <= 4 r (K u r)
        if abs(g0 * g0 + g1 * g1 - r[e] ** 2) > 4 * K * U * r[e] ** 2:
            bad.append(f"z0^2 + z1^2 = {g0 * g0 + g1 * g1!r}, r^2 = {r[e] ** 2!r}")
    return bad


# ------------------------------------------------------------------------------------------------------------ statistics
def _phi(x):
    return torch.special.ndtr(torch.from_numpy(np.ascontiguousarray(x))).numpy()


def ks_distance(x):
    """Kolmogorov-Smirnov distance of the sample x to the standard normal distribution function."""
    s = np.sort(np.asarray(x, dtype=np.float64))
    n = len(s)
    f = _phi(s)
    i = np.arange(1, n + 1, dtype=np.float64)
    return float(max((i / n - f).max(), (f - (i - 1) / n).max()))


def _corr(a, b):
    a, b = a.ravel(), b.ravel()
    return float(np.corrcoef(a, b)[0, 1]) * math.sqrt(a.size), a.size


def stat_figures(flat, steps=STAT_STEPS, batch=STAT_BATCH):
    """flat: the draws of `steps` consecutive steps x `batch` consecutive samples x per_sample (a multiple of 4) elements, in
    that order -> {name: (figure, limit)}, every figure in the unit its limit is stated in:
      moments  (m_k - E z^k) / se_k for k = 1 .. 4, per slot (element index mod 4) and pooled; se = 1/sqrt N, sqrt(2/N),
               sqrt(15/N), sqrt(96/N) (the variances of z, z^2, z^3, z^4 under N(0, 1) over N); limit 5.  The moments are
               about 0, not about the sample mean: the claim under test is N(0, 1), whose mean is known.
      ks       sqrt(N) D against Phi; limit 2.2
      corr     correlation x sqrt(number of pairs) of slots (0,1), (2,3), (0,2) of a group, of group g and g+1 (same slot), of
               step k and k+1 and of sample b and b+1 (same element); limit 5
      range    max |z| (limit 5.7684) and the count of non-finite values (limit 0)."""
    z = np.asarray(flat, dtype=np.float64).reshape(steps, batch, -1)
    assert z.shape[2] % 4 == 0
    g = z.reshape(steps, batch, -1, 4)
    fig = {"nonfinite": (float((~np.isfinite(z)).sum()), 0.0)}
    with np.errstate(invalid="ignore"):
        fig["max|z|"] = (float(np.abs(z).max()) if np.isfinite(z).all() else math.inf, Z_MAX)
    if fig["nonfinite"][0]:
        return fig
    for name, v in [("pooled", z.ravel())] + [(f"slot{s}", g[..., s].ravel()) for s in range(4)]:
        n = v.size
        for k, (mean, var) in enumerate([(0.0, 1.0), (1.0, 2.0), (0.0, 15.0), (3.0, 96.0)], start=1):
            fig[f"{name}.m{k}"] = ((float((v ** k).mean()) - mean) / math.sqrt(var / n), 5.0)
        fig[f"{name}.ks"] = (math.sqrt(n) * ks_distance(v), 2.2)
    for a, b in ((0, 1), (2, 3), (0, 2)):
        fig[f"corr.slot{a}{b}"] = (_corr(g[..., a], g[..., b])[0], 5.0)
    fig["corr.group"] = (_corr(g[:, :, :-1, :], g[:, :, 1:, :])[0], 5.0)
    fig["corr.step"] = (_corr(z[:-1], z[1:])[0], 5.0)
    fig["corr.sample"] = (_corr(z[:, :-1], z[:, 1:])[0], 5.0)
    return fig


def stat_failures(flat, steps=STAT_STEPS, batch=STAT_BATCH):
    return [f"{k}: {v:.3g} (limit {lim})" for k, (v, lim) in stat_figures(flat, steps, batch).items() if not abs(v) <= lim]


def stat_draw(key, draw):
    """The flat float64 array of a STAT_KEYS entry, from draw(batch, per_sample, seed, sample_offset, step) -> [batch, per]."""
    seed, off, step0 = key
    return np.concatenate([np.asarray(draw(STAT_BATCH, STAT_PER, seed, off, step0 + k), dtype=np.float64).ravel()
                           for k in range(STAT_STEPS)])
