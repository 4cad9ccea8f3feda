"""The in-kernel noise generator on the CPU: the Random123 known answers for oracle/philox.py's cipher, the float64 restatement
(philox_restatement.py) against the oracle's float32 normal(), the Box-Muller edge rows, the statistics of the key sets the GPU
test draws, and the negative controls: every mutant of philox_restatement.MUTANTS is rejected by the check the restatement's
docstring names for it.  tests/test_gpu_philox.py runs the same comparison functions on the device's draws."""
import itertools

import numpy as np
import pytest

import philox_restatement as P
from oracle import philox as op

# Philox4x32-10 rows of the Random123 known-answer table (kat_vectors): counter | key -> output
KAT = [
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000),
     (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff),
     (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def known_answer_failures(cipher):
    bad = []
    for ctr, key, want in KAT:
        got = cipher(np.array(ctr, dtype=np.uint32), key)
        if [int(v) for v in got] != list(want):
            bad.append((ctr, [hex(int(v)) for v in got]))
    return bad


def test_cipher_reproduces_the_random123_known_answers():
    assert not known_answer_failures(op.philox4x32_10)
    assert not known_answer_failures(P.cipher)
    # vectorised over leading axes as words() uses it
    ctr = np.array([k[0] for k in KAT], dtype=np.uint32)
    assert [int(v) for v in op.philox4x32_10(ctr[None, 2:3], KAT[2][1])[0, 0]] == list(KAT[2][2])


def test_words_keying_is_the_oracles():
    """counter = (group, step, sample lo, sample hi) with sample = sample_offset + b carried in 64 bits, key = (seed lo, seed hi)."""
    seed, off, step = 0x0123456789abcdef, 2 ** 32 - 2, 0x80000001
    w = P.words(4, 9, seed, off, step)
    assert w.shape == (4, 3, 4) and w.dtype == np.uint32
    for b, g in itertools.product(range(4), range(3)):
        s = off + b
        ctr = np.array([g, step, s & 0xffffffff, s >> 32], dtype=np.uint32)
        assert np.array_equal(w[b, g], op.philox4x32_10(ctr, (0x89abcdef, 0x01234567))), (b, g)
    assert len({tuple(r) for r in w.reshape(-1, 4).tolist()}) == 12


def _grid(shapes):
    for shape in shapes:
        per = int(np.prod(shape[1:]))
        for seed, off, step in itertools.product(P.SEEDS, P.OFFSETS, P.STEPS):
            yield P.batch_of(off, shape), per, seed, off, step


def test_k_is_four_times_the_oracles_own_float32_error():
    """The unit of the bound, measured: the oracle's float32 normal() against normal64 over every key set and shape of the GPU
    comparison.  K stays 4 x the recorded figure (3.503 with the numpy this was written against); numpy's float32 log / cos /
    sin differ by an ulp between instruction sets, so what is measured here may move, but must stay within half of K."""
    worst = {}
    for b, per, seed, off, step in _grid(P.SHAPES):
        z, r = P.reference(b, per, seed, off, step)
        got = op.normal(b, per, seed, off, step)
        assert got.shape == z.shape == (b, per)
        worst[per] = max(worst.get(per, 0.0), float(P.error_units(got, z, r).max()))
    print("philox-k cpu float32 oracle, worst error in units of 2^-24 max(r, 2^-12) by per-sample size:", worst)
    assert P.K == 4 * P.K_CPU_MEASURED
    assert P.K_GPU_MEASURED <= P.K_CPU_MEASURED
    assert max(worst.values()) <= P.K / 2


def test_second_sample_of_a_tail_shape_starts_a_fresh_group_zero():
    """63 elements per sample: sample b's element 0 is group 0 slot 0 of sample sample_offset + b, whatever the tail before."""
    z, _ = P.reference(5, 63, 7, 2 ** 32 - 3, 9)
    for b in range(5):
        one, _ = P.reference(1, 4, 7, 2 ** 32 - 3 + b, 9)
        assert np.array_equal(z[b, :4], one[0])


@pytest.mark.parametrize("step,group,slot,word,what", P.EDGES)
def test_edge_rows_hold_the_words_the_table_states(step, group, slot, word, what):
    w = P.words(1, P.EDGE_PER, P.EDGE_SEED, 0, step)
    assert int(w[0, group, slot]) == word
    z, r = P.reference(1, P.EDGE_PER, P.EDGE_SEED, 0, step)
    z, r = z[0], r[0]
    e = 4 * group + 2 * (slot // 2)
    want = P.edge_expectation(step, group, slot)
    if what == "u0 = 1":
        assert want == ("zero", "zero") and r[e] == 0 and z[e] == 0 and z[e + 1] == 0
    elif what == "u0 = 2^-24":
        assert want is None and abs(r[e] - P.R_MAX) < 1e-12 and P.R_MAX < P.Z_MAX
    elif what == "angle 0":
        assert want == ("radius", "zero") and z[e] == r[e] and z[e + 1] == 0
    else:                                           # fl32(2pi_f32 (1 - 2^-24)): one float32 step below 2pi_f32
        assert want is None
        a = np.float32(P.TWO_PI_F32 * np.float32(1 - 2.0 ** -24))
        assert a == np.nextafter(P.TWO_PI_F32, np.float32(0)) and (word >> 8) == 2 ** 24 - 1
        assert 0 < -z[e + 1] < 1e-6 * r[e]
    # the oracle's float32 path passes the checks the device's row is given
    assert not P.edge_failures(op.normal(1, P.EDGE_PER, P.EDGE_SEED, 0, step)[0], step, group, slot)
    assert not P.edge_failures(op.normal(1, P.EDGE_PER - 1, P.EDGE_SEED, 0, step)[0], step, group, slot)


@pytest.fixture(scope="module")
def stat_draws():
    return [P.stat_draw(key, lambda *a: P.reference(*a)[0]) for key in P.STAT_KEYS]


@pytest.mark.parametrize("i", range(len(P.STAT_KEYS)))
def test_statistics_of_the_restatement_at_the_chosen_key_sets(stat_draws, i):
    """The conditions of stat_figures follow from N; the key sets were chosen so that the float64 restatement meets them."""
    flat = stat_draws[i]
    assert flat.size == 2 ** 20
    fig = P.stat_figures(flat)
    print(f"philox-stat cpu {P.STAT_KEYS[i]}:", {k: round(v, 2) for k, (v, _) in fig.items()})
    assert not P.stat_failures(flat)


def test_ks_distance_against_a_hand_case():
    """Three points at the quartiles of Phi: F_n jumps by 1/3 at each, D = max over both sides of each jump."""
    x = np.array([-0.6744897501960817, 0.0, 0.6744897501960817])
    assert abs(P.ks_distance(x) - 0.25) < 1e-12      # at x = -0.674: Phi = 1/4 against F_n = 0 before the jump


# ------------------------------------------------------------------------------------------------------- negative controls
EXPECTED = {
    "nine_rounds": "known answers", "key_not_advanced": "known answers", "w1_off_by_one": "known answers",
    "hi_lo_exchanged": "known answers", "group_step_exchanged": "bound", "sample_hi_dropped": "bound",
    "sample_wraps_32": "bound", "shift_9": "bound", "u0_plus_one_missing": "edge rows", "angle_from_u0": "bound",
    "sin_is_cos": "bound",
}
ALSO_STATISTICS = ["shift_9", "angle_from_u0", "sin_is_cos"]


def _bound_catches(mutant):
    """(key sets of the small tail shape at which the mutant's float32 draw leaves the bound, all of them)"""
    caught, n = [], 0
    for b, per, seed, off, step in _grid(P.SHAPES[:1]):
        z, r = P.reference(b, per, seed, off, step)
        got = P.reference(b, per, seed, off, step, mutant)[0].astype(np.float32)
        n += 1
        if not P.within_bound(got, z, r):
            caught.append((seed, off, step))
    return caught, n


def _edge_catches(mutant):
    caught = []
    for step, group, slot, _, what in P.EDGES:
        with np.errstate(invalid="ignore", over="ignore"):
            row = P.reference(1, P.EDGE_PER, P.EDGE_SEED, 0, step, mutant)[0][0].astype(np.float32)
        bad = P.edge_failures(row, step, group, slot)
        if bad:
            caught.append((what, slot, bad))
    return caught


def test_the_unmutated_restatement_passes_every_check():
    assert _bound_catches(None)[0] == [] and _edge_catches(None) == []


@pytest.mark.parametrize("mutant", P.MUTANTS)
def test_the_checks_reject_the_mutant(mutant):
    assert set(EXPECTED) == set(P.MUTANTS)
    by = {}
    if known_answer_failures(lambda c, k: P.cipher(c, k, mutant)):
        by["known answers"] = True
    bound, n = _bound_catches(mutant)
    if bound:
        by["bound"] = f"{len(bound)} of {n} key sets"
    edges = _edge_catches(mutant)
    if edges:
        by["edge rows"] = [(what, slot) for what, slot, _ in edges]
    if mutant in ALSO_STATISTICS:
        bad = P.stat_failures(P.stat_draw(P.STAT_KEYS[0], lambda *a: P.reference(*a, mutant)[0]))
        if bad:
            by["statistics"] = bad[:4]
    print(f"philox-mutant {mutant}: rejected by {by}")
    assert EXPECTED[mutant] in by, by
    if mutant in ALSO_STATISTICS:
        assert "statistics" in by
    if mutant == "u0_plus_one_missing":                       # log(0) at the u = 2^-24 rows
        hit = [bad for what, _, bad in edges if what == "u0 = 2^-24"]
        assert len(hit) == 2 and all("non-finite value" in bad for bad in hit)
    if mutant == "sample_hi_dropped":
        assert all(off >= 2 ** 32 - 3 for _, off, _ in bound) and {off for _, off, _ in bound} == set(P.OFFSETS[1:])
    if mutant == "sample_wraps_32":
        assert {off for _, off, _ in bound} == {2 ** 32 - 3}
