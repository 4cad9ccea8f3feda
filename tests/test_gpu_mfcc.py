"""The MFCC front end (gdx_mfcc: mfcc_frames / mfcc_power / mfcc_cepstrum kernels of csrc/mfcc.hip and the two fp32 GEMMs in
between) stage by stage against float64, at five geometries and at the signals where such kernels go wrong.  Need an MI355X.

The stages are read from the caller's workspace (MfccExtractor.workspace / stage_views); each is compared on the device's own
output of the stage before it, with the bounds derived in tests/mfcc_restatement.py.  End to end, the unnormalised output is
compared per coefficient with oracle/mfcc.py in float64 throughout.  The two measured constants, L_U (logf) and E2E_BOUND,
are recorded with their margins in profiles/mfcc_stage_tests.txt, which holds the figures every test here prints before it
asserts.  tests/test_mfcc_host.py shows on the CPU that these checks reject eight plausible kernel mistakes.

Every run fills `out` with NaN, carries two sentinel rows behind it and 64 sentinel floats behind the workspace's last used
element, and starts from a workspace full of NaN: the library may ask nothing of its contents.

Still unpinned: agreement with python_speech_features itself (oracle/mfcc.py restates it), and which GEMM kernel a launch took
(G4's N = 8320 is beyond what the persistent kernel accepts; the library does not report the choice through gdx_mfcc).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import mfcc_restatement as mr
from gesturediffusion_amd import _lib
from oracle import mfcc as om

pytestmark = pytest.mark.gpu

NAN = float("nan")
TAIL = 64
STAGES = ("frames", "spec", "pw", "mel", "energy")


def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def setup(name):
    ex = mr.make_extractor(name, dev())
    return ex, mr.Tables(name, ex)


def vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def run(ex, x, mean=None, std=None, fill=NAN, signal=None):
    """One gdx_mfcc call on the fp32 numpy signal x (or the device tensor `signal`) -> the five stages and `out` as numpy.
    Asserts what holds of every call: rows past F and the floats past the workspace untouched, all F rows finite."""
    sig = torch.from_numpy(np.ascontiguousarray(x)).to(dev()) if signal is None else signal
    n = sig.numel()
    F = ex.num_frames(n)
    size = ex.workspace_size(F)
    work = torch.cat([ex.workspace(F, fill=fill), torch.full((TAIL,), NAN, device=dev())])
    out = torch.full((F + 2, ex.numcep), NAN, device=dev())
    d32 = lambda a: None if a is None else torch.tensor(np.asarray(a)[: ex.numcep], dtype=torch.float32, device=dev())   # noqa: E731
    m, s = d32(mean), d32(std)
    lib = _lib.load()
    _lib.check(lib.gdx_mfcc(vp(sig), n, ex.frame_len, ex.frame_step, F, ex.nfft, ex.nfilt, ex.numcep, C.c_float(ex.preemph),
                            vp(ex.dft), vp(ex.mel), vp(ex.dct), vp(ex.lift), vp(m), vp(s), vp(work), vp(out),
                            C.c_void_p(torch.cuda.current_stream().cuda_stream)), lib)
    torch.cuda.synchronize()
    assert bool(torch.isnan(work[size:]).all()), "a float behind the workspace's last used element was written"
    assert bool(torch.isnan(out[F:]).all()), "a row of out behind the last frame was written"
    assert bool(torch.isfinite(out[:F]).all()), "a row of out holds a non-finite value"
    st = {k: v.cpu().numpy().copy() for k, v in zip(STAGES, ex.stage_views(work[:size], F))}
    st["out"] = out[:F].cpu().numpy()
    return st


def fmt(v):
    return " ".join(f"{a:.1e}" for a in np.atleast_1d(v))


def report(label, fig, logf=None, e2e=None):
    line = f"mfcc[{label}] fraction of bound: " + " ".join(f"{k} {fig[k]:.3g}" for k in fig)
    if logf is not None:
        line += f" | logf {logf:.3f} u"
    print(line)
    if e2e is not None:
        print(f"mfcc[{label}] e2e max {float(e2e.max()):.2e} at c{int(np.argmax(e2e))}; per coefficient: {fmt(e2e)}")


def full_check(T, x, st, label, mean=None, std=None, e2e="all", rows=None):
    """Stage checks and (unnormalised runs) the end-to-end check; prints every figure, then asserts."""
    fig, bad = mr.check_stages(T, x, st, mean, std)
    err = None
    if mean is None and e2e is not None:
        err, b = mr.check_e2e(T, x, st["out"], coefs=None if e2e == "all" else e2e, rows=rows)
        bad += b
    report(label, fig, mr.logf_units(st) if mean is None and fig else None, err)
    assert not bad, bad
    return fig


LENGTH_CASES = [(g, i) for g in sorted(mr.GEOMS) for i in range(6)]


@pytest.mark.parametrize("name,i", LENGTH_CASES, ids=[f"{g}-n{i}" for g, i in LENGTH_CASES])
def test_lengths(name, i):
    """White noise (sigma 0.3) of 1, frame_len, frame_len + 1, frame_len + step, frame_len + step + 1 and
    frame_len + 2 step + 1 samples: every stage, every coefficient end to end, the shape against the package's frame count.
    n = 1: the frame is x0 followed by zeros, so the spectrum is x0 in every bin and pw = x0^2 / nfft in closed form."""
    ex, T = setup(name)
    n = mr.lengths(T)[i]
    x = mr.length_noise(T, n)
    st = run(ex, x)
    sr, fps, winlen = mr.GEOMS[name][:3]
    assert st["out"].shape == (om.frame_geometry(n, sr, winlen, 1 / fps)[2], min(mr.GEOMS[name][5], mr.GEOMS[name][3]))
    full_check(T, x, st, f"{name} noise n={n}")
    if n == 1:
        want = float(x[0]) ** 2 / T.nfft
        r = mr.worst_ratio(st["pw"][0, : T.nbins], want, 6 * mr.U * want)
        print(f"mfcc[{name} n=1] pw against x0^2/nfft: {r:.3g} of 6u")
        assert r <= 1.0
        assert np.array_equal(st["spec"][0, : T.nbins], np.full(T.nbins, x[0])) and not st["spec"][0, T.nbp:].any()


def test_one_row_past_the_gemm_tile():
    """G0, 129 frames: one row past a 128-row tile of either GEMM kernel."""
    ex, T = setup("G0")
    x = mr.length_noise(T, T.frame_len + 128 * T.step)
    st = run(ex, x)
    assert st["out"].shape == (129, 26)
    full_check(T, x, st, "G0 noise F=129")


@pytest.mark.parametrize("name", ["G0", "G3"])
def test_all_zero_signal(name):
    """Two silent frames: every stage exactly zero, energy and the mel energies floored at eps, the output log(eps) rows of the
    oracle within the cepstrum bound."""
    ex, T = setup(name)
    x = np.zeros(T.frame_len + T.step, dtype=np.float32)
    st = run(ex, x)
    fig = full_check(T, x, st, f"{name} all-zero", e2e=None)
    zero, bad = mr.check_zero_frames(T, x, st)
    assert zero.all() and st["out"].shape[0] == 2 and not bad, bad
    for k in ("frames", "spec", "pw", "mel"):
        assert not st[k].any(), k
    assert (st["energy"] == mr.EPS32).all() and fig["out"] <= 1.0


@pytest.mark.parametrize("name", ["G0", "G3"])
def test_silent_stretch_inside_noise(name):
    """Eight frames of noise with frames 3 and 4 exactly zero.  The silent frames equal the oracle's eps-floored rows within the
    cepstrum bound; the frames that straddle the gap's edges pass every stage check; the frames that read no zeroed sample
    come out bit for bit as in a run of the same noise without the gap (same shape, so the same tiles) and within E2E_BOUND."""
    ex, T = setup(name)
    x = mr.noise_with_gap(T, seed=3)
    st = run(ex, x)
    clear = mr.frames_clear_of_gap(T)
    assert clear[0] and clear[-1] and not clear[2:6].any()
    full_check(T, x, st, f"{name} noise with gap", rows=clear)
    zero, bad = mr.check_zero_frames(T, x, st)
    assert list(np.flatnonzero(zero)) == [3, 4] and not bad, bad
    assert (st["energy"][zero] == mr.EPS32).all() and not st["mel"][zero].any()
    whole = run(ex, mr.noise_with_gap(T, seed=3, gap=False))
    for k in STAGES + ("out",):
        assert np.array_equal(st[k][clear].view(np.int32), whole[k][clear].view(np.int32)), f"{k}: a frame clear of the gap changed"
    if name == "G3":                                   # the mel == 0 floor inside normal frames: four empty filters
        assert int((~st["mel"][0, : T.nfilt].astype(bool)).sum()) == 4


CONCENTRATED = {"constant": (mr.constant, 0, 64), "alternating": (mr.alternating, -64, None), "bin2400": (mr.tone, -197, None)}


@pytest.mark.parametrize("kind", sorted(CONCENTRATED))
def test_concentrated_spectra(kind):
    """G0, three frames of a constant (power in bin 0), of alternating +-0.5 (the last bin, 2500) and of a tone in bin 2400
    (inside the last partial stride, bins 2304..2500, of the power kernel's 256-thread loop).  Every stage bound; coefficient 0
    end to end (the others are logs of cancellation residue: the float64 reference itself is ill-conditioned there); and energy
    may not fall short of the float64 sum of the device's pw over the bins that hold the power.  That check is one-sided: a
    1323-sample frame padded to 5000 leaks 2e-3 to 5e-3 of its power outside any such window, thirty times the nbp u bound,
    so energy cannot be within the bound of the restricted sum; it is within it of the full sum (the energy stage check)."""
    ex, T = setup("G0")
    build, lo, hi = CONCENTRATED[kind]
    lo, hi = (lo if lo >= 0 else T.nbins + lo), (T.nbins if hi is None else hi)
    x = build(T)
    st = run(ex, x)
    assert st["out"].shape == (3, 26)
    pw = st["pw"].astype(np.float64)
    print(f"mfcc[G0 {kind}] share of power outside bins {lo}..{hi - 1} per frame: {fmt(1 - pw[:, lo:hi].sum(1) / pw.sum(1))}"
          f" (leakage of the zero-padded rectangular frame; the energy bound is {T.nbp * mr.U:.1e} relative)")
    full_check(T, x, st, f"G0 {kind}", e2e=[0])
    bad = mr.check_energy_window(T, st, lo, hi)
    assert not bad, bad


def test_two_tones_with_and_without_zscore():
    """The signal class of the existing end-to-end test at four frames.  Unnormalised: every stage and every coefficient.
    With mean / std: the stages before the cepstrum are the same bits, the cepstrum is within its z-scored bound of float64,
    and the output is (raw - mean) / std of the unnormalised run within the two roundings of the subtraction and the division."""
    ex, T = setup("G0")
    x = mr.two_tones(T.frame_len + 3 * T.step)
    rng = np.random.default_rng(7)
    mean, std = rng.normal(size=26), rng.uniform(0.5, 3.0, size=26)
    raw = run(ex, x)
    full_check(T, x, raw, "G0 two tones")
    z = run(ex, x, mean, std)
    full_check(T, x, z, "G0 two tones z-scored", mean, std)
    for k in STAGES:
        assert np.array_equal(raw[k].view(np.int32), z[k].view(np.int32)), k
    want, bound = mr.zscore(raw["out"].astype(np.float64), np.zeros(raw["out"].shape), mean, std)
    r = mr.worst_ratio(z["out"], want, bound + mr.TINY)
    print(f"mfcc[G0 two tones] z-scored output against (raw - mean)/std: {r:.3g} of two roundings")
    assert r <= 1.0
    # through the extractor, as the data loader calls it
    ez = mr.make_extractor("G0", dev(), mfcc_mean=mean, mfcc_std=std)
    got = ez(torch.from_numpy(x).to(dev()))
    assert np.array_equal(got.cpu().numpy().view(np.int32), z["out"].view(np.int32))
    assert np.array_equal(ex(torch.from_numpy(x).to(dev())).cpu().numpy().view(np.int32), raw["out"].view(np.int32))


@pytest.mark.parametrize("e", [15, -15])
def test_scale_by_a_power_of_two(e):
    """A float wav and its int16-scaled twin differ by 2^15.  Scaling by a power of two is exact in every stage up to the mel
    energies (bit equality after the exact rescale); coefficient 0 moves by 2 log(2^e), coefficient c >= 1 by
    lift_c sum_j dct_cj 2 log(2^e) (zero but for the tables' rounding), each within the two runs' cepstrum bounds."""
    ex, T = setup("G0")
    x = mr.length_noise(T, T.frame_len + 2 * T.step)
    s = np.float32(2.0 ** e)
    base, scaled = run(ex, x), run(ex, x * s)
    full_check(T, x * s, scaled, f"G0 noise * 2^{e}")
    for k, p in dict(frames=1, spec=1, pw=2, energy=2, mel=2).items():
        assert np.array_equal(scaled[k], base[k] * np.float32(2.0 ** (p * e))), f"{k} does not scale exactly"
    shift = T.lift * T.dct.sum(axis=1) * 2 * np.log(2.0 ** e)
    shift[0] = 2 * np.log(2.0 ** e)
    tol = mr.ref_cepstrum(T, base["mel"], base["energy"])[1] + mr.ref_cepstrum(T, scaled["mel"], scaled["energy"])[1]
    r = mr.worst_ratio(scaled["out"].astype(np.float64) - base["out"].astype(np.float64), shift[None, :], tol)
    print(f"mfcc[G0 noise * 2^{e}] shift of the coefficients: {r:.3g} of the two cepstrum bounds; c0 moves by "
          f"{float((scaled['out'][:, 0] - base['out'][:, 0]).mean()):.6f} (2 log 2^{e} = {shift[0]:.6f})")
    assert r <= 1.0


def test_workspace_contents_and_repeat_do_not_matter():
    """A workspace prefilled with NaN, with zeros and with 1e30 gives the same bits, and so does a second call; the
    extractor's own call (work=None and a caller's workspace) gives them too."""
    ex, T = setup("G0")
    x = mr.length_noise(T, T.frame_len + 2 * T.step + 1)
    runs = [run(ex, x, fill=NAN), run(ex, x, fill=0.0), run(ex, x, fill=1e30), run(ex, x, fill=NAN)]
    for r in runs[1:]:
        for k in STAGES + ("out",):
            assert np.array_equal(r[k].view(np.int32), runs[0][k].view(np.int32)), k
    sig = torch.from_numpy(x).to(dev())
    F = ex.num_frames(len(x))
    work = ex.workspace(F, fill=NAN)
    for got in (ex(sig), ex(sig, work=work)):
        assert np.array_equal(got.cpu().numpy().view(np.int32), runs[0]["out"].view(np.int32))
    for k, v in zip(STAGES, ex.stage_views(work, F)):
        assert np.array_equal(v.cpu().numpy().view(np.int32), runs[0][k].view(np.int32)), k
    with pytest.raises(ValueError):
        ex(sig, work=work[:-1])


@pytest.mark.parametrize("name", ["G0", "G3"])
def test_signal_off_16_byte_alignment(name):
    ex, T = setup(name)
    x = mr.length_noise(T, T.frame_len + 2 * T.step + 1)
    padded = torch.from_numpy(np.concatenate(([np.float32(9.0)], x))).to(dev())
    assert padded.data_ptr() % 16 == 0 and padded[1:].data_ptr() % 16 == 4
    a, b = run(ex, x), run(ex, None, signal=padded[1:])
    for k in STAGES + ("out",):
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k


def test_prefix_of_a_long_signal():
    """The first five rows of a 129-frame run against the run of the signal cut at 4 step + frame_len.  The frames are the same
    bits; each run's spectrum is within the spec bound of the same float64 product, so the two are within twice the bound of
    each other; both runs pass every stage check and the end-to-end bound.  Whether all bits are equal is printed, not
    asserted: the GEMM tile, and with it the summation order, may depend on the row count."""
    ex, T = setup("G0")
    long = mr.length_noise(T, T.frame_len + 128 * T.step)
    Fp = 5
    cut = long[: (Fp - 1) * T.step + T.frame_len]
    a, b = run(ex, long), run(ex, cut)
    assert b["out"].shape == (Fp, 26)
    full_check(T, cut, b, "G0 prefix (cut signal)")
    assert np.array_equal(a["frames"][:Fp].view(np.int32), b["frames"].view(np.int32))
    bound = mr.ref_spec(T, b["frames"])[1]
    r = mr.worst_ratio(a["spec"][:Fp].astype(np.float64), b["spec"].astype(np.float64), 2 * bound)
    err, bad = mr.check_e2e(T, cut, a["out"][:Fp])
    same = {k: bool(np.array_equal(a[k][:Fp].view(np.int32), b[k].view(np.int32))) for k in STAGES + ("out",)}
    print(f"mfcc[G0 prefix] spec of the long run's first rows against the cut run: {r:.3g} of twice the bound; "
          f"out differs by at most {float(np.abs(a['out'][:Fp] - b['out']).max()):.2e}; bits equal: {same}")
    assert r <= 1.0 and not bad, bad
