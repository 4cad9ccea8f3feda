"""The MFCC front end (gdx_mfcc and its kernels, csrc/mfcc.hip) restated stage by stage in float64, with the input builders,
the error bounds and the comparison functions that tests/test_gpu_mfcc.py (GPU) and tests/test_mfcc_host.py (CPU, mutation
check) share.  No GPU code here.

Each stage is compared on the output of the stage BEFORE it as the device stored it (fp32, converted to fp64), against the
extractor's own fp32 tables (converted to fp64), so a bound never depends on how well-conditioned the signal is.  u = 2^-24.

  frames    x[i] - p x[i-1], p = float32(preemph), x[0] unchanged.  As one FMA (what the compiler emits) the result is rounded
            once: the error is at most u |result| <= u (|x[i]| + |p x[i-1]|).  As a multiply and a subtract it stays inside
            that unless both roundings are near their worst on operands of opposite sign.  0 exactly past the signal and in
            columns frame_len..Lp-1.
  spec      frames @ dft.T.  Any summation order, with or without FMA: |err| <= K u sum_i |a_i b_i|, K = Lp.
  pw        (re^2 + im^2) / nfft: two squares, one add, one multiply by the ROUNDED 1/nfft: relative 6u (five roundings and
            the second-order terms).
  energy    row sum of pw; every term is >= 0, so any order of nbp terms is within relative nbp u.  0 -> float32(2^-52).
  mel       pw @ mel.T, non-negative terms again: relative nbp u.
  cepstrum  lift_c sum_j dct_cj log(m_j): logf is L_U u |log m_j| off, the product and the nfilt-term FMA chain add
            (nfilt + 2) u times the sum of |terms|.  Coefficient 0 is logf(energy) alone: L_U u |log energy|.
            z-score: a subtraction and a division, two more roundings.

Relative bounds carry TINY = 2^-126 of absolute slack: below the normal range fp32 has no relative accuracy.

Measured constants (an MI355X, profiles/mfcc_stage_tests.txt):
  L_U        logf's worst error over every input of tests/test_gpu_mfcc.py, in units of u |log x|, against float64 log of the
             same fp32 argument (coefficient 0 of the unnormalised output is logf(energy) and nothing else).  Measured 2.713
             on the noise scaled by 2^-15 (1.4 ulp of the result: |log x| = 16.07 sits just above a power of two, where an
             ulp is 2u |log x|); 2.24 at most elsewhere.  L_U is twice the worst.
  E2E_BOUND  absolute error per coefficient of the unnormalised output against oracle/mfcc.py in float64 throughout.  Worst
             over the broadband inputs 5.70e-5 (G2, 401 samples, coefficient 12; G3: 3.80e-5; production geometry G0:
             2.83e-5 on the signal scaled by 2^-15, 2.28e-5 at 129 frames).  E2E_BOUND is four times the worst, for a later
             GEMM tile with another summation order: 2.28e-4, against the 9e-3 the older end-to-end test lets through.  It may
             never exceed E2E_CAP, and a measured worst above 2.5e-4 would be a finding, not a reason to raise it.
"""
import numpy as np

from oracle import mfcc as om

U = 2.0 ** -24
TINY = 2.0 ** -126
EPS = np.finfo(np.float64).eps                  # python_speech_features' floor
EPS32 = np.float32(2.220446049250313e-16)       # the same number as fp32: 2^-52 exactly
L_U_MEASURED = 2.713
L_U = 2 * L_U_MEASURED
E2E_MEASURED = 5.70e-5
E2E_BOUND = 4 * E2E_MEASURED
E2E_CAP = 1e-3

# (sr, fps, winlen, nfilt, nfft, numcep)
GEOMS = {
    "G0": (22050, 30, 0.06, 26, 5000, 27),      # production: frame_len 1323, step 735
    "G1": (16000, 100, 0.025, 26, 512, 13),     # the package's defaults, numcep < nfilt
    "G2": (16000, 100, 0.025, 64, 512, 64),     # the largest nfilt the kernel accepts
    "G3": (8000, 400, 0.005, 26, 64, 13),       # frame_len 40, step 20, nbins 33: four empty mel filters
    "G4": (22050, 30, 0.06, 26, 8192, 26),      # DFT N = 8320: past the persistent GEMM's N <= 8192
}
MUTANTS = ["energy_no_last_bin", "energy_whole_strides_only", "no_imaginary_part", "inv_frame_len", "flt_epsilon_floor",
           "lifter_shifted", "frame1_first_sample_raw", "mel_shifted_one_bin"]


def make_extractor(name, device, **kw):
    from gesturediffusion_amd.data_loaders.mfcc import MfccExtractor
    sr, fps, winlen, nfilt, nfft, numcep = GEOMS[name]
    return MfccExtractor(device, sr=sr, fps=fps, winlen=winlen, numcep=numcep, nfilt=nfilt, nfft=nfft, **kw)


class Tables:
    """The extractor's own fp32 tables as float64, and its geometry."""

    def __init__(self, name, ex):
        self.name, self.geom = name, GEOMS[name]
        f64 = lambda t: t.detach().cpu().numpy().astype(np.float64)   # noqa: E731
        self.dft, self.mel, self.dct, self.lift = f64(ex.dft), f64(ex.mel), f64(ex.dct), f64(ex.lift)
        self.adft = np.abs(self.dft)
        self.p = float(np.float32(ex.preemph))
        self.frame_len, self.step, self.nfft, self.nfilt, self.numcep = ex.frame_len, ex.frame_step, ex.nfft, ex.nfilt, ex.numcep
        self.Lp, self.nbp, self.nbins = ex.Lp, ex.nbp, ex.nfft // 2 + 1

    def num_frames(self, n):
        sr, fps, winlen = self.geom[:3]
        return om.frame_geometry(n, sr, winlen, 1 / fps)[2]


# ---- input builders (numpy, seeded: the same bits on every machine) ----------------------------------------------------------
def lengths(T):
    L, s = T.frame_len, T.step
    return [1, L, L + 1, L + s, L + s + 1, L + 2 * s + 1]


def noise(n, seed, sigma=0.3):
    return (sigma * np.random.default_rng(seed).normal(size=n)).astype(np.float32)


GAP_FRAMES = 8


def gap_range(T):
    return 3 * T.step - 1, 4 * T.step + T.frame_len


def length_noise(T, n):
    """The white-noise input of the length tests: one seed per geometry and length."""
    return noise(n, seed=1000 * int(T.name[1:]) + n)


def noise_with_gap(T, seed, gap=True):
    """Eight frames of noise in which frames 3 and 4 are exactly zero after pre-emphasis (x[i-1] of their first sample
    included); their neighbours straddle the edges of the gap.  gap=False: the same noise left whole."""
    x = noise(T.frame_len + (GAP_FRAMES - 1) * T.step, seed)
    if gap:
        lo, hi = gap_range(T)
        x[lo:hi] = 0.0
    return x


def frames_clear_of_gap(T):
    """Rows of noise_with_gap's output that read no zeroed sample, x[i-1] of their first sample included: the first and the
    last frame at least."""
    lo, hi = gap_range(T)
    f = np.arange(GAP_FRAMES)
    return (f * T.step + T.frame_len <= lo) | (f * T.step - 1 >= hi)


def constant(T, F=3):
    return np.full(T.frame_len + (F - 1) * T.step, 0.5, dtype=np.float32)


def alternating(T, F=3):
    x = constant(T, F)
    x[1::2] = -0.5
    return x


def tone(T, k=2400, F=3):
    i = np.arange(T.frame_len + (F - 1) * T.step)
    return np.cos(2 * np.pi * ((k * i) % T.nfft) / T.nfft).astype(np.float32)


def two_tones(n, sr=22050):
    """The signal class of test_mfcc_front_end_vs_restated_package (tests/test_gpu_parity.py)."""
    rng = np.random.default_rng(n)
    t = np.arange(n) / float(sr)
    return (0.3 * np.sin(2 * np.pi * 220 * t) + 0.1 * np.sin(2 * np.pi * 1870 * t) + 0.05 * rng.normal(size=n)).astype(np.float32)


# ---- float64 stage references and their bounds -------------------------------------------------------------------------------
def ref_frames(T, x, F):
    """-> (frames [F, Lp] float64, bound)"""
    x = np.asarray(x, dtype=np.float64)
    prev = np.concatenate(([0.0], x[:-1]))
    s, b = x - T.p * prev, U * (np.abs(x) + np.abs(T.p * prev))
    s[0], b[0] = x[0], 0.0
    padlen = (F - 1) * T.step + T.frame_len
    s, b = (np.concatenate((a, np.zeros(max(0, padlen - len(a)))))[:padlen] for a in (s, b))
    idx = np.arange(T.frame_len)[None, :] + (np.arange(F) * T.step)[:, None]
    fr, bd = np.zeros((F, T.Lp)), np.zeros((F, T.Lp))
    fr[:, : T.frame_len], bd[:, : T.frame_len] = s[idx], b[idx]
    return fr, bd


def ref_spec(T, frames):
    a = np.asarray(frames, dtype=np.float64)
    return a @ T.dft.T, T.Lp * U * (np.abs(a) @ T.adft.T)


def ref_pw(T, spec):
    s = np.asarray(spec, dtype=np.float64)
    pw = np.zeros((s.shape[0], T.nbp))
    pw[:, : T.nbins] = (s[:, : T.nbins] ** 2 + s[:, T.nbp: T.nbp + T.nbins] ** 2) / T.nfft
    return pw, 6 * U * pw + TINY * (pw != 0)


def ref_energy(T, pw):
    e = np.asarray(pw, dtype=np.float64).sum(axis=1)
    return np.where(e == 0, float(EPS32), e), np.where(e == 0, 0.0, T.nbp * U * e + TINY)


def ref_mel(T, pw):
    m = np.asarray(pw, dtype=np.float64) @ T.mel.T
    return m, T.nbp * U * m + TINY * (m != 0)


def ref_cepstrum(T, mel, energy, mean=None, std=None, lu=L_U, floor=EPS, lift=None):
    lift = T.lift if lift is None else lift
    m = np.asarray(mel, dtype=np.float64)[:, : T.nfilt]
    lg = np.log(np.where(m == 0, floor, m))
    v = lift * (lg @ T.dct.T)
    b = np.abs(lift) * (np.abs(lg) @ np.abs(T.dct).T) * ((T.nfilt + 2) * U + lu * U)
    e = np.asarray(energy, dtype=np.float64)
    le = np.log(np.where(e == 0, floor, e))
    v[:, 0], b[:, 0] = le, lu * U * np.abs(le)
    if mean is not None:
        v, b = zscore(v, b, mean, std)
    return v, b


def zscore(v, b, mean, std):
    """(v - mean) / std of values known within b, computed in fp32: the subtraction and the division round once each."""
    mean, std = (np.asarray(np.asarray(a, dtype=np.float32), dtype=np.float64)[: v.shape[1]] for a in (mean, std))
    z, zb = (v - mean) / std, b / np.abs(std)
    return z, zb + 2 * U * (np.abs(z) + zb)


def oracle_out(T, x):
    sr, fps, winlen, nfilt, nfft, numcep = T.geom
    return om.mfcc(np.asarray(x, dtype=np.float64), samplerate=sr, winlen=winlen, winstep=1 / fps, numcep=numcep, nfilt=nfilt,
                   nfft=nfft)


# ---- the device pipeline in float64, each stage rounded to fp32 where the device stores it; optionally with one mistake --------
def emulate(T, x, mean=None, std=None, mutant=None):
    f32 = lambda a: np.asarray(a, dtype=np.float32)   # noqa: E731
    assert mutant is None or mutant in MUTANTS
    F = T.num_frames(len(x))
    fr = ref_frames(T, x, F)[0]
    if mutant == "frame1_first_sample_raw" and F > 1 and T.step < len(x):
        fr[1, 0] = x[T.step]
    fr = f32(fr)
    spec = f32(ref_spec(T, fr)[0])
    s = spec.astype(np.float64).copy()
    if mutant == "no_imaginary_part":
        s[:, T.nbp:] = 0.0
    pw = ref_pw(T, s)[0]
    if mutant == "inv_frame_len":
        pw = pw * T.nfft / T.frame_len
    pw = f32(pw)
    floor = float(np.float32(1.1920929e-07)) if mutant == "flt_epsilon_floor" else float(EPS32)
    keep = {"energy_no_last_bin": T.nbins - 1, "energy_whole_strides_only": 256 * (T.nbins // 256)}.get(mutant, T.nbp)
    e = pw[:, :keep].astype(np.float64).sum(axis=1)
    energy = f32(np.where(e == 0, floor, e))
    melt = np.roll(T.mel, 1, axis=1) if mutant == "mel_shifted_one_bin" else T.mel
    mel = f32(pw.astype(np.float64) @ melt.T)
    lift = np.concatenate((T.lift[1:], T.lift[:1])) if mutant == "lifter_shifted" else T.lift
    out = f32(ref_cepstrum(T, mel, energy, mean, std, floor=floor, lift=lift)[0])
    return dict(frames=fr, spec=spec, pw=pw, mel=mel, energy=energy, out=out)


# ---- comparisons -------------------------------------------------------------------------------------------------------------
def worst_ratio(got, want, bound):
    """max |got - want| / bound; 0 where both vanish, inf where an error meets a zero bound or a value is not finite."""
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got - want)
    err = np.where(np.isfinite(got), err, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(r.max()) if r.size else 0.0


def logf_units(st):
    """logf's error on the energies of an unnormalised run, in units of u |log x|."""
    e = st["energy"].astype(np.float64)
    le = np.log(e)
    return float(np.max(np.abs(st["out"][:, 0].astype(np.float64) - le) / (U * np.abs(le))))


def check_stages(T, x, st, mean=None, std=None):
    """Every stage of one run against its float64 reference.  -> (figures, failures): figures[stage] is the worst error as a
    fraction of the stage's bound, failures the list of broken claims (empty when the run is right)."""
    F = T.num_frames(len(x))
    fig, bad = {}, []

    def claim(ok, what):
        if not ok:
            bad.append(f"{T.name} n={len(x)}: {what}")

    for k, shape in dict(frames=(F, T.Lp), spec=(F, 2 * T.nbp), pw=(F, T.nbp), mel=(F, 64), energy=(F,), out=(F, T.numcep)).items():
        claim(st[k].shape == shape, f"{k} has shape {st[k].shape}, not {shape}")
        claim(bool(np.isfinite(st[k]).all()), f"{k} holds a non-finite value")
    if bad:
        return fig, bad
    refs = dict(frames=ref_frames(T, x, F), spec=ref_spec(T, st["frames"]), pw=ref_pw(T, st["spec"]),
                energy=ref_energy(T, st["pw"]), mel=ref_mel(T, st["pw"]),
                out=ref_cepstrum(T, st["mel"], st["energy"], mean, std))
    for k, (want, bound) in refs.items():
        fig[k] = worst_ratio(st[k], want, bound)
        claim(fig[k] <= 1.0, f"{k} is {fig[k]:.3g} of its bound away from float64")
    claim(not st["frames"][:, T.frame_len:].any(), "frames: a padding column is not zero")
    for half in (0, T.nbp):
        claim(not st["spec"][:, half + T.nbins: half + T.nbp].any(), "spec: a padding column is not zero")
    claim(not st["pw"][:, T.nbins:].any(), "pw: a padding column is not zero")
    claim(not st["mel"][:, T.nfilt:].any(), "mel: a column past nfilt is not zero")
    zero = ~st["pw"].any(axis=1)
    claim(bool((st["energy"][zero] == EPS32).all()), "energy of an all-zero row is not float32(2.220446049250313e-16)")
    return fig, bad


def check_e2e(T, x, out, coefs=None, rows=None):
    """-> (per-coefficient errors, failures) against E2E_BOUND, over the frames in `rows` and the coefficients in `coefs`."""
    assert E2E_BOUND <= E2E_CAP
    want = oracle_out(T, x)
    if out.shape != want.shape:
        return None, [f"{T.name} n={len(x)}: output shape {out.shape}, the package gives {want.shape}"]
    err = np.abs(out.astype(np.float64) - want)
    err = np.where(np.isfinite(out), err, np.inf)
    if rows is not None:
        err = err[rows]
    err = err.max(axis=0)
    sel = err if coefs is None else err[coefs]
    bad = [] if float(sel.max()) <= E2E_BOUND else [
        f"{T.name} n={len(x)}: end to end, coefficient {int(np.argmax(err))} is {float(err.max()):.3g} from the oracle "
        f"(bound {E2E_BOUND:.3g})"]
    return err, bad


def check_zero_frames(T, x, st):
    """Frames that are exactly zero after pre-emphasis: the output equals the oracle's eps-floored values within the cepstrum
    bound.  -> (rows that are zero, failures)"""
    F = T.num_frames(len(x))
    zero = ~ref_frames(T, x, F)[0].any(axis=1)
    want = oracle_out(T, x)
    bound = ref_cepstrum(T, st["mel"], st["energy"])[1]
    r = worst_ratio(st["out"][zero], want[zero], bound[zero])
    return zero, ([] if r <= 1.0 else [f"{T.name} n={len(x)}: a silent frame is {r:.3g} of the cepstrum bound from log(eps)"])


def check_energy_window(T, st, lo, hi, share=0.5):
    """Concentrated spectra: the bins lo..hi-1 hold the power (at least `share` of it in some frame), every term of the sum is
    non-negative, so energy may not be below the float64 sum of the device's pw over those bins alone, less the sum's own
    rounding.  A reduction that drops one of them falls short by that bin's power."""
    pw = st["pw"].astype(np.float64)
    part, total = pw[:, lo:hi].sum(axis=1), pw.sum(axis=1)
    bad = []
    if not (part >= share * total).any():
        bad.append(f"{T.name}: bins {lo}..{hi - 1} hold at most {float((part / total).max()):.3g} of a frame's power")
    short = st["energy"].astype(np.float64) < part * (1 - T.nbp * U) - TINY
    if short.any():
        bad.append(f"{T.name}: energy of frame {int(np.argmax(short))} is below the power in bins {lo}..{hi - 1}")
    return bad
