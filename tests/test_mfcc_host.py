"""CPU-only tests of the MFCC front end's host side (gesturediffusion_amd/data_loaders/mfcc.py): the extractor's tables against
oracle/mfcc.py and numpy's FFT, frame counts, the workspace layout against the formula at gdx_mfcc (csrc/mfcc.hip), what
gdx_mfcc refuses before it touches the device, and a mutation check of the bounds the GPU test asserts
(tests/mfcc_restatement.py): each of eight plausible kernel mistakes, applied to the float64 restatement of the pipeline, must
be rejected by the GPU test's own comparison functions on at least one of its inputs, and the unmutated restatement accepted
on all of them."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import mfcc_restatement as mr
from oracle import mfcc as om


@functools.lru_cache(maxsize=None)
def setup(name):
    ex = mr.make_extractor(name, "cpu")
    return ex, mr.Tables(name, ex)


def _lib_or_skip():
    from gesturediffusion_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgdx.so not built (run python __graft_entry__.py)")
    return _lib, _lib.load()


@pytest.mark.parametrize("name", sorted(mr.GEOMS))
def test_filterbank_dct_and_lifter_equal_the_oracles(name):
    from gesturediffusion_amd.data_loaders.mfcc import _mel_filterbank
    sr, fps, winlen, nfilt, nfft, numcep = mr.GEOMS[name]
    ex, T = setup(name)
    fb = om.get_filterbanks(nfilt, nfft, sr)
    assert np.array_equal(_mel_filterbank(nfilt, nfft, sr), fb)
    mel = ex.mel.numpy()
    assert mel.shape == (64, T.nbp) and np.array_equal(mel[:nfilt, : T.nbins], fb.astype(np.float32))
    assert not mel[nfilt:].any() and not mel[:, T.nbins:].any()
    nc = min(numcep, nfilt)
    assert ex.numcep == nc
    assert np.array_equal(ex.dct.numpy(), om.dct_ortho_matrix(nfilt)[:nc].astype(np.float32))
    assert np.array_equal(ex.lift.numpy(), (1 + (22 / 2.) * np.sin(np.pi * np.arange(nc) / 22)).astype(np.float32))
    if name == "G3":                                # the geometry was chosen for this: the mel == 0 floor acts inside a frame
        assert int((~fb.any(axis=1)).sum()) == 4


@pytest.mark.parametrize("name", sorted(mr.GEOMS))
def test_dft_table_is_the_rfft(name):
    """frames @ table.T in float64 against numpy's rfft zero-padded to nfft: 1e-6 of the frame's norm (the table's fp32
    rounding, 2^-25 per entry, summed over a frame)."""
    ex, T = setup(name)
    assert tuple(ex.dft.shape) == (2 * T.nbp, T.Lp)
    fr = np.random.default_rng(5).normal(size=(3, T.frame_len))
    got = fr @ T.dft[:, : T.frame_len].T
    want = np.fft.rfft(fr, T.nfft)
    norm = np.linalg.norm(fr, axis=1)[:, None]
    assert (np.abs(got[:, : T.nbins] - want.real) <= 1e-6 * norm).all()
    assert (np.abs(got[:, T.nbp: T.nbp + T.nbins] - want.imag) <= 1e-6 * norm).all()      # -sin sits at row nbp + k
    assert not T.dft[:, T.frame_len:].any()
    assert not T.dft[T.nbins: T.nbp].any() and not T.dft[T.nbp + T.nbins:].any()
    assert T.dft[1, 1] > 0 and T.dft[T.nbp + 1, 1] < 0


@pytest.mark.parametrize("name", sorted(mr.GEOMS))
def test_frame_counts_and_geometry(name):
    sr, fps, winlen, nfilt, nfft, numcep = mr.GEOMS[name]
    ex, T = setup(name)
    for n in mr.lengths(T) + [T.frame_len + 128 * T.step, T.frame_len - 1, 2]:
        fl, fs, F = om.frame_geometry(n, sr, winlen, 1 / fps)
        assert (ex.frame_len, ex.frame_step, ex.num_frames(n)) == (fl, fs, F)
    assert ex.Lp % 32 == 0 and 0 <= ex.Lp - ex.frame_len < 32 and ex.nbp % 64 == 0 and 0 <= ex.nbp - T.nbins < 64


def test_production_geometry():
    ex, T = setup("G0")
    assert (ex.frame_len, ex.frame_step, ex.Lp, ex.nbp, ex.numcep) == (1323, 735, 1344, 2560, 26)
    assert setup("G4")[0].nbp * 2 == 8320 and setup("G4")[0].nbp * 2 % 128 == 0    # gemm.hip reads W in 128-row tiles


def test_frame_longer_than_nfft_raises():
    from gesturediffusion_amd.data_loaders.mfcc import MfccExtractor
    with pytest.raises(ValueError, match="nfft"):
        MfccExtractor("cpu", sr=16000, fps=100, winlen=0.025, nfft=256)
    MfccExtractor("cpu", sr=16000, fps=100, winlen=0.025, nfft=400)                 # frame_len == nfft is allowed


@pytest.mark.parametrize("name", ["G0", "G3"])
@pytest.mark.parametrize("F", [1, 3, 129])
def test_workspace_layout_is_the_formula_at_gdx_mfcc(name, F):
    """work: (numframes + GDX_ROW_PAD) * (Lp + 2*nbp + nbp + 64) + numframes floats, frames | spec | pw | mel | energy."""
    from gesturediffusion_amd import _lib
    ex, T = setup(name)
    rows = F + _lib.GDX_ROW_PAD
    size = rows * (T.Lp + 2 * T.nbp + T.nbp + 64) + F
    work = ex.workspace(F, fill=7.0)
    assert work.dtype == torch.float32 and work.numel() == size == ex.workspace_size(F) and bool((work == 7.0).all())
    assert not ex.workspace(F).any()
    views = ex.stage_views(work, F)
    widths = [T.Lp, 2 * T.nbp, T.nbp, 64]
    off = 0
    for v, w in zip(views[:4], widths):
        assert tuple(v.shape) == (F, w) and v.stride() == (w, 1) and v.storage_offset() == off
        off += rows * w
    assert tuple(views[4].shape) == (F,) and views[4].storage_offset() == off and off + F == size
    views[4][F - 1] = 1.0                                                          # views, not copies
    assert work[size - 1] == 1.0
    with pytest.raises(ValueError):
        ex.stage_views(work[:-1], F)
    with pytest.raises(_lib.GdxError, match="no CPU fallback"):
        ex(torch.zeros((F - 1) * T.step + T.frame_len), work=work)


def test_gdx_mfcc_refusals():
    """Each refusal comes before the first HIP call (no device here, the pointers are never dereferenced): non-zero and a
    message from gdx_last_error."""
    _lib, lib = _lib_or_skip()
    p = C.c_void_p(0x1000)
    ok = dict(signal=p, n=2058, frame_len=1323, frame_step=735, numframes=2, nfft=5000, nfilt=26, numcep=26, dft=p, mel=p,
              dct=p, lifter=p, work=p, out=p)
    cases = [(dict({k: None}), b"null argument") for k in ("signal", "dft", "mel", "dct", "lifter", "work", "out")]
    cases += [(ch, b"bad geometry") for ch in (dict(n=0), dict(n=-5), dict(nfft=1322), dict(nfilt=65, numcep=27),
                                               dict(numcep=27), dict(frame_step=0), dict(numframes=0), dict(numcep=0),
                                               dict(frame_len=0), dict(nfilt=0, numcep=0))]
    for change, msg in cases:
        a = dict(ok, **change)
        lib.gdx_set_graph_replay(None, 0)                                          # leaves another message behind
        assert b"gdx_mfcc" not in lib.gdx_last_error()
        rc = lib.gdx_mfcc(a["signal"], a["n"], a["frame_len"], a["frame_step"], a["numframes"], a["nfft"], a["nfilt"],
                          a["numcep"], C.c_float(0.97), a["dft"], a["mel"], a["dct"], a["lifter"], None, None, a["work"],
                          a["out"], None)
        assert rc != 0, change
        assert b"gdx_mfcc" in lib.gdx_last_error() and msg in lib.gdx_last_error(), (change, lib.gdx_last_error())


# ---- mutation check ----------------------------------------------------------------------------------------------------------
def listed_inputs():
    """(geometry, label, signal, kind) of the GPU test's inputs that the mutants are run on."""
    out = []
    for name in ("G0", "G3"):
        T = setup(name)[1]
        out.append((name, "noise", mr.length_noise(T, mr.lengths(T)[-1]), "broadband"))
        out.append((name, "all-zero", np.zeros(T.frame_len + T.step, dtype=np.float32), "zero"))
        out.append((name, "noise with gap", mr.noise_with_gap(T, seed=3), "gap"))
    T = setup("G0")[1]
    out.append(("G0", "constant", mr.constant(T), (0, 64)))
    out.append(("G0", "alternating", mr.alternating(T), (T.nbins - 64, T.nbins)))
    out.append(("G0", "bin 2400", mr.tone(T), (256 * (T.nbins // 256), T.nbins)))
    out.append(("G0", "two tones", mr.two_tones(T.frame_len + 3 * T.step), "broadband"))
    return out


def verdict(T, x, kind, st):
    """What tests/test_gpu_mfcc.py asserts of one unnormalised run, as a list of failures."""
    bad = mr.check_stages(T, x, st)[1]
    if bad:
        return bad
    if kind == "broadband":
        bad += mr.check_e2e(T, x, st["out"])[1]
    elif kind in ("zero", "gap"):
        zero, b = mr.check_zero_frames(T, x, st)
        assert zero.all() if kind == "zero" else list(np.flatnonzero(zero)) == [3, 4]
        bad += b
        if kind == "gap":
            bad += mr.check_e2e(T, x, st["out"], rows=mr.frames_clear_of_gap(T))[1]
    else:
        bad += mr.check_e2e(T, x, st["out"], coefs=[0])[1] + mr.check_energy_window(T, st, *kind)
    return bad


def test_the_restatement_itself_passes_every_check():
    for name, label, x, kind in listed_inputs():
        T = setup(name)[1]
        st = mr.emulate(T, x)
        assert verdict(T, x, kind, st) == [], (name, label)
        assert mr.logf_units(st) <= 1.0                                           # correctly rounded: within u of float64
    rng = np.random.default_rng(0)
    T = setup("G0")[1]
    mean, std = rng.normal(size=26), rng.uniform(0.5, 3.0, size=26)
    x = mr.two_tones(T.frame_len + 3 * T.step)
    assert mr.check_stages(T, x, mr.emulate(T, x, mean, std), mean, std)[1] == []


@pytest.mark.parametrize("mutant", mr.MUTANTS)
def test_bounds_reject_the_mutant(mutant):
    caught = []
    for name, label, x, kind in listed_inputs():
        T = setup(name)[1]
        if verdict(T, x, kind, mr.emulate(T, x, mutant=mutant)):
            caught.append(f"{name} {label}")
    print(f"{mutant}: rejected on {caught}")
    assert caught, f"{mutant} passes every check on every listed input"


def test_committed_bounds_are_the_measured_figures_with_their_margins():
    assert mr.L_U == 2 * mr.L_U_MEASURED
    assert mr.E2E_BOUND == 4 * mr.E2E_MEASURED <= mr.E2E_CAP
    assert mr.E2E_MEASURED <= 2.5e-4
