"""Host-side checks of parallel-in-time sampling (gdx_window_sweep, gdx_parallel_loop, parallel_sample_loop, sample.generate
--parallel_window; the rule is in include/gdx.h): no GPU needed.  The restatement lives in parallel_restatement.py."""
import ctypes as C
import math
import os
import subprocess

import pytest
import torch

import parallel_restatement as R
from conftest import REPO, load_golden, weights_from
from oracle import mdm_forward as omf
from oracle import sampler as osamp
from oracle import schedule as osch
from test_dpm_host import diffusion

TINY = dict(njoints=16, nfeats=1, latent_dim=128, ff_size=256, num_layers=2, num_heads=4, seed_poses=10)
ARCHS = ["mdm", "mdm_old"]
B = 2


def tiny_case(arch, T=20, steps=10):
    """(weights, config, y, tape [steps + 1, B, 16, 1, T]) of a tiny fixture on the host: the first B samples, the first T frames."""
    g = load_golden(f"loops_{arch}_tiny.npz")
    y = {"seed": torch.from_numpy(g["seed"])[:B].contiguous(), "mfcc": torch.from_numpy(g["mfcc"])[:B, :, :, :T].contiguous()}
    tape = torch.from_numpy(g["tape"])
    if tape.shape[0] < steps + 1:                                  # longer loops than the fixture recorded: more of the same
        gen = torch.Generator().manual_seed(20230516)
        tape = torch.cat([tape, torch.randn(steps + 1 - tape.shape[0], *tape.shape[1:], generator=gen)])
    return weights_from(g), dict(TINY, arch=arch), y, tape[:steps + 1, :B, :, :, :T].contiguous()


# ------------------------------------------------------------------------------------------------------------ stride header
@pytest.fixture(scope="module")
def stride_probe(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++") if subprocess.run(
        ["sh", "-c", f"command -v {c}"], capture_output=True).returncode == 0), None)
    assert cxx, "no C++ compiler"
    exe = os.path.join(str(tmp_path_factory.mktemp("window_stride")), "window_stride_probe")
    built = subprocess.run([cxx, "-std=c++17", "-Werror", "-I", os.path.join(REPO, "gesturediffusion_amd", "csrc"),
                            os.path.join(REPO, "tests", "window_stride_probe.cpp"), "-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr

    def run(cases):
        """cases: (err rows [n][B], thresholds [num_steps], first_index) -> the header's strides."""
        lines = []
        for err, thr, first in cases:
            flat = [repr(float(e)) for row in err for e in row]
            lines.append(" ".join([str(len(err[0])), str(len(err)), str(first), str(len(thr))] + [repr(float(t)) for t in thr] + flat))
        got = subprocess.run([exe], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.split()
        assert len(got) == len(cases)
        return [int(v) for v in got]
    return run


def test_stride_header_equals_the_restatement(stride_probe):
    """csrc/gdx_window_stride.h, compiled with the host compiler alone, against the restatement's stride on hand-made error rows:
    all pass, none pass, a NaN, a pass behind a fail (which must not count), n = 1, a fail in one sample only, a threshold met
    exactly, tau = 0."""
    nan = float("nan")
    thr = [0.5, 0.25, 0.125, 1.0, 2.0, 4.0]                          # slot j of a window at first_index f reads thr[f - j]
    cases = [
        ([[0.1, 0.2], [0.3, 0.1], [0.05, 0.0]], thr, 5, 3),         # all pass: capped at n
        ([[9.0, 0.0], [0.0, 0.0], [0.0, 0.0]], thr, 5, 1),          # none of the leading pass
        ([[0.1, 0.1], [nan, 0.0], [0.0, 0.0]], thr, 5, 2),          # a NaN never passes
        ([[nan, nan]], thr, 0, 1),
        ([[0.1, 0.1], [9.0, 0.1], [0.0, 0.0], [0.0, 0.0]], thr, 5, 2),   # a pass behind a fail does not count
        ([[0.1]], thr, 3, 1), ([[9.0]], thr, 3, 1),                 # n = 1
        ([[0.1, 0.1], [0.1, 1.5], [0.0, 0.0]], thr, 5, 3),          # the worst sample decides: 1.5 <= thr[4] = 2.0
        ([[0.1, 0.1], [0.1, 2.5], [0.0, 0.0]], thr, 5, 2),          # 2.5 > thr[4]
        ([[0.125, 0.125], [0.25, 0.0]], thr, 2, 2),                 # thresholds met exactly (<=)
        ([[0.0, 0.0], [0.0, 0.0], [1e-300, 0.0], [0.0, 0.0]], [0.0] * 6, 5, 3),   # tau = 0: only an unchanged plane passes
        ([[0.3, 0.0], [0.0, 0.0]], thr, 2, 1),                      # thr[2] = 0.125 < 0.3
    ]
    want = [R.stride_of(err, [t[first - j] for j in range(len(err))]) for err, t, first, _ in cases]
    assert want == [c[3] for c in cases]
    assert stride_probe([c[:3] for c in cases]) == want


# ------------------------------------------------------------------------------------------------------------- restatement
@pytest.mark.parametrize("arch", ARCHS)
@pytest.mark.parametrize("kind", ["p", "ddim"])
def test_restatement_at_window_1_is_the_sequential_loop(arch, kind):
    """W = 1 is the sequential loop for any tau: bit-equal to oracle.sampler.sample_loop on ddim10, both kinds, both archs."""
    p, cfg, y, tape = tiny_case(arch)
    tab, tmap = osch.make_tables("cosine", 1000, "ddim10")
    with torch.no_grad():
        want = osamp.sample_loop(lambda x, t, yy: omf.forward(p, cfg, x, t, yy), tab, tmap, tuple(tape[0].shape), tape, y, kind=kind,
                                 eta=0.5)
    for tau in (0.0, 0.1, 1e6):
        got, strides = R.parallel_loop(p, cfg, tab, tmap, tape, y, kind, 1, tau, eta=0.5)
        assert torch.equal(got, want) and strides == [1] * 10, tau


@pytest.mark.parametrize("arch", ARCHS)
def test_restatement_iterations_and_strides(arch):
    """tau = 1e6 strides n every time: ceil(K / W) iterations; the strides sum to K for every tau tried; tau = 0 reproduces the
    sequential loop bit for bit at every window (an accepted plane did not change in a single bit)."""
    p, cfg, y, tape = tiny_case(arch)
    tab, tmap = osch.make_tables("cosine", 1000, "ddim10")
    K = tab.num_timesteps
    seq, _ = R.parallel_loop(p, cfg, tab, tmap, tape, y, "p", 1, 0.0)
    for W in (3, 4, 16):
        got, strides = R.parallel_loop(p, cfg, tab, tmap, tape, y, "p", W, 1e6)
        assert len(strides) == math.ceil(K / W) and sum(strides) == K
        assert torch.isfinite(got).all()
        for tau in (0.0, 1e-3, 1e-1):
            got, strides = R.parallel_loop(p, cfg, tab, tmap, tape, y, "p", W, tau)
            assert sum(strides) == K and math.ceil(K / W) <= len(strides) <= K and all(1 <= s <= W for s in strides), (W, tau)
            if tau == 0.0:
                assert torch.equal(got, seq), W


def test_restatement_ends_after_k_iterations_on_a_nan():
    p, cfg, y, tape = tiny_case("mdm_old")
    tab, tmap = osch.make_tables("cosine", 1000, "ddim10")
    tape = tape.clone()
    tape[0, 0, 3, 0, 5] = float("nan")
    _, strides = R.parallel_loop(p, cfg, tab, tmap, tape, y, "p", 4, 1e6)
    assert strides == [1] * 10                                       # sample 0 never passes, and the maximum is over the batch


# ------------------------------------------------------------------------------------------------------------------- C ABI
def _lib_or_skip():
    from gesturediffusion_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgdx.so not built (run python __graft_entry__.py)")
    return _lib


def _refused(lib, rc, text):
    return rc < 0 and text in lib.gdx_last_error()


SWEEP_PARAMS = ["kind", "batch", "njoints", "frames", "n_slots", "coef", "first_index", "planes", "x0", "inpaint_mask", "inpaint_motion",
                "clip_denoised", "noise", "philox_seed", "sample_offset", "rng_step", "err", "workspace", "stream"]
LOOP_PARAMS = ["h", "kind", "mode", "num_steps", "first_index", "coef", "timestep_map", "threshold", "window", "planes", "scale",
               "inpaint_mask", "inpaint_motion", "clip_denoised", "noise_tape", "philox_seed", "sample_offset", "anchor",
               "max_iterations", "strides_out", "strides_capacity", "iterations_out", "stream"]


def test_exports_come_from_the_header():
    """Both entries are declared in gdx.h with plain arguments: the header's set of argument structs is unchanged."""
    from gesturediffusion_amd import _lib
    protos = _lib.HEADER.prototypes
    assert "gdx_window_sweep" in _lib.EXPORTS and "gdx_parallel_loop" in _lib.EXPORTS
    assert [n for _, n in protos["gdx_window_sweep"][1]] == SWEEP_PARAMS
    assert [n for _, n in protos["gdx_parallel_loop"][1]] == LOOP_PARAMS
    assert protos["gdx_window_sweep"][0] == protos["gdx_parallel_loop"][0] == "int"
    assert dict((n, t) for t, n in protos["gdx_window_sweep"][1])["err"] == "double*"
    assert dict((n, t) for t, n in protos["gdx_parallel_loop"][1])["threshold"] == "const double*"
    assert not any("window" in s or "parallel" in s for s in _lib.HEADER.structs)


def test_sweep_refusals_without_gpu():
    """gdx_window_sweep is stateless: every refusal is decided from the arguments (addresses are never followed)."""
    _lib = _lib_or_skip()
    lib = _lib.load()
    P, Q, S = 4096, 8192, 12288
    ok = dict(kind=_lib.GDX_SAMPLER_P, batch=2, njoints=3, frames=5, n_slots=4, coef=P, first_index=9, planes=P, x0=Q, clip_denoised=0,
              philox_seed=0, sample_offset=0, rng_step=1, err=S, workspace=S)
    sweep = lambda **kw: lib.gdx_window_sweep(*[{**ok, **kw}.get(n) for n in SWEEP_PARAMS])   # noqa: E731
    for missing in ("coef", "planes", "x0", "err", "workspace"):
        assert _refused(lib, sweep(**{missing: None}), b"gdx_window_sweep: null argument"), missing
    assert _refused(lib, sweep(kind=7), b"kind must be")
    for bad in (0, -1, 65):
        assert _refused(lib, sweep(n_slots=bad, first_index=99), b"n_slots must lie in 1 .. 64"), bad
    assert _refused(lib, sweep(batch=65536), b"bad shape") and _refused(lib, sweep(frames=-1), b"bad shape")
    assert _refused(lib, sweep(first_index=2), b"below index 0")
    assert _refused(lib, sweep(inpaint_mask=Q), b"mask without motion")
    assert _refused(lib, sweep(err=S + 4), b"8-byte aligned")
    assert sweep(batch=0) == 0 and sweep(frames=0) == 0              # nothing to do is not an error


def test_loop_refusals_without_gpu():
    """The argument checks of gdx_parallel_loop need no handle: they come first, then the null handle, then the handle's refresh
    and layer cache, then readiness -- all before any HIP call."""
    _lib = _lib_or_skip()
    lib = _lib.load()
    P = 4096
    anchor, its = C.c_int32(0), C.c_int32(0)
    ok = dict(kind=_lib.GDX_SAMPLER_P, mode=0, num_steps=10, first_index=9, coef=P, timestep_map=P, threshold=P, window=4, planes=P,
              clip_denoised=0, philox_seed=0, sample_offset=0, anchor=C.byref(anchor), max_iterations=0, strides_capacity=0,
              iterations_out=C.byref(its))
    loop = lambda **kw: lib.gdx_parallel_loop(*[{**ok, **kw}.get(n) for n in LOOP_PARAMS])   # noqa: E731
    for missing in ("coef", "timestep_map", "threshold", "planes", "anchor", "iterations_out"):
        assert _refused(lib, loop(**{missing: None}), b"gdx_parallel_loop: null argument"), missing
    assert _refused(lib, loop(kind=7), b"kind must be")
    assert _refused(lib, loop(mode=3), b"bad mode") and _refused(lib, loop(mode=2), b"needs scale")
    for bad in (dict(num_steps=0), dict(first_index=10), dict(first_index=-1)):
        assert _refused(lib, loop(**bad), b"bad step range"), bad
    for bad in (0, -1, 65):
        assert _refused(lib, loop(window=bad), b"window must lie in 1 .. 64"), bad
    for bad in (-1, 11):
        assert _refused(lib, loop(anchor=C.byref(C.c_int32(bad))), b"anchor must lie"), bad
    assert _refused(lib, loop(max_iterations=-1), b"bad max_iterations") and _refused(lib, loop(strides_capacity=3), b"strides_out")
    assert _refused(lib, loop(inpaint_mask=P), b"mask without motion")
    for fine in (dict(), dict(window=1), dict(window=64), dict(anchor=C.byref(C.c_int32(10)))):
        assert _refused(lib, loop(**fine), b"null handle"), fine
    h = C.c_void_p()
    cfg = _lib.Config(arch=1, njoints=16, latent_dim=128, ff_size=256, num_layers=2, num_heads=4, seed_poses=10, mfcc_dim=26,
                      cl_head=8, window=10)
    if lib.gdx_create(C.byref(cfg), C.byref(h)) == 0:          # where a handle can be made without a device: not prepared
        assert _refused(lib, loop(h=h), b"gdx_prepare")
        assert lib.gdx_set_guidance_refresh(h, 2) == 0
        assert _refused(lib, loop(h=h), b"guidance refresh")
        assert lib.gdx_set_guidance_refresh(h, 1) == 0 and lib.gdx_set_layer_cache(h, 2, 1) == 0
        assert _refused(lib, loop(h=h), b"layer cache")
        lib.gdx_destroy(h)
    assert anchor.value == 0 and its.value == 0


# ------------------------------------------------------------------------------------------------------------------ Python
def test_python_refusals_need_no_device():
    from gesturediffusion_amd.model.cfg_sampler import ClassifierFreeSampleModel
    df = diffusion("cosine", "ddim10")
    shape = (2, 3, 1, 4)
    guided = object.__new__(ClassifierFreeSampleModel)       # only its type is looked at
    with pytest.raises(ValueError, match="native"):
        df.parallel_sample_loop(lambda x, t, **kw: x, shape)
    with pytest.raises(ValueError, match="native"):
        df.parallel_sample_loop(None, shape)
    with pytest.raises(ValueError, match="guidance_refresh"):
        df.parallel_sample_loop(guided, shape, model_kwargs={"y": {"guidance_refresh": 2}})
    with pytest.raises(ValueError, match="layer_cache"):
        df.parallel_sample_loop(guided, shape, model_kwargs={"y": {"layer_cache": (2, 1)}})
    for window in (0, 65, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="window must be"):
            df.parallel_sample_loop(guided, shape, window=window)
    for tol in (-0.1, float("nan"), "0.1", None):
        with pytest.raises(ValueError, match="tolerance must be"):
            df.parallel_sample_loop(guided, shape, tolerance=tol)
    for sampler in ("plms", "dpmpp", "P", None):
        with pytest.raises(ValueError, match="sampler 'p' or 'ddim'"):
            df.parallel_sample_loop(guided, shape, sampler=sampler)
    with pytest.raises(TypeError):                              # keyword-only behind init_image
        df.parallel_sample_loop(guided, shape, None, True, None, None, False, 0, None, "p")


def test_threshold_is_the_restatements():
    import numpy as np
    for resp in ("ddim10", [40], [1000]):
        df = diffusion("cosine", resp)
        tab, _ = osch.make_tables("cosine", 1000, resp)
        for tau in (0.0, 1e-2, 0.1):
            got = df.parallel_threshold(tau)
            assert got.dtype == np.float64 and got.shape == (df.num_timesteps,) and np.array_equal(got, R.threshold(tab, tau))
        assert not df.parallel_threshold(0.0).any() and (df.parallel_threshold(0.1) > 0).all()


def test_parser_parallel_flags():
    from gesturediffusion_amd.utils.parser_util import generate_args
    a = generate_args(["--synthetic"])
    assert a.parallel_window == 0 and a.parallel_tolerance == 0.1                  # off by default
    a = generate_args(["--synthetic", "--parallel_window", "4", "--parallel_tolerance", "0", "--sampler", "ddim"])
    assert a.parallel_window == 4 and a.parallel_tolerance == 0 and a.rng == "philox"
    assert generate_args(["--synthetic", "--parallel_window", "64"]).sampler == "p"
    assert generate_args(["--synthetic", "--parallel_window", "8", "--guidance_refresh", "1"]).parallel_window == 8
    assert generate_args(["--synthetic", "--parallel_window", "8", "--layer_cache", "1", "3"]).layer_cache is None
    assert generate_args(["--synthetic", "--parallel_window", "8", "--guidance_interval", "200", "800"]).parallel_window == 8
    assert generate_args(["--synthetic", "--guidance_refresh", "2", "--layer_cache", "2", "3"]).parallel_window == 0
    for bad in (["--parallel_window", "8", "--sampler", "plms"], ["--parallel_window", "8", "--sampler", "unipc"],
                ["--parallel_window", "8", "--sampler", "dpmpp_sde"], ["--parallel_window", "8", "--guidance_refresh", "2"],
                ["--parallel_window", "8", "--layer_cache", "2", "3"], ["--parallel_window", "65"], ["--parallel_window", "-1"],
                ["--parallel_window", "8", "--parallel_tolerance", "-1"], ["--parallel_window", "8", "--parallel_tolerance", "nan"],
                ["--parallel_window", "8", "--rng", "torch"]):
        with pytest.raises(SystemExit):
            generate_args(["--synthetic"] + bad)


def test_parser_refuses_parallel_with_invert_gt(tmp_path):
    from gesturediffusion_amd.utils.parser_util import generate_args
    data = ["--dataset", "genea2023", "--data_dir", str(tmp_path), "--sampler", "ddim", "--invert_gt"]
    assert generate_args(data).invert_gt
    with pytest.raises(SystemExit):
        generate_args(data + ["--parallel_window", "8"])


def test_sample_chunks_refuses_what_the_window_cannot_run():
    from gesturediffusion_amd.sample.generate import sample_chunks
    seed = torch.zeros(2, 3, 1, 4)
    df = diffusion("cosine", "ddim10")
    with pytest.raises(ValueError, match="sampler='p' or 'ddim'"):
        sample_chunks(None, df, seed, None, 1, 10, 4, guidance_param=1.0, sampler="plms", rng="philox", parallel=(4, 0.1))
    with pytest.raises(ValueError, match="side by side"):
        sample_chunks(None, df, seed, None, 1, 10, 4, guidance_param=2.5, guidance_refresh=2, rng="philox", parallel=(4, 0.1))
    with pytest.raises(ValueError, match="side by side"):
        sample_chunks(None, df, seed, None, 1, 10, 4, guidance_param=1.0, layer_cache=(2, 1), rng="philox", parallel=(4, 0.1))
    with pytest.raises(ValueError, match="philox"):
        sample_chunks(None, df, seed, None, 1, 10, 4, guidance_param=1.0, rng="torch", parallel=(4, 0.1))
