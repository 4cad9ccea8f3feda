"""Host-side checks of RePaint resampling (gdx_set_resample, repaint_sample_loop, sample.generate --edit_mode / --resample; the rule
is in include/gdx.h): no GPU needed.  The restatement lives in resample_restatement.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import resample_restatement as R
from conftest import REPO
from test_dpm_host import diffusion

GRID = [(N, jump, repeats) for N in (1, 2, 3, 6, 7, 10, 20, 50) for jump in (1, 2, 3, 5, 7, 10, 19, 20, 60) for repeats in (1, 2, 3, 10)]


def _words(plan):
    return ["r%d" % h[1] if h[0] == "r" else "f%d,%d" % (h[1], h[2]) for h in plan]


# ------------------------------------------------------------------------------------------------------------------ the plan
def test_known_answer():
    df = diffusion("cosine", [6])
    want = "r5 r4 r3 r2 f2,4 r3 r2 r1 r0 f0,2 r1 r0".split()
    assert _words(df.resample_plan(2, 2)) == want == _words(R.hops(6, 2, 2))


@pytest.mark.parametrize("steps", [2, 3, 6, 7, 10, 20, 50])
def test_plan_against_the_restatement_and_the_call_count(steps):
    """Over the grid: the package's plan is the restatement's (RePaint's single steps, ascending runs joined); the reverse hops
    number N + n_levels (repeats - 1) jump; every forward hop climbs exactly `jump` from a jump level; no hop leaves 0 .. N; the
    walk ends at level 0; repeats = 1 and jump >= N give the plain descent; skip_timesteps shifts N."""
    df = diffusion("cosine", [steps])
    for N, jump, repeats in GRID:
        if N > steps:
            continue
        skip = steps - N
        plan = df.resample_plan(jump, repeats, skip_timesteps=skip)
        assert plan == R.hops(N, jump, repeats), (N, jump, repeats)
        n_levels = len([l for l in range(0, N, jump) if l + jump < N])
        assert sum(h[0] == "r" for h in plan) == N + n_levels * (repeats - 1) * jump == R.calls(N, jump, repeats)
        assert sum(h[0] == "f" for h in plan) == n_levels * (repeats - 1)
        level = N
        for h in plan:
            if h[0] == "r":
                assert h[1] == level - 1
                level -= 1
            else:
                assert h[1] == level and h[2] == level + jump and level % jump == 0 and level + jump < N
                level = h[2]
            assert 0 <= level <= N
        assert level == 0
        if repeats == 1 or jump >= N:
            assert plan == [("r", i) for i in range(N - 1, -1, -1)]
    assert df.resample_plan(np.int64(2), np.int32(2)) == df.resample_plan(2, 2)


def test_jump_edges():
    """jump = N - 1 has the single jump level 0; jump = N - 2 as well (level N - 2 would need level 2N - 4 + ... >= N)."""
    df = diffusion("cosine", [6])
    assert _words(df.resample_plan(5, 2)) == "r5 r4 r3 r2 r1 r0 f0,5 r4 r3 r2 r1 r0".split()
    assert _words(df.resample_plan(6, 5)) == "r5 r4 r3 r2 r1 r0".split()
    assert _words(df.resample_plan(3, 2)) == "r5 r4 r3 r2 r1 r0 f0,3 r2 r1 r0".split()      # level 3: 3 + 3 < 6 fails
    assert _words(df.resample_plan(1, 2, skip_timesteps=3)) == "r2 r1 f1,2 r1 r0 f0,1 r0".split()


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++") if subprocess.run(
        ["sh", "-c", f"command -v {c}"], capture_output=True).returncode == 0), None)
    assert cxx, "no C++ compiler"
    exe = os.path.join(str(tmp_path_factory.mktemp("resample_plan")), "resample_plan_probe")
    built = subprocess.run([cxx, "-std=c++17", "-Werror", "-I", os.path.join(REPO, "gesturediffusion_amd", "csrc"),
                            os.path.join(REPO, "tests", "resample_plan_probe.cpp"), "-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr

    def run(lines):
        got = subprocess.run([exe], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()
        assert len(got) == len(lines)
        return [ln.split() for ln in got]
    return run


def test_header_walk_equals_the_python_plan(probe):
    """csrc/gdx_resample_plan.h, compiled with the host compiler alone: the same hops, call count and hop count over the grid."""
    got = probe([f"W {N} {jump} {repeats}" for N, jump, repeats in GRID])
    for (N, jump, repeats), words in zip(GRID, got):
        plan = diffusion("cosine", [max(N, 2)]).resample_plan(jump, repeats, skip_timesteps=max(N, 2) - N)   # no 1-step schedule
        assert words[2:] == _words(plan), (N, jump, repeats)
        assert int(words[0]) == sum(h[0] == "r" for h in plan) and int(words[1]) == len(plan)


# ---------------------------------------------------------------------------------------------------------- the coefficients
@pytest.mark.parametrize("schedule", ["cosine", "linear"])
@pytest.mark.parametrize("respacing", [[1000], "ddim50"])
def test_coefficients(schedule, respacing, probe):
    """a^2 + b^2 = 1 to 1 ulp in fp64 (before the rounding to fp32); a hop from level 0 uses abar = 1; the fp32 rows have the bits of
    the numpy fp64 -> fp32 statement, and so have the header's."""
    df = diffusion(schedule, respacing)
    n = df.num_timesteps
    for jump, repeats in ((1, 2), (7, 3), (10, 2), (n - 1, 2)):
        plan = df.resample_plan(jump, repeats)
        fwd = [h for h in plan if h[0] == "f"]
        rows = df.resample_coef(plan)
        assert rows.dtype == np.float32 and rows.shape == (len(fwd), 2) and len(fwd) > 0
        lvl = np.concatenate(([1.0], df.alphas_cumprod))
        lines = []
        for row, (_, frm, to) in zip(rows, fwd):
            r = lvl[to] / lvl[frm]
            a64, b64 = np.sqrt(r), np.sqrt(1.0 - r)
            assert abs(a64 * a64 + b64 * b64 - 1.0) <= np.finfo(np.float64).eps
            want = R.coef(df.alphas_cumprod, frm, to)
            assert row[0].tobytes() == want[0].tobytes() and row[1].tobytes() == want[1].tobytes()
            if frm == 0:
                assert row[0].tobytes() == np.float32(np.sqrt(df.alphas_cumprod[to - 1])).tobytes()
                assert row[1].tobytes() == np.float32(np.sqrt(1.0 - df.alphas_cumprod[to - 1])).tobytes()
            lines.append(f"C {frm} {to} {n} " + " ".join(float(v).hex() for v in df.alphas_cumprod))
        assert any(frm == 0 for _, frm, _ in fwd)
        got = probe(lines)
        assert [(int(a), int(b)) for a, b in got] == [tuple(int(v) for v in row.view(np.uint32)) for row in rows]
    assert df.resample_coef(df.resample_plan(3, 1)).shape == (0, 2)


# --------------------------------------------------------------------------------------------------------- the analytic case
@pytest.mark.parametrize("kind", ["p", "ddim"])
def test_resampling_halves_the_analytic_bias(kind):
    """Prior N(0, [[1, 0.9], [0.9, 1]]) with its exact linear denoiser, dimension 0 inpainted to 1.5, cosine schedule on 50 evenly
    strided steps, float64, 20 000 chains of a fixed seed.  Truth for dimension 1: mean 1.35, variance 0.19.  At (jump, repeats) =
    (10, 5) the errors |mean - 1.35| and |var - 0.19| are each below half their values at repeats = 1.  Measured at 200 000 chains:
    mean p 0.098 against 0.429, ddim 0.173 against 0.695; variance p 0.001 against 0.142, ddim 0.040 against 0.308; standard error
    of the mean about 3e-3 at this sample count."""
    m1, v1 = R.analytic(kind, 10, 1)
    m5, v5 = R.analytic(kind, 10, 5)
    print(f"{kind}: repeats 1 mean {m1:.4f} var {v1:.4f}; (10, 5) mean {m5:.4f} var {v5:.4f}")
    assert abs(m5 - R.TRUE_MEAN) < 0.5 * abs(m1 - R.TRUE_MEAN)
    assert abs(v5 - R.TRUE_VAR) < 0.5 * abs(v1 - R.TRUE_VAR)


# ----------------------------------------------------------------------------------------------------------- the ValueErrors
def _never():
    def plain(xx, t, **k):
        raise AssertionError("the model was called")
    return plain


def test_argument_errors_come_before_the_first_model_call():
    df = diffusion("cosine", "ddim10")
    shape = (2, 16, 1, 20)
    kw = dict(model_kwargs={"y": {}}, device=torch.device("cpu"), noise=torch.zeros(shape))
    for bad in (0, -1, 2.0, True, "2", None):
        with pytest.raises(ValueError, match="jump must be an int >= 1"):
            df.repaint_sample_loop(_never(), shape, jump=bad, repeats=2, **kw)
        with pytest.raises(ValueError, match="repeats must be an int >= 1"):
            df.repaint_sample_loop(_never(), shape, jump=2, repeats=bad, **kw)
        with pytest.raises(ValueError, match="must be an int >= 1"):
            df.resample_plan(bad, 2)
    for sampler in ("plms", "dpmpp", "unipc", "P", None):
        with pytest.raises(ValueError, match="runs sampler 'p' or 'ddim'"):
            df.repaint_sample_loop(_never(), shape, sampler=sampler, **kw)
    with pytest.raises(ValueError, match="rng must be"):
        df.repaint_sample_loop(_never(), shape, rng="numpy", **kw)
    hops = len(df.resample_plan(2, 2))
    for n in (hops, hops + 2, 11):
        with pytest.raises(ValueError, match=f"1 \\+ {hops}, got {n}"):
            df.repaint_sample_loop(_never(), shape, jump=2, repeats=2, noise_tape=torch.zeros(n, *shape), **kw)
    with pytest.raises(ValueError, match="const_noise-style broadcast"):
        df.repaint_sample_loop(_never(), shape, jump=2, repeats=2, noise_tape=torch.zeros(1 + hops, 1, 16, 1, 20), **kw)


def test_options_with_memory_are_refused_on_both_routes():
    from gesturediffusion_amd.model.cfg_sampler import ClassifierFreeSampleModel
    df = diffusion("cosine", "ddim10")

    class Never(ClassifierFreeSampleModel):
        def __init__(self):                                  # no inner model: nothing here may reach it
            torch.nn.Module.__init__(self)

        def forward(self, *a, **k):
            raise AssertionError("the model was called")

    shape = (2, 16, 1, 20)
    for fused in (True, False):
        kw = dict(device=torch.device("cpu"), noise=torch.zeros(shape), jump=2, repeats=2, fused=fused)
        with pytest.raises(ValueError, match=r"y\['guidance_refresh'\] = 2 does not combine with repaint_sample_loop.*forward hop"):
            df.repaint_sample_loop(Never(), shape, model_kwargs={"y": {"guidance_refresh": 2, "scale": torch.ones(2)}}, **kw)
        for model in (Never(), _never()):
            with pytest.raises(ValueError, match=r"y\['layer_cache'\] = \(2, 1\) does not combine with repaint_sample_loop"):
                df.repaint_sample_loop(model, shape, model_kwargs={"y": {"layer_cache": (2, 1)}}, **kw)


# ------------------------------------------------------------------------------------------------------------------- the CLI
def test_parser_flags():
    from gesturediffusion_amd.utils.parser_util import generate_args
    a = generate_args(["--synthetic"])
    assert a.edit_mode is None and a.resample is None and (a.prefix_end, a.suffix_start) == (0.25, 0.75)      # off by default
    a = generate_args(["--synthetic", "--edit_mode", "in_between", "--prefix_end", "0.1", "--suffix_start", "0.5", "--resample", "10", "5"])
    assert (a.edit_mode, a.prefix_end, a.suffix_start, a.resample) == ("in_between", 0.1, 0.5, (10, 5))
    assert generate_args(["--synthetic", "--resample", "3", "2", "--sampler", "ddim"]).resample == (3, 2)     # without --edit_mode
    assert generate_args(["--synthetic", "--resample", "3", "1"]).resample == (3, 1)
    assert generate_args(["--synthetic", "--edit_mode", "in_between", "--sampler", "plms"]).edit_mode == "in_between"
    assert generate_args(["--synthetic", "--edit_mode", "upper_body"]).edit_mode == "upper_body"               # refused by main


def test_parser_refusals(tmp_path, capsys):
    from gesturediffusion_amd.utils.parser_util import generate_args
    for bad, text in ((["--resample", "10", "5", "--sampler", "plms"], "--resample runs --sampler p or ddim only"),
                      (["--resample", "10", "5", "--sampler", "dpmpp"], "--resample runs --sampler p or ddim only"),
                      (["--resample", "10", "5", "--sampler", "dpmpp_sde"], "--resample runs --sampler p or ddim only"),
                      (["--resample", "10", "5", "--sampler", "unipc"], "--resample runs --sampler p or ddim only"),
                      (["--resample", "10", "5", "--guidance_refresh", "2"], "--resample runs no guidance refresh"),
                      (["--resample", "10", "5", "--layer_cache", "2", "3"], "--resample runs no layer cache"),
                      (["--resample", "10", "5", "--parallel_window", "4"], "--resample does not combine with --parallel_window"),
                      (["--resample", "0", "5"], "must both be at least 1"), (["--resample", "10", "0"], "must both be at least 1"),
                      (["--resample", "10"], "expected 2 arguments"), (["--edit_mode", "lower_body"], "invalid choice"),
                      (["--prefix_end", "0.8"], "0 <= prefix_end <= suffix_start <= 1"),
                      (["--suffix_start", "1.5"], "0 <= prefix_end <= suffix_start <= 1"),
                      (["--prefix_end", "-0.1"], "0 <= prefix_end <= suffix_start <= 1")):
        with pytest.raises(SystemExit):
            generate_args(["--synthetic"] + bad)
        assert text in capsys.readouterr().err, bad
    data = ["--dataset", "genea2023", "--data_dir", str(tmp_path), "--sampler", "ddim", "--invert_gt"]
    with pytest.raises(SystemExit):
        generate_args(data + ["--resample", "10", "5"])
    assert "--resample does not combine with --invert_gt" in capsys.readouterr().err


def test_sample_chunks_refusals_and_the_edit_mask():
    from gesturediffusion_amd.sample.generate import edit_mask, sample_chunks, synthetic_ground_truth
    args = (None, diffusion("cosine", "ddim10"), torch.zeros(2, 16, 1, 10), None, 1, 20, 10)
    for sampler in ("plms", "dpmpp", "dpmpp_sde", "unipc"):
        with pytest.raises(ValueError, match="resample needs sampler='p' or 'ddim'"):
            sample_chunks(*args, sampler=sampler, resample=(2, 2))
    for kw in (dict(guidance_refresh=2, guidance_param=2.5), dict(layer_cache=(2, 1)), dict(parallel=(4, 0.1), rng="philox"),
               dict(invert_of_chunk=lambda c: None, sampler="ddim")):
        with pytest.raises(ValueError, match="resample runs neither"):
            sample_chunks(*args, resample=(2, 2), **kw)
    with pytest.raises(NotImplementedError, match="HumanML"):
        edit_mask("upper_body", 0.25, 0.75, (2, 16, 1, 20), "cpu")
    with pytest.raises(ValueError, match="edit_mode"):
        edit_mask("between", 0.25, 0.75, (2, 16, 1, 20), "cpu")
    m = edit_mask("in_between", 0.25, 0.75, (2, 16, 1, 20), "cpu")
    assert m.dtype == torch.bool and m.shape == (2, 16, 1, 20)
    assert bool(m[..., :5].all()) and bool(m[..., 15:].all()) and not bool(m[..., 5:15].any())
    m = edit_mask("in_between", 0.3, 0.3, (1, 2, 1, 7), "cpu")                   # an empty gap: everything is kept
    assert bool(m.all())
    m = edit_mask("in_between", 0.0, 1.0, (1, 2, 1, 7), "cpu")                   # everything is generated
    assert not bool(m.any())
    a, b = synthetic_ground_truth(10, 3, 16, 20, 2), synthetic_ground_truth(10, 3, 16, 20, 2)
    assert len(a) == 2 and a[0].shape == (3, 16, 1, 20) and all(torch.equal(u, v) for u, v in zip(a, b))
    assert not torch.equal(a[0], a[1]) and not torch.equal(a[0], synthetic_ground_truth(11, 3, 16, 20, 2)[0])


# ---------------------------------------------------------------------------------------------------------------- the header
def test_header_states_the_rule_at_the_setter():
    hdr = open(os.path.join(REPO, "include", "gdx.h")).read()
    rule = hdr[hdr.index("int gdx_sample_loop("):hdr.index("int gdx_set_resample(")]
    for phrase in ("arXiv:2201.09865", "first_index + 1", "l + jump < N", "r5 r4 r3 r2 f(2->4) r3 r2 r1 r0 f(0->2) r1 r0",
                   "N + n_levels * (repeats - 1) * jump", "sqrt(1 - r)", "rounded to fp32 once", "gdx_randn followed by gdx_q_sample",
                   "Philox draw k + 1", "WHOLE loop's first", "token-major", "graph", "dump_steps", "const_noise", "gdx_plms_loop",
                   "gdx_dpm_loop", "gdx_dpm_sde_loop", "gdx_unipc_loop", "gdx_ddim_reverse_loop", "gdx_parallel_loop", "gdx_bpd_loop",
                   "trained"):
        assert phrase in rule, phrase


# --------------------------------------------------------------------------------------------------------------------- C ABI
def test_setter_refusals_need_no_device():
    from gesturediffusion_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgdx.so not built (run python __graft_entry__.py)")
    lib = _lib.load()
    ab = np.ascontiguousarray(diffusion("cosine", "ddim10").alphas_cumprod, dtype=np.float64)
    assert lib.gdx_set_resample(None, 2, 2, ab.ctypes.data, 10) == -1
    assert b"gdx_set_resample: null handle" in lib.gdx_last_error()
    h = C.c_void_p()
    cfg = _lib.Config(arch=1, njoints=16, latent_dim=128, ff_size=256, num_layers=2, num_heads=4, seed_poses=10, mfcc_dim=26,
                      cl_head=8, window=10)
    if lib.gdx_create(C.byref(cfg), C.byref(h)) == 0:          # where a handle can be made without a device
        for jump, repeats, text in ((0, 2, b"jump must be at least 1"), (-3, 2, b"jump must be at least 1"),
                                    (2, 0, b"repeats must be at least 1"), (2, -1, b"repeats must be at least 1")):
            assert lib.gdx_set_resample(h, jump, repeats, ab.ctypes.data, 10) == -1
            assert text in lib.gdx_last_error()
        assert lib.gdx_set_resample(h, 2, 2, None, 10) == -1 and b"needs alpha_bar" in lib.gdx_last_error()
        assert lib.gdx_set_resample(h, 2, 2, ab.ctypes.data, 0) == -1 and b"needs alpha_bar" in lib.gdx_last_error()
        for bad in (ab[::-1].copy(), np.append(ab[:-1], 0.0), np.append(ab[:-1], np.nan), np.append(1.5, ab[1:])):
            assert lib.gdx_set_resample(h, 2, 2, bad.ctypes.data, 10) == -1
            assert b"alpha_bar must lie in (0, 1] and must not increase" in lib.gdx_last_error()
        assert lib.gdx_set_resample(h, 2, 2, ab.ctypes.data, 10) == 0
        assert lib.gdx_set_resample(h, 20, 3, ab.ctypes.data, 10) == 0            # a jump longer than the schedule: no forward hop
        assert lib.gdx_set_resample(h, 7, 1, None, 0) == 0                        # off: alpha_bar is not looked at
        lib.gdx_destroy(h)
