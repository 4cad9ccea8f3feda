"""Host-side checks of the SDE-DPM-Solver++ multistep sampler (dpm_sde_coef_table, gdx_dpm_sde_step, gdx_dpm_sde_loop, the CLI
flags): no GPU needed.  The fp64 restatement and the covariance recursion live in dpm_sde_restatement.py; the constants the GPU
tests (test_gpu_dpm_sde.py) rely on are measured here, on the CPU."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import dpm_sde_restatement as S
from test_dpm_host import S2, analytic_x_T, diffusion

ETAS = [0.0, 0.5, 1.0]

# Worst relative error of the restatement's recurrence run in torch fp32 on the CPU against fp64 over the four analytic cases
# (logsnr20 / logsnr40 x orders 1..2, eta = 1, x_T and tape of shape (2, 3, 1, 4), seeds 0 and 1) measured 2.115e-7; the GPU
# test allows 4x over the recorded figure.
FP32_LOOP_WORST = 2.12e-7
FP32_LOOP_TOL = 4 * FP32_LOOP_WORST

# Order 1 at eta = 1 against p_sample, one step, in units of 2^-24 * (|phi*m0| + |a*x| + |s*z|).  Both are fp32 evaluations of
# one real number (the tables round the same fp64 posterior coefficients; p_sample's noise scale goes through
# exp(0.5*log(.)) in fp32).  On the CPU at t = 5 and 9 of ddim10 (cosine, 64 x 16 x 20 elements each) either op order lies
# within 2.381 units of the fp64 value (t = 5; 2.292 at t = 9), so two of them differ by at most twice the recorded worst case:
# that is the GPU bound.  (On the CPU the two differ by 0 units at both rows: the fp32 rows coincide there and the sum of the two
# mean terms commutes.)  No row needs an exception the way t = 1 did against DDIM.
P_SAMPLE_WORST_UNITS = 2.4
P_SAMPLE_BOUND_UNITS = 2 * P_SAMPLE_WORST_UNITS

# The statistical test (GPU test 16): linear schedule, logsnr20, eta = 1, N = 8 * 16 * 256 elements
STAT_SHAPE = (8, 16, 1, 256)
STAT_SEED = 2024
STAT_BOUND = 5 * np.sqrt(2.0 / (8 * 16 * 256))        # 3.9 %


def analytic_tape(n):
    """Noise of n steps for analytic_x_T()'s shape, fp64."""
    return torch.randn(n, 2, 3, 1, 4, generator=torch.Generator().manual_seed(1), dtype=torch.float64)


def p_sample_bound_unit(row, x, m0, z):
    """2^-24 * (|phi*m0| + |a*x| + |s*z|), elementwise, from rows [B, 8] of dpm_sde_coef_table(eta = 1): order 1 and p_sample are
    two fp32 evaluations of one real number, and these are the magnitudes their roundings act on."""
    c = lambda j: row[:, j].view(-1, 1, 1, 1).double()   # noqa: E731
    return 2.0 ** -24 * ((c(1) * m0.double()).abs() + (c(0) * x.double()).abs() + (c(7) * z.double()).abs())


def stat_prediction(order):
    df = diffusion("linear", "logsnr20")
    return S.sde_final_variance(df.alphas_cumprod, df.alphas_cumprod_prev, S2, order, 1.0)


# ------------------------------------------------------------------------------------------------------------------ table
@pytest.mark.parametrize("schedule", ["linear", "cosine"])
@pytest.mark.parametrize("respacing", [[1000], "ddim10", "logsnr20"])
@pytest.mark.parametrize("eta", ETAS)
def test_table_is_the_rounded_restatement(schedule, respacing, eta):
    """Each fp32 entry is np.float32 of the restatement's fp64 value, or within 1 fp32 ulp of it (the package evaluates closed
    forms, the restatement the update on unit vectors: the fp64 values can differ in their last bits)."""
    df = diffusion(schedule, respacing)
    got = df.dpm_sde_coef_table("cpu", eta)
    assert got.dtype == torch.float32 and tuple(got.shape) == (df.num_timesteps, 8)
    assert df.dpm_sde_coef_table("cpu", eta) is got                          # cached per (device, eta)
    assert df.dpm_sde_coef_table("cpu", eta + 0.25) is not got
    want = S.sde_weights(df.alphas_cumprod, df.alphas_cumprod_prev, eta)
    w32 = want.astype(np.float32)
    ulp = np.spacing(np.abs(w32)).astype(np.float64)
    diff = np.abs(got.numpy().astype(np.float64) - w32.astype(np.float64))
    assert (diff <= ulp).all(), np.argwhere(diff > ulp)[:5]
    assert float((diff == 0).mean()) > 0.9


@pytest.mark.parametrize("schedule", ["linear", "cosine"])
@pytest.mark.parametrize("respacing", [[1000], "ddim10", "logsnr20"])
def test_table_identities(schedule, respacing):
    df = diffusion(schedule, respacing)
    n = df.num_timesteps
    ode = df.dpm_coef_rows()
    # eta = 0: the ODE rows bit for bit in fp64, and no noise
    r0 = df.dpm_sde_coef_rows(0.0)
    assert r0.dtype == np.float64 and r0.shape == (n, 8)
    assert np.array_equal(r0[:, :4], ode[:, :4]) and (r0[:, 4:] == 0).all()
    # eta = 1: order 1 is the ancestral step with the posterior (FIXED_SMALL) variance, an fp64 algebraic identity
    r1 = df.dpm_sde_coef_rows(1.0)
    np.testing.assert_allclose(r1[1:, 1], df.posterior_mean_coef1[1:], rtol=1e-9, atol=0)
    np.testing.assert_allclose(r1[1:, 0], df.posterior_mean_coef2[1:], rtol=1e-9, atol=0)
    np.testing.assert_allclose(r1[1:, 7] ** 2, df.posterior_variance[1:], rtol=1e-9, atol=0)
    eps = np.finfo(np.float64).eps
    for eta in ETAS + [2.0]:
        rows = df.dpm_sde_coef_rows(eta)
        assert rows[0].tolist() == [0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
        assert (rows[:, 4:7] == 0).all() and (rows[n - 1, 2:4] == 0).all()
        w, phi = rows[1:n - 1, 2:4], rows[1:n - 1, 1]
        assert (np.abs(w.sum(axis=1) - phi) <= 4 * eps * np.abs(w).sum(axis=1)).all()      # w2_0 + w2_1 = phi
        assert (rows[1:, 7] > 0).all() if eta > 0 else (rows[:, 7] == 0).all()
        assert (rows[1:, 0] > 0).all() and (rows[1:, 0] <= ode[1:, 0]).all()                # a shrinks by exp(-eta*h)
    with pytest.raises(ValueError, match="eta"):
        df.dpm_sde_coef_rows(-0.1)


# ------------------------------------------------------------------------------------------------- the covariance recursion
@pytest.mark.parametrize("order,eta", [(1, 1.0), (2, 1.0), (2, 0.5)])
def test_covariance_recursion_matches_monte_carlo(order, eta):
    """The restatement's own loop in fp64 on N = 2^18 independent elements drawn from the exact marginal, against the closed-form
    recursion: a sample variance of N normals has relative standard deviation sqrt(2/N), the bound is 5 of them."""
    N = 1 << 18
    df = diffusion("linear", "logsnr20")
    ab, abp = df.alphas_cumprod, df.alphas_cumprod_prev
    g = S.gaussian_gain(ab, S2)
    rng = np.random.default_rng(10 * order + int(4 * eta))
    x_T = np.sqrt(ab[-1] * S2 + 1.0 - ab[-1]) * rng.standard_normal(N)
    tape = rng.standard_normal((len(ab), N))
    x = S.sde_loop(ab, abp, x_T, lambda x, i: g[i] * x, order, eta, tape)
    want = S.sde_final_variance(ab, abp, S2, order, eta)
    rel = float(np.mean(x * x) / want - 1.0)
    print(f"order {order} eta {eta}: Monte Carlo variance / recursion - 1 = {rel:+.4%} (bound {5 * np.sqrt(2 / N):.4%})")
    assert abs(rel) <= 5 * np.sqrt(2.0 / N)


def test_variance_table_conditions():
    """Linear schedule, s0^2 = 0.25, eta = 1 (the table of DESIGN.md 4e): second order converges, and beats the ancestral
    step at the same step count (measured ratios 3.4 and 5.3)."""
    e = {}
    for sp in ("logsnr10", "logsnr20", "logsnr40", "logsnr80"):
        df = diffusion("linear", sp)
        for order in (1, 2):
            e[order, sp] = S.sde_variance_error(df.alphas_cumprod, df.alphas_cumprod_prev, S2, order, 1.0)
        print(f"{sp} ({df.num_timesteps} steps): order 1 {e[1, sp]:+.1%}, order 2 {e[2, sp]:+.1%}, ODE 2M "
              f"{S.sde_variance_error(df.alphas_cumprod, df.alphas_cumprod_prev, S2, 2, 0.0):+.1%}")
    assert abs(e[2, "logsnr40"]) <= abs(e[2, "logsnr20"]) / 3
    assert abs(e[2, "logsnr20"]) <= abs(e[1, "logsnr20"]) / 4
    # the two predictions of the statistical GPU test are far apart next to its bound
    assert abs(stat_prediction(2) - stat_prediction(1)) / S2 > 0.4 > 10 * STAT_BOUND


def test_statistical_case_holds_on_the_cpu_with_the_chosen_seed():
    """GPU test 16 restated on the CPU: the fp64 restatement driven by the numpy restatement of the in-kernel Philox noise
    (oracle/philox.py: draw 0 scaled to the exact marginal as x_T, draw k + 1 at executed step k) with STAT_SEED stays inside
    STAT_BOUND of each order's own prediction, and outside it of the other order's."""
    from oracle import philox
    B, J, _, T = STAT_SHAPE
    df = diffusion("linear", "logsnr20")
    ab, abp = df.alphas_cumprod, df.alphas_cumprod_prev
    g = S.gaussian_gain(ab, S2)
    draw = lambda step: philox.normal(B, J * T, STAT_SEED, 0, step).astype(np.float64)   # noqa: E731
    x_T = np.sqrt(ab[-1] * S2 + 1.0 - ab[-1]) * draw(0)
    tape = [draw(k + 1) for k in range(len(ab))]
    for order in (1, 2):
        x = S.sde_loop(ab, abp, x_T, lambda x, i: g[i] * x, order, 1.0, tape)
        rel = float(np.mean(x * x) / stat_prediction(order) - 1.0)
        print(f"order {order}: sample variance / prediction - 1 = {rel:+.3%} (bound {STAT_BOUND:.3%})")
        assert abs(rel) <= STAT_BOUND
        assert abs(np.mean(x * x) / stat_prediction(3 - order) - 1.0) > STAT_BOUND


# ------------------------------------------------------------------------------------------ constants of the GPU tests
def test_fp32_recurrence_stays_inside_the_gpu_tolerance():
    """Where FP32_LOOP_TOL comes from: the restatement's recurrence in torch fp32 on the CPU against fp64, the four cases of the
    GPU test, same x_T and tape."""
    x_T = analytic_x_T()
    worst = 0.0
    for sp in ("logsnr20", "logsnr40"):
        df = diffusion("linear", sp)
        ab, abp = df.alphas_cumprod, df.alphas_cumprod_prev
        tape = analytic_tape(len(ab))
        g64 = S.gaussian_gain(ab, S2)
        g32 = torch.from_numpy(g64).float()
        for order in (1, 2):
            want = S.sde_loop(ab, abp, x_T.numpy(), lambda x, i: g64[i] * x, order, 1.0, tape.numpy())
            got = S.sde_loop(ab, abp, x_T.float(), lambda x, i: g32[i] * x, order, 1.0, tape.float(), xp=torch)
            assert got.dtype == torch.float32
            rel = float(np.abs(got.double().numpy() - want).max() / np.abs(want).max())
            print(f"{sp} order {order}: fp32 recurrence rel err {rel:.3e}")
            worst = max(worst, rel)
    assert worst <= FP32_LOOP_WORST, worst


def test_order1_vs_p_sample_bound_holds_on_the_cpu():
    """Before the GPU test relies on P_SAMPLE_BOUND_UNITS: torch-fp32 restatements of both op orders at t in {5, 9} of ddim10,
    the fp64 value as arbiter.  Each lies within the recorded worst case of it, so their difference within twice that."""
    df = diffusion("cosine", "ddim10")
    anc, sde, rows64 = df.coef_table(0, "cpu"), df.dpm_sde_coef_table("cpu", 1.0), torch.from_numpy(df.dpm_sde_coef_rows(1.0))
    g = torch.Generator().manual_seed(12)
    for t in (5, 9):
        tt = torch.full((64,), t)
        x, m0, z = (torch.randn(64, 16, 1, 20, generator=g) * s for s in (1.0, 1.5, 1.0))
        c = lambda tab, j: tab[tt][:, j].view(-1, 1, 1, 1)   # noqa: E731
        v_p = (c(anc, 0) * m0 + c(anc, 1) * x) + c(anc, 2) * z
        v_sde = (c(sde, 0) * x + c(sde, 1) * m0) + c(sde, 7) * z
        assert v_p.dtype == v_sde.dtype == torch.float32
        v64 = rows64[t, 0] * x.double() + rows64[t, 1] * m0.double() + rows64[t, 7] * z.double()
        unit = p_sample_bound_unit(sde[tt], x, m0, z)
        for what, d in (("p_sample vs fp64", v_p.double() - v64), ("order 1 vs fp64", v_sde.double() - v64),
                        ("p_sample vs order 1", v_p.double() - v_sde.double())):
            ratio = float((d.abs() / unit.clamp_min(1e-300)).max())
            print(f"t={t} {what}: {ratio:.3f} units of 2^-24 * magnitudes")
            assert ratio <= (P_SAMPLE_BOUND_UNITS if what == "p_sample vs order 1" else P_SAMPLE_WORST_UNITS), (t, what, ratio)


# ------------------------------------------------------------------------------------------------------------------- C ABI
def _lib_or_skip():
    from gesturediffusion_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgdx.so not built (run python __graft_entry__.py)")
    return _lib


def _refused(lib, rc, text, who):
    err = lib.gdx_last_error()
    return rc < 0 and text in err and who in err


def test_dpm_sde_step_refusals_without_gpu():
    """gdx_dpm_sde_step is stateless: every refusal is decided from the argument struct (addresses are never followed) and
    names the entry point."""
    _lib = _lib_or_skip()
    lib = _lib.load()
    P, who = 4096, b"gdx_dpm_sde_step:"                 # a non-null address; a refused call reads nothing through it
    assert _refused(lib, lib.gdx_dpm_sde_step(None, None), b"null argument", who)
    assert _refused(lib, lib.gdx_dpm_sde_step(C.byref(_lib.DpmSdeStepArgs()), None), b"null argument", who)
    ok = dict(order=1, batch=2, njoints=3, frames=5, coef=P, x=P, x0_cond=P, out=P)
    step = lambda **kw: lib.gdx_dpm_sde_step(C.byref(_lib.DpmSdeStepArgs(**{**ok, **kw})), None)   # noqa: E731
    for missing in ("coef", "x", "x0_cond", "out"):
        assert _refused(lib, step(**{missing: None}), b"null argument", who), missing
    for order in (0, 3, -1):
        assert _refused(lib, step(order=order), b"order must be", who), order
    assert _refused(lib, step(batch=65536), b"bad shape", who) and _refused(lib, step(frames=-1), b"bad shape", who)
    assert _refused(lib, step(x0_uncond=P), b"CFG needs scale", who)
    assert _refused(lib, step(inpaint_mask=P), b"mask without motion", who)
    assert _refused(lib, step(order=2), b"missing history", who)         # order 2 reads one older prediction
    a = _lib.DpmSdeStepArgs(**{**ok, "order": 2, "pred_out": P})
    a.hist[0] = P
    assert _refused(lib, lib.gdx_dpm_sde_step(C.byref(a), None), b"aliases a history slot", who)
    assert step(batch=0) == 0 and step(batch=0, noise=P) == 0            # nothing to do is not an error


def test_dpm_sde_loop_refusals_without_gpu():
    """The argument checks of gdx_dpm_sde_loop need no handle: they come first, then the null handle, then readiness."""
    _lib = _lib_or_skip()
    lib = _lib.load()
    P, who = 4096, b"gdx_dpm_sde_loop:"
    ok = dict(mode=0, order=2, num_steps=10, first_index=9, coef=P, timestep_map=P, x=P, hist=P)
    loop = lambda **kw: lib.gdx_dpm_sde_loop(None, C.byref(_lib.DpmSdeLoopArgs(**{**ok, **kw})), None)   # noqa: E731
    assert _refused(lib, lib.gdx_dpm_sde_loop(None, None, None), b"null argument", who)
    for missing in ("coef", "timestep_map", "x"):
        assert _refused(lib, loop(**{missing: None}), b"null argument", who), missing
    assert _refused(lib, loop(mode=3), b"bad mode", who) and _refused(lib, loop(mode=-1), b"bad mode", who)
    assert _refused(lib, loop(mode=2), b"needs scale", who)
    for bad in (dict(num_steps=0), dict(first_index=10), dict(first_index=-1), dict(k_base=-1), dict(run_steps=-1),
                dict(first_index=5, k_base=5), dict(first_index=3, run_steps=5)):
        assert _refused(lib, loop(**bad), b"bad step range", who), bad
    for order in (0, 3, -2):
        assert _refused(lib, loop(order=order), b"order must be", who), order
    assert _refused(lib, loop(inpaint_mask=P), b"mask without motion", who)
    assert _refused(lib, loop(hist=None), b"missing history", who)
    assert _refused(lib, loop(order=1, hist=None), b"null handle", who)   # first order keeps no history
    assert _refused(lib, loop(noise_tape=P), b"null handle", who)         # every argument in order: only the handle is missing
    h = C.c_void_p()
    cfg = _lib.Config(arch=1, njoints=16, latent_dim=128, ff_size=256, num_layers=2, num_heads=4, seed_poses=10, mfcc_dim=26,
                      cl_head=8, window=10)
    if lib.gdx_create(C.byref(cfg), C.byref(h)) == 0:          # where a handle can be made without a device: not prepared
        assert _refused(lib, lib.gdx_dpm_sde_loop(h, C.byref(_lib.DpmSdeLoopArgs(**ok)), None), b"gdx_prepare", who)
        lib.gdx_destroy(h)


# --------------------------------------------------------------------------------------------------------------------- CLI
def test_parser_takes_dpmpp_sde_its_order_and_eta(capsys):
    from gesturediffusion_amd.utils.parser_util import generate_args
    a = generate_args(["--synthetic", "--sampler", "dpmpp_sde", "--dpm_eta", "0.5"])
    assert a.sampler == "dpmpp_sde" and a.dpm_eta == 0.5 and a.dpm_order == 2 and a.eta == 0.0
    assert generate_args(["--synthetic", "--sampler", "dpmpp_sde", "--dpm_order", "1"]).dpm_order == 1
    assert generate_args(["--synthetic"]).dpm_eta == 1.0
    assert generate_args(["--synthetic", "--sampler", "dpmpp", "--dpm_order", "3"]).dpm_order == 3     # the ODE solver keeps it
    with pytest.raises(SystemExit):
        generate_args(["--synthetic", "--sampler", "dpmpp_sde", "--dpm_order", "3"])
    assert "orders 1 and 2 only" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        generate_args(["--synthetic", "--sampler", "dpmpp_sde", "--dpm_eta", "-1"])


def test_python_refusals_need_no_device():
    df = diffusion("linear", "logsnr20")
    for order in (0, 3):
        with pytest.raises(ValueError, match="order is invalid"):
            df.dpm_solver_sde_sample_loop(None, (2, 3, 1, 4), order=order)
    with pytest.raises(ValueError, match="eta must be"):
        df.dpm_solver_sde_sample_loop(None, (2, 3, 1, 4), eta=-0.5)
    with pytest.raises(ValueError, match="rng must be"):
        df.dpm_solver_sde_sample_loop(None, (2, 3, 1, 4), rng="numpy")
    for kw in (dict(cond_fn_with_grad=True), dict(randomize_class=True)):
        with pytest.raises(NotImplementedError):
            df.dpm_solver_sde_sample_loop(None, (2, 3, 1, 4), **kw)
        with pytest.raises(NotImplementedError):
            next(df.dpm_solver_sde_sample_loop_progressive(None, (2, 3, 1, 4), **kw))
