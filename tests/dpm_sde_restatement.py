"""fp64 numpy restatement of the SDE-DPM-Solver++ multistep sampler (include/gdx.h at gdx_dpm_sde_step / gdx_dpm_sde_loop), orders
1 and 2, written from the update in its D1 form (Lu et al. 2022, arXiv:2211.01095, at eta = 1; the eta generalisation is the
midpoint form of k-diffusion's dpmpp_2m_sde with alpha != 1) -- never from collected weights -- plus the closed-form covariance
recursion of the linear-Gaussian case.  A helper, not a test; it shares no code with the package."""
import numpy as np

from dpm_restatement import effective_order, gaussian_gain, lam_of, schedule  # noqa: F401  (re-exported for the tests)


def sde_update(abar, abar_prev, i, order, eta, x, m, z, xp=np):
    """x' of one step at index i: m = x0 predictions, newest first (m[0] this step's, m[1] of index i + 1), z the step's
    standard normal.  xp: the array module of x / m / z (numpy, or torch for the fp32 restatement; the scalar coefficients stay
    Python floats)."""
    if abar_prev[i] == 1.0:                                   # the step to sigma = 0: h = inf, x' = m0, no noise
        assert order == 1
        return m[0] + 0.0 * x
    lam = lam_of(abar)
    alpha_p, sigma_p, sigma_i = np.sqrt(abar_prev[i]), np.sqrt(1.0 - abar_prev[i]), np.sqrt(1.0 - abar[i])
    h = 0.5 * np.log(abar_prev[i] / (1.0 - abar_prev[i])) - lam[i]
    f = float if xp is not np else (lambda v: v)
    decay = -np.expm1(-(1.0 + eta) * h)                       # 1 - exp(-(1 + eta) h)
    out = f(sigma_p / sigma_i * np.exp(-eta * h)) * x + f(alpha_p * decay) * m[0]
    if order == 2:
        r0 = (lam[i] - lam[i + 1]) / h
        out = out + f(0.5 * alpha_p * decay) * ((m[0] - m[1]) / f(r0))
    else:
        assert order == 1
    return out + f(sigma_p * np.sqrt(-np.expm1(-2.0 * eta * h))) * z


def sde_weights(abar, abar_prev, eta):
    """[n, 8] fp64 rows (a, w1_0, w2_0, w2_1, 0, 0, 0, s): the update is linear, so its weights are its values on the unit
    vectors of (x, m0, m1, z).  Entries that would need an index >= n, and row 0's second order, are 0."""
    n = len(abar)
    rows = np.zeros((n, 8))
    one, zero = np.float64(1.0), np.float64(0.0)
    for i in range(n):
        rows[i, 0] = sde_update(abar, abar_prev, i, 1, eta, one, [zero, zero], zero)
        rows[i, 1] = sde_update(abar, abar_prev, i, 1, eta, zero, [one, zero], zero)
        rows[i, 7] = sde_update(abar, abar_prev, i, 1, eta, zero, [zero, zero], one)
        if 0 < i < n - 1:
            rows[i, 2] = sde_update(abar, abar_prev, i, 2, eta, zero, [one, zero], zero)
            rows[i, 3] = sde_update(abar, abar_prev, i, 2, eta, zero, [zero, one], zero)
    return rows


def sde_loop(abar, abar_prev, x_T, denoise, order, eta, tape, first_index=None, xp=np):
    """The whole loop from index first_index (default: the last) down to 0; denoise(x, i) -> x0 prediction at index i; tape[k] is
    the noise of executed step k."""
    x, hist = x_T, []
    first_index = len(abar) - 1 if first_index is None else first_index
    for k, i in enumerate(range(first_index, -1, -1)):
        hist.insert(0, denoise(x, i))
        del hist[2:]
        x = sde_update(abar, abar_prev, i, effective_order(order, k, i), eta, x, hist, tape[k], xp=xp)
    return x


# ---- the linear-Gaussian case: data N(0, s2 * I) and its exact denoiser m_i = g_i * x_i.  Every element is an independent
# scalar chain, linear in (x_k, x_{k-1}) with independent noise added, so its covariance obeys a closed recursion.
def sde_final_variance(abar, abar_prev, s2, order, eta):
    """Variance of the loop's final sample when x_T is drawn from the exact marginal N(0, abar_T*s2 + 1 - abar_T).  State
    (x_k, x_{k-1}); per step the 2x2 linear map M = [[a + w0*g_i, w1*g_{i+1}], [1, 0]] and s^2 added to the x variance, with
    (a, w0, w1, s) read off sde_update on unit vectors."""
    n = len(abar)
    g = gaussian_gain(abar, s2)
    one, zero = np.float64(1.0), np.float64(0.0)
    P = np.array([[abar[-1] * s2 + 1.0 - abar[-1], 0.0], [0.0, 0.0]])
    for k, i in enumerate(range(n - 1, -1, -1)):
        o = effective_order(order, k, i)
        a = sde_update(abar, abar_prev, i, o, eta, one, [zero, zero], zero)
        w0 = sde_update(abar, abar_prev, i, o, eta, zero, [one, zero], zero)
        w1 = sde_update(abar, abar_prev, i, o, eta, zero, [zero, one], zero) if o == 2 else 0.0
        s = sde_update(abar, abar_prev, i, o, eta, zero, [zero, zero], one)
        M = np.array([[a + w0 * g[i], w1 * g[i + 1] if o == 2 else 0.0], [1.0, 0.0]])
        P = M @ P @ M.T
        P[0, 0] += s * s
    return float(P[0, 0])


def sde_variance_error(abar, abar_prev, s2, order, eta):
    """Relative error of the final sample's variance against the data's."""
    return sde_final_variance(abar, abar_prev, s2, order, eta) / s2 - 1.0
