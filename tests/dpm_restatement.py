"""fp64 numpy restatement of the DPM-Solver++ multistep sampler (include/gdx.h at gdx_dpm_step / gdx_dpm_loop), written from
the recurrences in their D1 / D2 form (Lu et al. 2022, arXiv:2211.01095) -- never from collected weights -- plus the analytic
Gaussian case the tests measure convergence on.  A helper, not a test; it shares no code with the package."""
import numpy as np


def schedule(betas):
    """(abar, abar_prev) of a beta schedule, fp64."""
    abar = np.cumprod(1.0 - np.asarray(betas, dtype=np.float64))
    return abar, np.append(1.0, abar[:-1])


def lam_of(abar):
    return 0.5 * np.log(abar / (1.0 - abar))


def effective_order(order, k, i):
    """Executed step k of a loop, at index i."""
    return min(order, k + 1, i + 1)


def dpm_update(abar, abar_prev, i, order, x, m, xp=np):
    """x' of one step at index i: m = x0 predictions, newest first (m[0] this step's, m[1] of index i + 1, m[2] of i + 2).
    xp: the array module of x / m (numpy, or torch for the fp32 restatement; the scalar coefficients stay Python floats)."""
    if abar_prev[i] == 1.0:                                   # the step to sigma = 0: h = inf, x' = m0
        assert order == 1
        return m[0] + 0.0 * x
    lam = lam_of(abar)
    alpha_p, sigma_p, sigma_i = np.sqrt(abar_prev[i]), np.sqrt(1.0 - abar_prev[i]), np.sqrt(1.0 - abar[i])
    h = 0.5 * np.log(abar_prev[i] / (1.0 - abar_prev[i])) - lam[i]
    em1 = np.expm1(-h)
    f = float if xp is not np else (lambda v: v)
    first = f(sigma_p / sigma_i) * x - f(alpha_p * em1) * m[0]
    if order == 1:
        return first
    r0 = (lam[i] - lam[i + 1]) / h
    d10 = (m[0] - m[1]) / f(r0)
    if order == 2:
        return first - f(0.5 * alpha_p * em1) * d10
    r1 = (lam[i + 1] - lam[i + 2]) / h
    d11 = (m[1] - m[2]) / f(r1)
    d1 = d10 + f(r0 / (r0 + r1)) * (d10 - d11)
    d2 = (d10 - d11) / f(r0 + r1)
    return first + f(alpha_p * (em1 / h + 1.0)) * d1 - f(alpha_p * ((em1 + h) / (h * h) - 0.5)) * d2


def dpm_weights(abar, abar_prev):
    """[n, 8] fp64 rows (a, w1_0, w2_0, w2_1, w3_0, w3_1, w3_2, 0): the update is linear, so its weights are its values on
    the unit vectors of (x, m0, m1, m2).  Entries that would need an index >= n, and row 0's higher orders, are 0."""
    n = len(abar)
    rows = np.zeros((n, 8))
    one, zero = np.float64(1.0), np.float64(0.0)
    unit = lambda j: [one if q == j else zero for q in range(3)]   # noqa: E731
    for i in range(n):
        rows[i, 0] = dpm_update(abar, abar_prev, i, 1, one, [zero, zero, zero])
        col = 1
        for order in (1, 2, 3):
            ok = i + order - 1 < n and (i > 0 or order == 1)
            for j in range(order):
                rows[i, col] = dpm_update(abar, abar_prev, i, order, zero, unit(j)) if ok else 0.0
                col += 1
    return rows


def dpm_loop(abar, abar_prev, x_T, denoise, order, first_index=None, xp=np):
    """The whole loop from index first_index (default: the last) down to 0; denoise(x, i) -> x0 prediction at index i."""
    x, hist = x_T, []
    first_index = len(abar) - 1 if first_index is None else first_index
    for k, i in enumerate(range(first_index, -1, -1)):
        hist.insert(0, denoise(x, i))
        del hist[3:]
        x = dpm_update(abar, abar_prev, i, effective_order(order, k, i), x, hist, xp=xp)
    return x


# ---- the analytic case: data N(0, s2 * I), for which the exact denoiser is linear and the probability-flow ODE is solved in
# closed form (the marginal at abar is N(0, abar*s2 + 1 - abar), and the flow scales x by the ratio of standard deviations)
def gaussian_gain(abar, s2):
    """g with E[x0 | x_t] = g * x_t at cumulative alpha abar."""
    return np.sqrt(abar) * s2 / (abar * s2 + 1.0 - abar)


def gaussian_end_point(x_T, abar_T, s2):
    return x_T * np.sqrt(s2) / np.sqrt(abar_T * s2 + 1.0 - abar_T)


def gaussian_error(x, x_T, abar_T, s2):
    """Error of a final sample against the exact end point, relative to the largest exact value."""
    want = gaussian_end_point(np.asarray(x_T, dtype=np.float64), abar_T, s2)
    return float(np.abs(np.asarray(x, dtype=np.float64) - want).max() / np.abs(want).max())
