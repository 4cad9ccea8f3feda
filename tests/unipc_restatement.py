"""fp64 numpy restatement of the UniPC sampler (include/gdx.h at gdx_unipc_step / gdx_unipc_loop), written from the recurrences
in their D form (Zhao et al. 2023, arXiv:2302.04867, data prediction with B(h) = expm1(-h)) and numpy.linalg.solve -- never from
collected weights.  A helper, not a test; it shares no code with the package.  The analytic Gaussian case is dpm_restatement's."""
import numpy as np


def lam_of(abar):
    return 0.5 * np.log(abar / (1.0 - abar))


def unipc_update(abar, abar_prev, b, q, x, m, m_new=None, xp=np):
    """One step of order q with base index b on the state x: m = x0 predictions, newest first (m[0] of index b, m[1] of b + 1,
    ...).  m_new None: the predictor UniP-q -> the state at b's target.  m_new given (the prediction made at b's target): the
    corrector UniC-q -> the corrected state there.  xp: the array module of x / m (numpy, or torch for the fp32 restatement; the
    scalar coefficients stay Python floats)."""
    if abar_prev[b] == 1.0:                                   # the step to sigma = 0: h = inf, x' = m_b
        assert q == 1 and m_new is None
        return m[0] + 0.0 * x
    lam = lam_of(abar)
    alpha_p, sigma_p, sigma_b = np.sqrt(abar_prev[b]), np.sqrt(1.0 - abar_prev[b]), np.sqrt(1.0 - abar[b])
    h = 0.5 * np.log(abar_prev[b] / (1.0 - abar_prev[b])) - lam[b]
    big_e = np.expm1(-h)
    big_b = big_e                                             # the bh2 variant
    f = float if xp is not np else (lambda v: v)
    first = f(sigma_p / sigma_b) * x - f(alpha_p * big_e) * m[0]
    r = [(lam[b + j] - lam[b]) / h for j in range(1, q)]
    d = [(m[j] - m[0]) / f(r[j - 1]) for j in range(1, q)]
    hh = -h
    g, fact, beta = np.expm1(hh) / hh - 1.0, 1.0, []
    for n in range(1, q + 1):
        beta.append(g * fact / big_b)
        fact *= n + 1
        g = g / hh - 1.0 / fact
    vander = lambda rs: np.array([[v ** p for v in rs] for p in range(len(rs))])   # noqa: E731  R[n][j] = r_j^(n-1)
    if m_new is None:
        if q == 1:
            return first
        rho = [0.5] if q == 2 else np.linalg.solve(vander(r), np.array(beta[:q - 1]))
        res = sum(f(rho[j]) * d[j] for j in range(q - 1))
    else:
        rho = [0.5] if q == 1 else np.linalg.solve(vander(r + [1.0]), np.array(beta))
        res = f(rho[q - 1]) * (m_new - m[0])
        for j in range(q - 1):
            res = res + f(rho[j]) * d[j]
    return first - f(alpha_p * big_b) * res


def unipc_weights(abar, abar_prev):
    """(pred [n, 8], corr [n, 16]) fp64 rows in the layout of gdx_unipc_step: both updates are linear, so their weights are
    their values on the unit vectors of (x, m_new, m_b, m_{b+1}, m_{b+2}).  Entries that would need an index >= n, and row 0's
    beyond (0, 1, 0, ...), are 0."""
    n = len(abar)
    pred, corr = np.zeros((n, 8)), np.zeros((n, 16))
    one, zero = np.float64(1.0), np.float64(0.0)
    unit = lambda j, cnt=3: [one if q == j else zero for q in range(cnt)]   # noqa: E731
    for b in range(n):
        pred[b, 0] = unipc_update(abar, abar_prev, b, 1, one, unit(-1))
        col = 1
        for q in (1, 2, 3):
            ok = b + q - 1 < n and (b > 0 or q == 1)
            for j in range(q):
                pred[b, col] = unipc_update(abar, abar_prev, b, q, zero, unit(j)) if ok else 0.0
                col += 1
            if ok and b > 0:
                corr[b, 4 * (q - 1)] = unipc_update(abar, abar_prev, b, q, zero, unit(-1), m_new=one)
                for j in range(q):
                    corr[b, 4 * (q - 1) + 1 + j] = unipc_update(abar, abar_prev, b, q, zero, unit(j), m_new=zero)
    return pred, corr


def effective_orders(order, k, i):
    """(corrector, predictor) order of executed step k of a loop, at index i; corrector 0 = none."""
    return (0 if k == 0 or i == 0 else min(order, k)), min(order, k + 1, i + 1)


def unipc_loop(abar, abar_prev, x_T, denoise, order, first_index=None, xp=np, corrector=True):
    """The whole loop from index first_index (default: the last) down to 0; denoise(x, i) -> x0 prediction at index i.
    corrector=False leaves the predictor alone (UniP: DDIM / 2M at orders 1 / 2)."""
    x, base, hist = x_T, None, []
    first_index = len(abar) - 1 if first_index is None else first_index
    for k, i in enumerate(range(first_index, -1, -1)):
        m_i = denoise(x, i)
        qc, qp = effective_orders(order, k, i)
        base = unipc_update(abar, abar_prev, i + 1, qc, base, hist, m_new=m_i, xp=xp) if qc and corrector else x
        hist.insert(0, m_i)
        del hist[3:]
        x = unipc_update(abar, abar_prev, i, qp, base, hist, xp=xp)
    return x
