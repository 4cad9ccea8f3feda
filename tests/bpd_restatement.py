"""fp64 restatement of the variational bound, written from the maths (Ho et al. 2020, eq. 5-7 and the discretised decoder
of section 3.3; Nichol & Dhariwal 2021 for the variance choices), plus the tolerance rule the bound's tests share.

    q(x_t | x_0)        = N(sqrt(abar_t) x_0, (1 - abar_t) I)
    q(x_{t-1}|x_t,x_0)  = N(c1_t x_0 + c2_t x_t, btilde_t I)
    p(x_{t-1}|x_t)      = N(c1_t x0_hat + c2_t x_t, sigma_t^2 I)           (x0-predicting model, fixed variance)
    L_t   = KL(q || p) = 0.5 (log sigma^2 - log btilde - 1 + btilde / sigma^2 + (mu_q - mu_p)^2 / sigma^2)
    L_0   = -log integral over the 2/255 bin around x_0 of p(x_0 | x_1), open-ended bins beyond +-0.999, with the Gaussian cdf
            approximated by 0.5 (1 + tanh(sqrt(2 / pi) (u + 0.044715 u^3))) and probabilities floored at 1e-12
    L_T   = KL(q(x_T | x_0) || N(0, I))
all averaged over the elements of a sample and divided by ln 2.  The schedule tables enter rounded to fp32 once (that is how
the library and the reference hand them to the arithmetic); everything else is fp64.
"""
import numpy as np

FWD_TOL = 2e-5       # tests/test_gpu_parity.py: per-step quantities, relative to max|reference|
LOOP_TOL = 2e-4      # tests/test_gpu_parity.py: whole-loop quantities
OUTS = ("total_bpd", "prior_bpd", "vb", "xstart_mse", "mse")
LN2 = np.log(2.0)


def tables(betas, var_type="FIXED_SMALL"):
    betas = np.asarray(betas, dtype=np.float64)
    abar = np.cumprod(1.0 - betas)
    abar_prev = np.append(1.0, abar[:-1])
    btilde = betas * (1.0 - abar_prev) / (1.0 - abar)
    log_btilde = np.log(np.append(btilde[1], btilde[1:]))
    log_sigma2 = log_btilde if var_type == "FIXED_SMALL" else np.log(np.append(btilde[1], betas[1:]))
    r = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)   # noqa: E731
    return dict(c1=r(betas * np.sqrt(abar_prev) / (1.0 - abar)), c2=r((1.0 - abar_prev) * np.sqrt(1.0 - betas) / (1.0 - abar)),
                log_btilde=r(log_btilde), log_sigma2=r(log_sigma2), sqrt_abar=r(np.sqrt(abar)),
                sqrt_1m_abar=r(np.sqrt(1.0 - abar)), sqrt_recip=r(np.sqrt(1.0 / abar)), sqrt_recipm1=r(np.sqrt(1.0 / abar - 1.0)),
                log_1m_abar=r(np.log(1.0 - abar)), n=len(betas))


def respaced_betas(base_betas, timestep_map):
    abar = np.cumprod(1.0 - np.asarray(base_betas, dtype=np.float64))[list(timestep_map)]
    return 1.0 - abar / np.concatenate(([1.0], abar[:-1]))


def _cdf(u):
    return 0.5 * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (u + 0.044715 * u ** 3)))


def step_terms(tab, t, x0, x_t, z, pred, model_mean=None):
    """Per-sample (vb, xstart_mse, mse) at per-sample steps t [B] from the (already blended / clamped) x0 prediction."""
    x0, x_t, z, pred = (np.asarray(a, dtype=np.float64) for a in (x0, x_t, z, pred))
    t = np.asarray(t).reshape(-1)
    e = lambda a: a[t].reshape(-1, *([1] * (x0.ndim - 1)))   # noqa: E731
    mu_q = e(tab["c1"]) * x0 + e(tab["c2"]) * x_t
    mu_p = e(tab["c1"]) * pred + e(tab["c2"]) * x_t if model_mean is None else np.asarray(model_mean, dtype=np.float64)
    lq, lp = e(tab["log_btilde"]), e(tab["log_sigma2"])
    kl = 0.5 * (lp - lq - 1.0 + np.exp(lq - lp) + (mu_q - mu_p) ** 2 * np.exp(-lp))
    inv_std = np.exp(-0.5 * lp)
    upper, lower = _cdf(inv_std * (x0 - mu_p + 1.0 / 255.0)), _cdf(inv_std * (x0 - mu_p - 1.0 / 255.0))
    prob = np.where(x0 < -0.999, upper, np.where(x0 > 0.999, 1.0 - lower, upper - lower))
    nll = -np.log(np.maximum(prob, 1e-12))
    flat = lambda a: a.reshape(a.shape[0], -1).mean(axis=1)   # noqa: E731
    vb = np.where(t == 0, flat(nll), flat(kl)) / LN2
    eps = (e(tab["sqrt_recip"]) * x_t - pred) / e(tab["sqrt_recipm1"])
    return vb, flat((pred - x0) ** 2), flat((eps - z) ** 2)


def prior_term(tab, x0):
    x0 = np.asarray(x0, dtype=np.float64)
    # The data-free part -1 - lv + exp(lv) (~ lv^2 / 2, a cancellation) is a function of the fp32 table entry alone and is
    # evaluated in fp32 by the reference in BOTH its runs and by the library, so the fixture's fp32-vs-fp64 deviation does
    # not contain its rounding error (up to an ulp of 1, i.e. percents of a 1e-5 prior): it enters here as that fp32 scalar.
    lv = np.float32(tab["log_1m_abar"][-1])
    s = np.float64((np.float32(-1.0) - lv) + np.exp(lv))
    kl = 0.5 * (s + (tab["sqrt_abar"][-1] * x0) ** 2)
    return kl.reshape(kl.shape[0], -1).mean(axis=1) / LN2


def q_sample(tab, t, x0, z):
    return tab["sqrt_abar"][t] * np.asarray(x0, dtype=np.float64) + tab["sqrt_1m_abar"][t] * np.asarray(z, dtype=np.float64)


def blend(out, out_uncond=None, scale=None, mask=None, motion=None, clip=False):
    p = np.asarray(out, dtype=np.float64)
    if out_uncond is not None:
        u = np.asarray(out_uncond, dtype=np.float64)
        p = u + np.asarray(scale, dtype=np.float64).reshape(-1, *([1] * (p.ndim - 1))) * (p - u)
    if mask is not None:
        p = np.where(mask, np.asarray(motion, dtype=np.float64), p)
    return np.clip(p, -1.0, 1.0) if clip else p


def loop(tab, x0, tape, predict, mean_type="START_X"):
    """The whole bound: predict(x_t, i) -> the denoiser's (blended / clamped) reading at respaced index i."""
    n, B = tab["n"], x0.shape[0]
    vb, xm, em = (np.empty((B, n)) for _ in range(3))
    for k in range(n):
        i = n - 1 - k
        x_t = q_sample(tab, i, x0, tape[k])
        vb[:, k], xm[:, k], em[:, k] = step_terms(tab, np.full(B, i), x0, x_t, tape[k], predict(x_t, i))
    prior = prior_term(tab, x0)
    return {"total_bpd": vb.sum(axis=1) + prior, "prior_bpd": prior, "vb": vb, "xstart_mse": xm, "mse": em}


def worst_ratios(got, g, case, against="fp32"):
    """Error of `got` over its allowance for each of the five outputs of fixture case `case`, measured against the
    reference's fp32 run (what an fp32 implementation is held to) or its fp64 run (what the fp64 restatement is held to).  xstart_mse / mse: FWD_TOL,
    total_bpd: LOOP_TOL, each relative to max|fixture|.  vb and prior_bpd are ill-conditioned, so each entry is allowed 10 x the
    reference's own |fp32 - fp64| deviation at that entry, floored at FWD_TOL * max|fixture|."""
    out = {}
    for k in OUTS:
        ref32 = np.asarray(g[f"{case}.{k}"], dtype=np.float64)
        ref64 = np.asarray(g[f"{case}.{k}_fp64"], dtype=np.float64)
        v = np.asarray(got[k], dtype=np.float64)
        assert v.shape == ref32.shape, (case, k, v.shape, ref32.shape)
        top = np.abs(ref32).max()
        want = ref32 if against == "fp32" else ref64
        if k in ("vb", "prior_bpd"):
            allow = np.maximum(10.0 * np.abs(ref32 - ref64), FWD_TOL * top)
        else:
            allow = np.full(ref32.shape, (LOOP_TOL if k == "total_bpd" else FWD_TOL) * top)
        out[k] = float((np.abs(v - want) / allow).max())
    return out


def assert_case(got, g, case, label="", against="fp32"):
    r = worst_ratios(got, g, case, against)
    print(f"bpd-ratio {label} {case} " + " ".join(f"{k}={v:.3g}" for k, v in r.items()))
    assert all(np.isfinite(v) and v <= 1.0 for v in r.values()), (label, case, r)
    return r
