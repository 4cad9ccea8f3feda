"""CPU restatement of the guidance rescale (include/gdx.h at gdx_set_guidance_rescale; Lin et al. 2023, arXiv:2305.08891, section
3.4): the guided blend g = u + s * (c - u) in fp32 torch, the per-sample sums of c, c^2, g, g^2 in fp64 numpy, the factor
f = phi * sqrt(SS_c / SS_g) + (1 - phi) rounded once to fp32, g * f in fp32; an unguided sample keeps c.  The denoiser is the
oracle's forward (oracle/mdm_forward.py); the loops are the oracle's (oracle/sampler.py) and, for DPM-Solver++, the fp64 recurrence
of dpm_restatement.py.  A helper, not a test; it shares no code with the package."""
import numpy as np
import torch

import dpm_restatement as R
from oracle import mdm_forward as omf
from oracle import sampler as osamp
from oracle import schedule as osch


def blend(c, u, scale):
    """u + s * (c - u), every operation its own fp32 rounding (torch runs them as separate kernels)."""
    return u + (scale.view(-1, 1, 1, 1) * (c - u))


def factor_of(c, g, phi):
    """[B] fp32 factors of fp32 tensors c, g [B, ...]; phi is the float the C ABI carries, widened to fp64."""
    B = c.shape[0]
    c64 = c.reshape(B, -1).double().numpy()
    g64 = g.reshape(B, -1).double().numpy()
    n = c64.shape[1]
    phi = np.float64(np.float32(phi))
    f = np.empty(B, dtype=np.float32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for b in range(B):
            ss = []
            for v in (c64[b], g64[b]):
                s, q = v.sum(), (v * v).sum()
                d = q - s * s / n
                ss.append(np.float64(0.0) if d < 0 else d)        # a NaN stays a NaN
            r = np.float64(1.0) if ss[1] == 0 else np.sqrt(ss[0] / ss[1])
            f[b] = np.float32(phi * r + (np.float64(1.0) - phi))
    return torch.from_numpy(f)


def rescale(c, u, scale, phi, guided=None):
    """(out, factor) of CPU fp32 tensors c, u [B,J,1,T] and scale [B]; guided: bool [B] (None = every sample)."""
    g = blend(c, u, scale)
    f = factor_of(c, g, phi)
    out = g * f.view(-1, 1, 1, 1)
    if guided is not None:
        f = torch.where(guided, f, torch.ones_like(f))
        out = torch.where(guided.view(-1, 1, 1, 1), out, c)
    return out, f


def model_fn(p, cfg, phi, interval=None):
    """fn(x, mapped_t, y) -> rescaled x0 prediction (under the interval, if one is given); y carries 'scale'.  fn.factors
    collects the factor of every guided sample it computed."""
    factors = []

    def fn(x, t, y):
        y_c = {k: v for k, v in y.items() if k not in ("scale", "guidance_interval", "guidance_rescale")}
        c = omf.forward(p, cfg, x, t, y_c)
        guided = torch.ones_like(t, dtype=torch.bool) if interval is None else (t >= interval[0]) & (t <= interval[1])
        if not bool(guided.any()):
            return c
        u = omf.forward(p, cfg, x, t, dict(y_c, uncond=True))
        out, f = rescale(c, u, y["scale"], phi, guided)
        factors.extend(float(v) for v in f[guided])
        return out
    fn.factors = factors
    return fn


def sample_loop(p, cfg, phi, interval, schedule, respacing, tape, y, kind, eta=0.0):
    """p_sample_loop / ddim_sample_loop of the oracle on tape [n + 1, B, J, 1, T] (entry 0 = x_T) -> (sample, factors)."""
    tab, tmap = osch.make_tables(schedule, 1000, respacing)
    fn = model_fn(p, cfg, phi, interval)
    with torch.no_grad():
        out = osamp.sample_loop(fn, tab, tmap, tuple(tape[0].shape), tape, y, kind=kind, eta=eta)
    return out, fn.factors


def dpm_loop(p, cfg, phi, interval, schedule, tmap, x_T, y, order):
    """DPM-Solver++ multistep in fp64 over the kept timesteps `tmap` (ascending) of the 1000-step `schedule` -> (sample, factors)."""
    abar_full = np.cumprod(1.0 - np.asarray(osch.named_beta_schedule(schedule, 1000), dtype=np.float64))
    ab = abar_full[np.asarray(tmap)]
    abp = np.append(1.0, ab[:-1])
    fn = model_fn(p, cfg, phi, interval)
    B = x_T.shape[0]

    def denoise(x, i):
        with torch.no_grad():
            out = fn(torch.from_numpy(x).float(), torch.full((B,), int(tmap[i]), dtype=torch.long), y)
        return out.double().numpy()
    return torch.from_numpy(R.dpm_loop(ab, abp, x_T.double().numpy(), denoise, order)), fn.factors
