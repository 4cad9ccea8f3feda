"""CPU restatement of sampling under a guidance interval (include/gdx.h at gdx_set_guidance_interval): the denoiser is the
oracle's forward (oracle/mdm_forward.py), guided -- u + scale * (c - u) -- on the samples whose MODEL timestep lies in [lo, hi] and
the conditional output c itself elsewhere; the loops are the oracle's (oracle/sampler.py) and, for DPM-Solver++, the fp64
recurrence of dpm_restatement.py.  A helper, not a test; it shares no code with the package."""
import numpy as np
import torch

import dpm_restatement as R
from oracle import mdm_forward as omf
from oracle import sampler as osamp
from oracle import schedule as osch


def model_fn(p, cfg, interval):
    """fn(x, mapped_t, y) -> x0 prediction under the interval; y carries 'scale'."""
    lo, hi = interval

    def fn(x, t, y):
        y_c = {k: v for k, v in y.items() if k not in ("scale", "guidance_interval")}
        c = omf.forward(p, cfg, x, t, y_c)
        guided = (t >= lo) & (t <= hi)
        if not bool(guided.any()):
            return c
        u = omf.forward(p, cfg, x, t, dict(y_c, uncond=True))
        blend = u + (y["scale"].view(-1, 1, 1, 1) * (c - u))
        return torch.where(guided.view(-1, 1, 1, 1), blend, c)
    return fn


def sample_loop(p, cfg, interval, schedule, respacing, tape, y, kind, eta=0.0):
    """p_sample_loop / ddim_sample_loop of the oracle on tape [n + 1, B, J, 1, T] (entry 0 = x_T)."""
    tab, tmap = osch.make_tables(schedule, 1000, respacing)
    with torch.no_grad():
        return osamp.sample_loop(model_fn(p, cfg, interval), tab, tmap, tuple(tape[0].shape), tape, y, kind=kind, eta=eta)


def dpm_loop(p, cfg, interval, schedule, tmap, x_T, y, order):
    """DPM-Solver++ multistep in fp64 over the kept timesteps `tmap` (ascending) of the 1000-step `schedule`."""
    abar_full = np.cumprod(1.0 - np.asarray(osch.named_beta_schedule(schedule, 1000), dtype=np.float64))
    ab = abar_full[np.asarray(tmap)]
    abp = np.append(1.0, ab[:-1])
    fn = model_fn(p, cfg, interval)
    B = x_T.shape[0]

    def denoise(x, i):
        with torch.no_grad():
            out = fn(torch.from_numpy(x).float(), torch.full((B,), int(tmap[i]), dtype=torch.long), y)
        return out.double().numpy()
    return R.dpm_loop(ab, abp, x_T.double().numpy(), denoise, order)
