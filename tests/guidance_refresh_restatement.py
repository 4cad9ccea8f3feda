"""CPU restatement of sampling under the guidance refresh (include/gdx.h at gdx_set_guidance_refresh): the denoiser is the
oracle's forward (oracle/mdm_forward.py); the guided calls of a loop are counted n = 0, 1, ... in execution order, call n
computes the unconditional pass and keeps d = c - u when n % every == 0, and every other guided call blends with u' = c - d.
Calls outside the guidance interval return the conditional output and are not counted.  The loops are the oracle's
(oracle/sampler.py) and, for DPM-Solver++, the fp64 recurrence of dpm_restatement.py.  A helper, not a test; it shares no code
with the package."""
import numpy as np
import torch

import dpm_restatement as R
from oracle import mdm_forward as omf
from oracle import sampler as osamp
from oracle import schedule as osch

EVERY_TIMESTEP = (-2**63, 2**63 - 1)


class RefreshModel:
    """fn(x, mapped_t, y) -> x0 prediction of one loop (a fresh instance per loop: the counter and the difference are its
    state).  every = None: the unguided loop (the conditional output everywhere).  `calls` records what each call did."""

    def __init__(self, p, cfg, every, interval=None):
        self.p, self.cfg, self.every = p, cfg, every
        self.lo, self.hi = interval if interval is not None else EVERY_TIMESTEP
        self.n, self.d, self.calls = 0, None, []

    def __call__(self, x, t, y):
        y_c = {k: v for k, v in y.items() if k not in ("scale", "guidance_interval", "guidance_refresh")}
        c = omf.forward(self.p, self.cfg, x, t, y_c)
        ts = set(t.tolist())
        assert len(ts) == 1, "a loop calls the denoiser with one timestep for the batch"
        tau = ts.pop()
        if self.every is None or not self.lo <= tau <= self.hi:
            self.calls.append("off")
            return c
        if self.n % self.every == 0:
            u = omf.forward(self.p, self.cfg, x, t, dict(y_c, uncond=True))
            self.d = c - u
            self.calls.append("refresh")
        else:
            u = c - self.d
            self.calls.append("reuse")
        self.n += 1
        return u + (y["scale"].view(-1, 1, 1, 1) * (c - u))


def sample_loop(p, cfg, every, schedule, respacing, tape, y, kind, eta=0.0, interval=None):
    """p_sample_loop / ddim_sample_loop of the oracle on tape [n + 1, B, J, 1, T] (entry 0 = x_T) -> (sample, calls)."""
    tab, tmap = osch.make_tables(schedule, 1000, respacing)
    fn = RefreshModel(p, cfg, every, interval)
    with torch.no_grad():
        out = osamp.sample_loop(fn, tab, tmap, tuple(tape[0].shape), tape, y, kind=kind, eta=eta)
    return out, fn.calls


def dpm_loop(p, cfg, every, schedule, tmap, x_T, y, order, interval=None):
    """DPM-Solver++ multistep in fp64 over the kept timesteps `tmap` (ascending) of the 1000-step `schedule` -> (sample, calls)."""
    abar_full = np.cumprod(1.0 - np.asarray(osch.named_beta_schedule(schedule, 1000), dtype=np.float64))
    ab = abar_full[np.asarray(tmap)]
    abp = np.append(1.0, ab[:-1])
    fn = RefreshModel(p, cfg, every, interval)
    B = x_T.shape[0]

    def denoise(x, i):
        with torch.no_grad():
            out = fn(torch.from_numpy(x).float(), torch.full((B,), int(tmap[i]), dtype=torch.long), y)
        return out.double().numpy()
    return R.dpm_loop(ab, abp, x_T.double().numpy(), denoise, order), fn.calls


def plan(flags, every, plms=False, skip_timesteps=0):
    """The rule on the host, from per-index guidance flags: "off" | "refresh" | "reuse" per denoiser call in execution order."""
    n_t = len(flags)
    calls = list(range(n_t - skip_timesteps))[::-1]
    if plms and calls:
        calls.insert(1, (calls[0] - 1) % n_t)
    out, n = [], 0
    for i in calls:
        if not flags[i]:
            out.append("off")
        else:
            out.append("refresh" if n % every == 0 else "reuse")
            n += 1
    return out
