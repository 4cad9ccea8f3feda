"""CPU restatement of sampling under the layer cache (include/gdx.h at gdx_set_layer_cache): the denoiser is the oracle's forward
with its per-layer taps (oracle/mdm_forward.py).  ALL denoiser calls of a loop are counted m = 0, 1, ... in execution order; a
full call runs every layer and keeps delta = out - in, `in` the residual stream after layer keep - 1 without token 0 and `out`
the last layer's output without token 0; a partial call takes its own `in'` and feeds in' + delta to the output layer.  A call is
full when m % every == 0 or the stored mode does not cover its own.  Guidance (interval, refresh) is restated as in
guidance_refresh_restatement.py, whose loops this module reuses.  A helper, not a test; it shares no code with the package."""
import torch
import torch.nn.functional as F

import guidance_refresh_restatement as FR
from oracle import mdm_forward as omf

COND, UNCOND, CFG = "cond", "uncond", "cfg"


def covers(stored, mode):
    return stored == mode or (stored == CFG and mode == COND)


def plan(modes, every):
    """modes: the forward mode of every denoiser call in execution order -> "full" | "partial" per call."""
    out, stored = [], None
    for m, c in enumerate(modes):
        full = m % every == 0 or not covers(stored, c)
        if full:
            stored = c
        out.append("full" if full else "partial")
    return out


def modes_of(flags, refresh=1, guided=True, plms=False, skip_timesteps=0, mode=COND):
    """The forward mode of every call of a loop over per-index guidance flags: a guided loop's refresh calls run as CFG, its
    reuse calls and the calls outside the interval as COND; an unguided loop runs every call in `mode`."""
    calls = FR.plan(flags if guided else [False] * len(flags), refresh, plms=plms, skip_timesteps=skip_timesteps)
    return [CFG if c == "refresh" else COND if guided else mode for c in calls]


class CachedModel:
    """fn(x, mapped_t, y) -> x0 prediction of one loop (a fresh instance per loop: the counters, the stored change and the
    stored guidance difference are its state).  every = 1: the uncached loop.  guided False: the conditional model alone."""

    def __init__(self, p, cfg, every, keep, guided=True, interval=None, refresh=1):
        self.p, self.cfg, self.every, self.keep, self.guided, self.refresh = p, cfg, every, keep, guided, refresh
        self.lo, self.hi = interval if interval is not None else FR.EVERY_TIMESTEP
        self.m, self.n, self.stored, self.delta, self.d = 0, 0, None, {}, None
        self.calls, self.layers = [], 0

    def _pass(self, x, t, y, row, full):
        """One pass of the denoiser over the batch (row: the delta slot, "c" or "u")."""
        L = self.cfg["num_layers"]
        taps = {}
        out = omf.forward(self.p, self.cfg, x, t, y, taps)
        self.layers += x.shape[0] * (L if full else self.keep)
        if self.every == 1:
            return out
        inner = taps[f"seqTransEncoder.layers.{self.keep - 1}.out"][1:]          # [T, B, d]
        if full:
            self.delta[row] = taps[f"seqTransEncoder.layers.{L - 1}.out"][1:] - inner
            return out
        T, B, _ = inner.shape
        x0 = F.linear(inner + self.delta[row], self.p["output_process.poseFinal.weight"], self.p["output_process.poseFinal.bias"])
        return x0.reshape(T, B, x.shape[1], x.shape[2]).permute(1, 2, 3, 0)

    def __call__(self, x, t, y):
        y_c = {k: v for k, v in y.items() if k not in ("scale", "guidance_interval", "guidance_refresh", "layer_cache")}
        ts = set(t.tolist())
        assert len(ts) == 1, "a loop calls the denoiser with one timestep for the batch"
        tau = ts.pop()
        is_guided = self.guided and self.lo <= tau <= self.hi
        refreshes = is_guided and self.n % self.refresh == 0
        mode = CFG if refreshes else UNCOND if (not self.guided and y_c.get("uncond")) else COND
        full = self.m % self.every == 0 or not covers(self.stored, mode)
        if full:
            self.stored = mode
        self.m += 1
        self.calls.append("full" if full else "partial")
        c = self._pass(x, t, y_c, "u" if mode == UNCOND else "c", full)
        if not is_guided:
            return c
        if refreshes:
            u = self._pass(x, t, dict(y_c, uncond=True), "u", full)
            self.d = c - u
        else:
            u = c - self.d
        self.n += 1
        return u + (y["scale"].view(-1, 1, 1, 1) * (c - u))


def sample_loop(p, cfg, every, keep, schedule, respacing, tape, y, kind, eta=0.0, **model_kw):
    """p_sample_loop / ddim_sample_loop of the oracle on tape [n + 1, B, J, 1, T] (entry 0 = x_T) -> (sample, model)."""
    from oracle import sampler as osamp
    from oracle import schedule as osch
    tab, tmap = osch.make_tables(schedule, 1000, respacing)
    fn = CachedModel(p, cfg, every, keep, **model_kw)
    with torch.no_grad():
        out = osamp.sample_loop(fn, tab, tmap, tuple(tape[0].shape), tape, y, kind=kind, eta=eta)
    return out, fn


def dpm_loop(p, cfg, every, keep, schedule, tmap, x_T, y, order, **model_kw):
    """DPM-Solver++ multistep in fp64 over the kept timesteps `tmap` of the 1000-step `schedule` -> (sample, model)."""
    import numpy as np

    import dpm_restatement as R
    from oracle import schedule as osch
    abar_full = np.cumprod(1.0 - np.asarray(osch.named_beta_schedule(schedule, 1000), dtype=np.float64))
    ab = abar_full[np.asarray(tmap)]
    abp = np.append(1.0, ab[:-1])
    fn = CachedModel(p, cfg, every, keep, **model_kw)
    B = x_T.shape[0]

    def denoise(x, i):
        with torch.no_grad():
            out = fn(torch.from_numpy(x).float(), torch.full((B,), int(tmap[i]), dtype=torch.long), y)
        return out.double().numpy()
    return torch.from_numpy(R.dpm_loop(ab, abp, x_T.double().numpy(), denoise, order)), fn
