"""Parallel-in-time sampling restated for the tests (not a test module; CPU tensors): the rule of include/gdx.h at
gdx_parallel_loop over the oracle's forward (oracle.mdm_forward) and the oracle's one-step updates (oracle.sampler.p_sample_step /
ddim_step on a noise tape).  It shares no code with the package.

A loop executes steps k = 0 .. K-1 at indices i_k = first - k.  The window holds an anchor a and planes P_0 .. P_W; one iteration
evaluates the denoiser on P_0 .. P_{n-1} (n = min(W, K - a); each plane on its own, at its own timestep), re-runs the update chain
from P_0 with those predictions held fixed, measures each plane's mean squared change in float64, strides past plane 1 and every
further plane whose predecessors all stayed within their thresholds, and slides."""
import numpy as np
import torch

from oracle import mdm_forward as omf
from oracle import sampler as osamp

EVERY_TIMESTEP = (-2**63, 2**63 - 1)


def threshold(tab, tau):
    """threshold[i] = tau^2 * exp(posterior_log_variance_clipped[i]), float64."""
    return float(tau) ** 2 * np.exp(np.asarray(tab.posterior_log_variance_clipped, dtype=np.float64))


def stride_of(err, thr):
    """err: n rows of per-sample errors; thr: the n thresholds of those slots -> 1 + the number of leading rows whose every entry
    is <= its threshold (a NaN is not), capped at n."""
    lead = 0
    for row, t in zip(err, thr):
        if not all(float(e) <= t for e in row):
            break
        lead += 1
    return min(lead + 1, len(err))


def x0_of(p, cfg, x, t_model, y, clip=False, interval=None):
    """The blended x0 prediction of one plane at one model timestep: guided inside the interval (the conditional pass alone
    outside it), then the inpainting blend and the clamp, as p_mean_variance forms it."""
    lo, hi = interval if interval is not None else EVERY_TIMESTEP
    guided = "scale" in y and lo <= int(t_model[0]) <= hi
    y_c = {k: v for k, v in y.items() if k != "scale"}
    out = omf.cfg_forward(p, cfg, x, t_model, y) if guided else omf.forward(p, cfg, x, t_model, y_c)
    return osamp.process_xstart(osamp.inpaint(out, y), clip)


def parallel_loop(p, cfg, tab, tmap, tape, y, kind, window, tau, eta=0.0, clip=False, interval=None, max_iterations=None):
    """tape [K + 1, B, J, 1, T] (entry 0 = x_T, entry 1 + k = the noise of executed step k) -> (sample, strides)."""
    K = tab.num_timesteps
    B, per = tape[0].shape[0], tape[0][0].numel()
    thr = threshold(tab, tau)
    mapt = torch.tensor(tmap, dtype=torch.long)
    step = (lambda x0, v, t, z: osamp.p_sample_step(tab, x0, v, t, z)) if kind == "p" else \
           (lambda x0, v, t, z: osamp.ddim_step(tab, x0, v, t, z, eta))
    planes = [tape[0].clone() for _ in range(window + 1)]
    a, strides = 0, []
    with torch.no_grad():
        while a < K and (max_iterations is None or len(strides) < max_iterations):
            n = min(window, K - a)
            idx = [K - 1 - (a + j) for j in range(n)]
            ts = [torch.full((B,), i, dtype=torch.long) for i in idx]
            M = [x0_of(p, cfg, planes[j], mapt[ts[j]], y, clip, interval) for j in range(n)]
            v, err = planes[0], []
            for j in range(n):
                v = step(M[j], v, ts[j], tape[1 + a + j])
                err.append((((v.double() - planes[j + 1].double()) ** 2).reshape(B, -1).sum(1) / per).tolist())
                planes[j + 1] = v
            s = stride_of(err, [thr[i] for i in idx])
            planes = [planes[min(j + s, window)] for j in range(window + 1)]
            a += s
            strides.append(s)
    return planes[0], strides
