"""RePaint resampling restated for the tests (not a test module; CPU only): the rule of include/gdx.h at gdx_set_resample, written
the way RePaint's own get_schedule_jump writes it (a list of times, one entry per single step), over the oracle's forward
(oracle.mdm_forward) and the oracle's one-step updates (oracle.sampler.p_sample_step / ddim_step on a noise tape), and the analytic
two-dimensional case of DESIGN.md 4p in float64.  It shares no code with the package.

Levels: level L is the input of the reverse step at schedule index L - 1, level 0 the sample, a loop starts at level N."""
import numpy as np
import torch

import guidance_rescale_restatement as GR
from oracle import mdm_forward as omf
from oracle import sampler as osamp
from oracle import schedule as osch

EVERY_TIMESTEP = (-2**63, 2**63 - 1)


def level_sequence(N, jump, repeats):
    """RePaint's schedule (get_schedule_jump with one jump length, range(0, t_T - jump, jump)) as the levels the state visits,
    N first: down one level at a time, and at a jump level with jumps left `jump` single levels up again."""
    left = {level: repeats - 1 for level in range(0, N - jump, jump)}
    t, seq = N, [N]
    while t >= 1:
        t -= 1
        seq.append(t)
        if left.get(t, 0) > 0:
            left[t] -= 1
            for _ in range(jump):
                t += 1
                seq.append(t)
    return seq


def hops(N, jump, repeats):
    """The sequence as hops: ("r", index) for one level down (the reverse step at index = the level reached), ("f", from, to) for a
    whole ascending run taken in one hop."""
    seq, out, i = level_sequence(N, jump, repeats), [], 1
    while i < len(seq):
        if seq[i] < seq[i - 1]:
            out.append(("r", seq[i]))
            i += 1
        else:
            j = i
            while j + 1 < len(seq) and seq[j + 1] > seq[j]:
                j += 1
            out.append(("f", seq[i - 1], seq[j]))
            i = j + 1
    return out


def calls(N, jump, repeats):
    """Denoiser calls = N + n_levels * (repeats - 1) * jump, n_levels = the jump levels 0, jump, ... with level + jump < N."""
    return N + len(range(0, N - jump, jump)) * (repeats - 1) * jump


def coef(alphas_cumprod, frm, to):
    """(a, b) of the forward hop frm -> to: float64 sqrt(r), sqrt(1 - r), r = abar_lvl[to] / abar_lvl[frm], abar_lvl = [1, abar ...],
    each rounded to float32 once."""
    lvl = np.concatenate(([1.0], np.asarray(alphas_cumprod, dtype=np.float64)))
    r = lvl[to] / lvl[frm]
    return np.float32(np.sqrt(r)), np.float32(np.sqrt(1.0 - r))


def x0_of(p, cfg, x, t_model, y, clip=False, interval=None, rescale=0.0):
    """The x0 prediction of one reverse hop at one model timestep: guided inside the interval (under rescale > 0 by the rule of
    gdx_cfg_rescale, guidance_rescale_restatement.py), the conditional pass alone outside it; then the inpainting blend and the
    clamp, as p_mean_variance forms it."""
    lo, hi = interval if interval is not None else EVERY_TIMESTEP
    guided = "scale" in y and lo <= int(t_model[0]) <= hi
    y_c = {k: v for k, v in y.items() if k != "scale"}
    if guided and rescale > 0:
        out = GR.model_fn(p, cfg, rescale, interval)(x, t_model, y)
    else:
        out = omf.cfg_forward(p, cfg, x, t_model, y) if guided else omf.forward(p, cfg, x, t_model, y_c)
    return osamp.process_xstart(osamp.inpaint(out, y), clip)


def repaint_loop(p, cfg, tab, tmap, tape, y, kind, jump, repeats, eta=0.0, clip=False, interval=None, skip_timesteps=0,
                 init_image=None, rescale=0.0):
    """tape [1 + hops, B, J, 1, T] (entry 0 = x_T, entry 1 + k = the noise of executed hop k, reverse or forward) -> sample."""
    N = tab.num_timesteps - skip_timesteps
    plan = hops(N, jump, repeats)
    assert len(tape) == 1 + len(plan)
    B = tape[0].shape[0]
    mapt = torch.tensor(tmap, dtype=torch.long)
    img = tape[0]
    if skip_timesteps and init_image is None:
        init_image = torch.zeros_like(img)
    if init_image is not None:
        img = osamp.q_sample(tab, init_image, torch.full((B,), N - 1, dtype=torch.long), img)
    with torch.no_grad():
        for k, hop in enumerate(plan):
            z = tape[1 + k]
            if hop[0] == "f":
                a, b = coef(tab.alphas_cumprod, hop[1], hop[2])
                img = torch.tensor(a) * img + torch.tensor(b) * z
                continue
            t = torch.full((B,), hop[1], dtype=torch.long)
            x0 = x0_of(p, cfg, img, mapt[t], y, clip, interval, rescale)
            img = osamp.p_sample_step(tab, x0, img, t, z) if kind == "p" else osamp.ddim_step(tab, x0, img, t, z, eta)
    return img


# --------------------------------------------------------------------------------------------------------- the analytic case
RHO, KNOWN = 0.9, 1.5            # prior N(0, [[1, rho], [rho, 1]]); dimension 0 is inpainted to KNOWN
TRUE_MEAN, TRUE_VAR = RHO * KNOWN, 1.0 - RHO * RHO      # of dimension 1 given dimension 0: 1.35, 0.19


def analytic(kind, jump, repeats, samples=20000, seed=0, respacing="50"):
    """float64: the exact linear denoiser E[x0 | x_t] = sqrt(abar) Sigma (abar Sigma + (1 - abar) I)^-1 x_t of the Gaussian prior on a
    cosine schedule of 1000 steps strided to `respacing`, dimension 0 of every prediction replaced by KNOWN (the reference's
    inpainting), ancestral ("p", FIXED_SMALL) or DDIM eta = 0 ("ddim") reverse hops and forward hops x <- a x + b z between levels
    -> (mean, variance) of dimension 1 over `samples` chains."""
    tab, _ = osch.make_tables("cosine", 1000, respacing)
    abar = np.asarray(tab.alphas_cumprod, dtype=np.float64)
    lvl = np.concatenate(([1.0], abar))
    N = len(abar)
    sigma = np.array([[1.0, RHO], [RHO, 1.0]])
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((samples, 2))
    for hop in hops(N, jump, repeats):
        if hop[0] == "f":
            r = lvl[hop[2]] / lvl[hop[1]]
            x = np.sqrt(r) * x + np.sqrt(1.0 - r) * rng.standard_normal(x.shape)
            continue
        i = hop[1]
        gain = np.sqrt(abar[i]) * sigma @ np.linalg.inv(abar[i] * sigma + (1.0 - abar[i]) * np.eye(2))
        x0 = x @ gain.T
        x0[:, 0] = KNOWN
        if kind == "p":
            mean = tab.posterior_mean_coef1[i] * x0 + tab.posterior_mean_coef2[i] * x
            noise = rng.standard_normal(x.shape) if i > 0 else 0.0
            x = mean + np.exp(0.5 * tab.posterior_log_variance_clipped[i]) * noise
        else:
            eps = (x - np.sqrt(abar[i]) * x0) / np.sqrt(1.0 - abar[i])
            x = np.sqrt(lvl[i]) * x0 + np.sqrt(1.0 - lvl[i]) * eps
    return float(x[:, 1].mean()), float(x[:, 1].var())
