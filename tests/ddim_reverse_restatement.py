"""DDIM inversion restated for the tests (not a test module; CPU or GPU tensors alike).

Two restatements of ddim_reverse_sample (reference gaussian_diffusion.py:841-877) and of the loop around it:
  * `oracle_loop`: the loop over oracle.sampler.ddim_reverse_step + oracle.mdm_forward.forward with the CFG blend, the inpainting
    blend and the clamp as tests/test_oracle_golden.py::test_ddim_reverse_tiny drives them -- what the reference computes;
  * `step`: the op order of one step in torch, one torch op per rounding, on explicit coefficient rows -- what gdx_ddim_reverse_step
    is compared with bit for bit.  With the rows of the sampling direction (`rows_of(tab, "prev")`) the same statement is the
    ddim_sample step at eta = 0, so `round_trip` inverts and re-generates with one function; `wide=True` keeps its tables and state
    in float64 (the denoiser still runs in fp32 on the rounded state), which measures how far the step arithmetic's own rounding
    moves the result."""
import numpy as np
import torch

from oracle import mdm_forward as omf
from oracle import sampler as osamp


def rows_of(tab, direction="next", dtype=torch.float32):
    """[n, 4] rows (c0, c1, c2, c3) = (sqrt_recip_alphas_cumprod, sqrt_recipm1_alphas_cumprod, sqrt(abar_d), sqrt(1 - abar_d)),
    abar_d = alphas_cumprod_next (the inversion) or alphas_cumprod_prev (ddim_sample at eta 0): each fp64 table is rounded to
    `dtype` first (_extract_into_tensor's .float()), the square roots are taken in `dtype` like the reference's torch ops."""
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dtype)   # noqa: E731
    ab = f(tab.alphas_cumprod_next if direction == "next" else tab.alphas_cumprod_prev)
    return torch.stack([f(tab.sqrt_recip_alphas_cumprod), f(tab.sqrt_recipm1_alphas_cumprod), torch.sqrt(ab), torch.sqrt(1 - ab)], 1)


def step(rows, x, oc, ou=None, scale=None, mask=None, motion=None, clip=False):
    """One step on per-sample rows [B, >= 4] -> (out, m0, eps): m0 = oc -> CFG blend -> inpainting blend -> clamp,
    eps = (c0*x - m0)/c1, out = m0*c2 + c3*eps."""
    c = lambda j: rows[:, j].view(-1, 1, 1, 1)   # noqa: E731
    m0 = oc
    if ou is not None:
        m0 = ou + scale.view(-1, 1, 1, 1) * (oc - ou)
    if mask is not None:
        m0 = torch.where(mask, motion, m0)
    if clip:
        m0 = m0.clamp(-1, 1)
    eps = (c(0) * x - m0) / c(1)
    return m0 * c(2) + c(3) * eps, m0, eps


def x0_of(p, cfg, x, t_model, y, clip=False):
    """The x0 prediction the reference's p_mean_variance forms: (guided) forward -> inpainting blend -> clamp."""
    out = omf.cfg_forward(p, cfg, x, t_model, y) if "scale" in y else omf.forward(p, cfg, x, t_model, y)
    return osamp.process_xstart(osamp.inpaint(out, y), clip)


def oracle_loop(p, cfg, tab, tmap, x, y, until, clip=False, first=0):
    """Indices first .. until - 1 of the inversion through the oracle -> the state at index `until`."""
    mapt = torch.tensor(tmap)
    with torch.no_grad():
        for i in range(first, until):
            t = torch.full((x.shape[0],), i, dtype=torch.long)
            x = osamp.ddim_reverse_step(tab, x0_of(p, cfg, x, mapt[t], y, clip), x, t)
    return x


def round_trip(p, cfg, tab, tmap, x, y, until, clip=False, wide=False):
    """Inversion over indices 0 .. until - 1, then ddim_sample at eta 0 over until .. 0, both through `step` -> (latent, sample).
    wide: rows and state in float64; the denoiser sees the state rounded to fp32."""
    dtype = torch.float64 if wide else torch.float32
    mapt = torch.tensor(tmap)
    up, down = rows_of(tab, "next", dtype), rows_of(tab, "prev", dtype)
    x = x.to(dtype)

    def one(rows, x, i):
        t = torch.full((x.shape[0],), i, dtype=torch.long)
        return step(rows[t], x, x0_of(p, cfg, x.float(), mapt[t], y, clip).to(dtype))[0]
    with torch.no_grad():
        for i in range(until):
            x = one(up, x, i)
        latent = x
        for i in range(until, -1, -1):
            x = one(down, x, i)
    return latent, x
