"""Gaussian diffusion *sampling* process: drop-in for the hot subset of reference
`diffusion/gaussian_diffusion.py` (schedule :20-64, tables :120-199, q_sample :233-251,
p_mean_variance :277-388, p_sample :496-548, p_sample_loop{,_progressive} :598-730,
ddim_sample :732-782, ddim_sample_loop{,_progressive} :879-993).

Host side only builds the fp64 schedule tables (numpy, like the reference) and the per-step fp32
coefficient rows; every per-element operation runs in libgdx.so:

  * `gdx_forward`         the denoiser (through the model callable protocol `model(x, ts, **kw)`)
  * `gdx_sampler_update`  CFG blend + inpainting + posterior mean / DDIM step + noise, one pass
  * `gdx_sample_loop`     the whole loop enqueued from C++ with in-kernel Philox noise
  * `gdx_plms_step` / `gdx_plms_loop`   plms_sample_loop (`:995-1190`): one fused multistep update per step, the loop in C++
  * `gdx_dpm_step` / `gdx_dpm_loop`     dpm_solver_sample_loop: DPM-Solver++ multistep (2M / 3M), additive, same pattern
  * `gdx_dpm_sde_step` / `gdx_dpm_sde_loop`   dpm_solver_sde_sample_loop: its stochastic twin (SDE-DPM-Solver++, orders 1 / 2)
  * `gdx_unipc_step` / `gdx_unipc_loop`   unipc_sample_loop: UniPC, a corrector and the multistep predictor in one launch per step
  * `gdx_window_sweep` / `gdx_parallel_loop`   parallel_sample_loop: parallel-in-time sampling, a window of states per denoiser call
  * `gdx_bpd_terms` / `gdx_bpd_loop`   the variational bound in bits/dim (`_vb_terms_bpd` :1192-1225, `_prior_bpd`
                          :1519-1535, `calc_bpd_loop` :1537-1592, and `training_losses` under LossType.KL / RESCALED_KL)

Configured mode = the one the reference hard-codes (`utils/model_util.py:37-72`): START_X mean, FIXED_SMALL / FIXED_LARGE
variance; this is what `gdx_sample_loop` runs.  The other two readings of the denoiser output, EPSILON and PREVIOUS_X
(`:357-372`), go through the step-wise protocol (one extra element-wise launch per step).  The backward half of training
and cond_fn_with_grad (autograd through the denoiser) raise NotImplementedError, and so do learned variances: they need a
denoiser with twice the channels, which neither MDM has (the reference's own assert at `:317` fires for them).

RNG.  `rng="torch"` (default) draws x_T with `torch.randn` and one N(0,1) tensor per step from torch's
generator on the sample's device, in the reference's order (`:694`, `:532`), so a run is reproducible against
the reference on the same device and seed; the draws are made `NOISE_BLOCK` steps ahead into a tape and the
loop itself runs inside libgdx (`gdx_sample_loop`, one call per block), so the reference caller's own kwargs
(`sample/generate.py:119-130`: `progress=True, noise=None`) take the fused path.  `rng="philox"` generates the
noise inside the update kernel, counter-based and keyed by (seed, global sample index, step): results do not
depend on how a batch is sharded over GPUs.  `noise_tape=` replays recorded noise (parity tests).
"""
import enum
import math

import numpy as np
import torch as th

from .. import engine as E
from .. import sampling_options
from ..engine import GDX_CFG, GDX_COND, GDX_UNCOND
from .._lib import GDX_SAMPLER_DDIM, GDX_SAMPLER_P


def get_named_beta_schedule(schedule_name, num_diffusion_timesteps, scale_betas=1.0):
    if schedule_name == "linear":
        scale = scale_betas * 1000 / num_diffusion_timesteps
        return np.linspace(scale * 0.0001, scale * 0.02, num_diffusion_timesteps, dtype=np.float64)
    if schedule_name == "cosine":
        return betas_for_alpha_bar(num_diffusion_timesteps,
                                   lambda t: math.cos((t + 0.008) / 1.008 * math.pi / 2) ** 2)
    raise NotImplementedError(f"unknown beta schedule: {schedule_name}")


def betas_for_alpha_bar(num_diffusion_timesteps, alpha_bar, max_beta=0.999):
    betas = []
    for i in range(num_diffusion_timesteps):
        t1 = i / num_diffusion_timesteps
        t2 = (i + 1) / num_diffusion_timesteps
        betas.append(min(1 - alpha_bar(t2) / alpha_bar(t1), max_beta))
    return np.array(betas)


class ModelMeanType(enum.Enum):
    PREVIOUS_X = enum.auto()
    START_X = enum.auto()
    EPSILON = enum.auto()


class ModelVarType(enum.Enum):
    LEARNED = enum.auto()
    FIXED_SMALL = enum.auto()
    FIXED_LARGE = enum.auto()
    LEARNED_RANGE = enum.auto()


class LossType(enum.Enum):
    MSE = enum.auto()
    RESCALED_MSE = enum.auto()
    KL = enum.auto()
    RESCALED_KL = enum.auto()

    def is_vb(self):
        return self == LossType.KL or self == LossType.RESCALED_KL


NOISE_BLOCK = 50        # most steps of torch-generator noise drawn ahead of one gdx_sample_loop call (rng="torch") ...
NOISE_BLOCK_BYTES = 256 << 20   # ... within this many bytes of tape (660 MB at config 2 and 6.6 GB at config 5 otherwise)


def noise_block_steps(n_steps, per_step_elems):
    """Steps of pre-drawn noise per gdx_sample_loop call: at most NOISE_BLOCK, at most NOISE_BLOCK_BYTES of fp32 tape, at least one.
    Blocks are issued back to back without a host synchronisation, so smaller blocks cost nothing measurable."""
    by_bytes = NOISE_BLOCK_BYTES // max(1, 4 * int(per_step_elems))
    return max(1, min(int(n_steps), NOISE_BLOCK, by_bytes))


def _is_native(model):
    from ..model.cfg_sampler import ClassifierFreeSampleModel
    from ..model.mdm import _NativeDenoiser
    return isinstance(model, (_NativeDenoiser, ClassifierFreeSampleModel))


class GaussianDiffusion:
    def __init__(self, *, betas, model_mean_type, model_var_type, loss_type, rescale_timesteps=False,
                 lambda_rcxyz=0.0, lambda_vel=0.0, lambda_pose=1.0, lambda_orient=1.0, lambda_loc=1.0,
                 data_rep="rot6d", lambda_root_vel=0.0, lambda_vel_rcxyz=0.0, lambda_fc=0.0):
        self.model_mean_type = model_mean_type
        self.model_var_type = model_var_type
        self.loss_type = loss_type
        self.rescale_timesteps = rescale_timesteps
        self.data_rep = data_rep
        if data_rep != "rot_vel" and lambda_pose != 1.0:
            raise ValueError("lambda_pose is relevant only when training on velocities!")
        self.lambda_pose, self.lambda_orient, self.lambda_loc = lambda_pose, lambda_orient, lambda_loc
        self.lambda_rcxyz, self.lambda_vel, self.lambda_root_vel = lambda_rcxyz, lambda_vel, lambda_root_vel
        self.lambda_vel_rcxyz, self.lambda_fc = lambda_vel_rcxyz, lambda_fc

        betas = np.array(betas, dtype=np.float64)
        self.betas = betas
        assert len(betas.shape) == 1, "betas must be 1-D"
        assert (betas > 0).all() and (betas <= 1).all()
        self.num_timesteps = int(betas.shape[0])

        alphas = 1.0 - betas
        self.alphas_cumprod = np.cumprod(alphas, axis=0)
        self.alphas_cumprod_prev = np.append(1.0, self.alphas_cumprod[:-1])
        self.alphas_cumprod_next = np.append(self.alphas_cumprod[1:], 0.0)
        assert self.alphas_cumprod_prev.shape == (self.num_timesteps,)
        self.sqrt_alphas_cumprod = np.sqrt(self.alphas_cumprod)
        self.sqrt_one_minus_alphas_cumprod = np.sqrt(1.0 - self.alphas_cumprod)
        self.log_one_minus_alphas_cumprod = np.log(1.0 - self.alphas_cumprod)
        self.sqrt_recip_alphas_cumprod = np.sqrt(1.0 / self.alphas_cumprod)
        self.sqrt_recipm1_alphas_cumprod = np.sqrt(1.0 / self.alphas_cumprod - 1)
        self.posterior_variance = betas * (1.0 - self.alphas_cumprod_prev) / (1.0 - self.alphas_cumprod)
        self.posterior_log_variance_clipped = np.log(np.append(self.posterior_variance[1], self.posterior_variance[1:]))
        self.posterior_mean_coef1 = betas * np.sqrt(self.alphas_cumprod_prev) / (1.0 - self.alphas_cumprod)
        self.posterior_mean_coef2 = (1.0 - self.alphas_cumprod_prev) * np.sqrt(alphas) / (1.0 - self.alphas_cumprod)
        self._coef_cache = {}

    # ------------------------------------------------------------------ coefficient rows
    def _model_variance_tables(self):
        if self.model_var_type == ModelVarType.FIXED_LARGE:
            v = np.append(self.posterior_variance[1], self.betas[1:])
            return v, np.log(v)
        if self.model_var_type == ModelVarType.FIXED_SMALL:
            return self.posterior_variance, self.posterior_log_variance_clipped
        raise NotImplementedError("learned variances are outside the sampling hot path")

    def _check_supported(self):
        """START_X (the reference's configuration; the only reading the fused loop takes), EPSILON and PREVIOUS_X
        (step-wise protocol) with fixed variances.  Learned variances need a denoiser with 2x the channels, which neither
        MDM nor MDM_Old has (the reference's own assert at :317 fires for them)."""
        self._model_variance_tables()

    def _xstart_table(self, device):
        """Rows (c0, c1) of gdx_plms_update kind 8 for the configured reading of the denoiser output, rounded like every
        other table (fp64 -> .float()): EPSILON (sqrt_recip_alphas_cumprod, sqrt_recipm1_alphas_cumprod), reference
        :390-396; PREVIOUS_X (1 / posterior_mean_coef1, posterior_mean_coef2 / posterior_mean_coef1), :398-405."""
        key = ("xstart", self.model_mean_type, str(device))
        if key not in self._coef_cache:
            f32 = lambda a: th.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).float()   # noqa: E731
            c = th.zeros(self.num_timesteps, 8, dtype=th.float32)
            if self.model_mean_type == ModelMeanType.EPSILON:
                c[:, 0], c[:, 1] = f32(self.sqrt_recip_alphas_cumprod), f32(self.sqrt_recipm1_alphas_cumprod)
            else:
                c[:, 0] = f32(1.0 / self.posterior_mean_coef1)
                c[:, 1] = f32(self.posterior_mean_coef2 / self.posterior_mean_coef1)
            self._coef_cache[key] = c.to(device)
        return self._coef_cache[key]

    def _identity_mean_table(self, device):
        """The ancestral coefficient rows with mean = 1 * x0-slot + 0 * x_t: PREVIOUS_X takes the denoiser output itself
        as the posterior mean (:361), and 1 * m + 0 * x is m bit for bit."""
        key = ("identity", str(device))
        if key not in self._coef_cache:
            c = self.coef_table(GDX_SAMPLER_P, device).clone()
            c[:, 0], c[:, 1] = 1.0, 0.0
            self._coef_cache[key] = c
        return self._coef_cache[key]

    def coef_table(self, kind, device, eta=0.0):
        """[num_timesteps, 8] fp32 rows consumed by gdx_sampler_update.  Every entry is rounded
        exactly like the reference: fp64 table -> .float() (gaussian_diffusion.py:1595-1608), then
        fp32 torch ops in the reference's order."""
        key = (kind, str(device), eta if eta == "reverse" else float(eta))
        if key in self._coef_cache:
            return self._coef_cache[key]
        self._check_supported()
        f32 = lambda a: th.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).float()   # noqa: E731
        n = self.num_timesteps
        nz = (th.arange(n) != 0).float()
        c = th.zeros(n, 8, dtype=th.float32)
        if kind == GDX_SAMPLER_P:
            _, logvar = self._model_variance_tables()
            c[:, 0] = f32(self.posterior_mean_coef1)
            c[:, 1] = f32(self.posterior_mean_coef2)
            c[:, 2] = nz * th.exp(0.5 * f32(logvar))
            c[:, 3] = f32(self._model_variance_tables()[0])     # model variance, used by condition_mean
        else:
            ab, abp = f32(self.alphas_cumprod), f32(self.alphas_cumprod_prev)
            sigma = (0.0 if eta == "reverse" else eta) * th.sqrt((1 - abp) / (1 - ab)) * th.sqrt(1 - ab / abp)
            c[:, 0] = f32(self.sqrt_recip_alphas_cumprod)
            c[:, 1] = f32(self.sqrt_recipm1_alphas_cumprod)
            c[:, 2] = th.sqrt(abp)
            c[:, 3] = th.sqrt(1 - abp - sigma ** 2)
            c[:, 4] = nz * sigma
        if kind == GDX_SAMPLER_DDIM and eta == "reverse":
            abn = f32(self.alphas_cumprod_next)          # ddim_reverse_sample (:841-877): same kernel, next-alpha rows
            c[:, 2] = th.sqrt(abn)
            c[:, 3] = th.sqrt(1 - abn)
            c[:, 4] = 0.0
        c[:, 5] = f32(self.sqrt_alphas_cumprod)
        c[:, 6] = f32(self.sqrt_one_minus_alphas_cumprod)
        c[:, 7] = nz                                      # (t != 0), used by the PLMS update
        c = c.to(device)
        self._coef_cache[key] = c
        return c

    # ------------------------------------------------------------------ forward process
    def q_sample(self, x_start, t, noise=None):
        if noise is None:
            noise = th.randn_like(x_start)
        assert noise.shape == x_start.shape
        E.require_device(x_start, "x_start")
        coef = self.coef_table(GDX_SAMPLER_P, x_start.device)
        tv = E.require_device(t, "t").reshape(-1).to(th.int64).contiguous()
        return E.q_sample_t(E.f32c(x_start, "x_start"), E.f32c(noise, "noise"), coef, tv)

    def _expand(self, table, t, like):
        """_extract_into_tensor (reference :1595-1608): fp64 table -> gather -> .float() -> expanded view of `like`'s shape."""
        return th.from_numpy(np.ascontiguousarray(table, dtype=np.float64)).to(like.device)[t].float().view(
            -1, *([1] * (like.dim() - 1))).expand(like.shape)

    def q_mean_variance(self, x_start, t):
        """q(x_t | x_0) (reference :216-231): (mean, variance, log_variance), all of x_start's shape.  The mean is the q_sample
        kernel with zero noise (a * x_start + b * 0); the two variance entries are per-sample table values."""
        E.require_device(x_start, "x_start")
        xs = E.f32c(x_start, "x_start")
        tv = E.require_device(t, "t").reshape(-1).to(th.int64).contiguous()
        mean = E.q_sample_t(xs, th.zeros_like(xs), self.coef_table(GDX_SAMPLER_P, xs.device), tv)
        return mean, self._expand(1.0 - self.alphas_cumprod, tv, xs), self._expand(self.log_one_minus_alphas_cumprod, tv, xs)

    def q_posterior_mean_variance(self, x_start, x_t, t):
        """q(x_{t-1} | x_t, x_0) (reference :253-275): (posterior_mean, posterior_variance, posterior_log_variance_clipped).
        The mean is the fused update kernel's coef1 * x_start + coef2 * x_t with zero noise weight."""
        assert x_start.shape == x_t.shape
        E.require_device(x_t, "x_t")
        xt, xs = E.f32c(x_t, "x_t"), E.f32c(x_start, "x_start")
        tv = E.require_device(t, "t").reshape(-1).to(th.int64).contiguous()
        mean = th.empty_like(xt)
        E.sampler_update(GDX_SAMPLER_P, self._posterior_table(xt.device), xt, xs, mean, t=tv, noise=th.zeros_like(xt))
        var, logvar = self._expand(self.posterior_variance, tv, xt), self._expand(self.posterior_log_variance_clipped, tv, xt)
        assert mean.shape[0] == var.shape[0] == logvar.shape[0] == x_start.shape[0]
        return mean, var, logvar

    def _posterior_table(self, device):
        """Ancestral coefficient rows with the POSTERIOR variance whatever model_var_type says (q_posterior_mean_variance is a
        property of the forward process; only columns 0 / 1 are used with zero noise)."""
        key = ("posterior", str(device))
        if key not in self._coef_cache:
            f32 = lambda a: th.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).float()   # noqa: E731
            c = th.zeros(self.num_timesteps, 8, dtype=th.float32)
            c[:, 0], c[:, 1] = f32(self.posterior_mean_coef1), f32(self.posterior_mean_coef2)
            self._coef_cache[key] = c.to(device)
        return self._coef_cache[key]

    def condition_mean(self, cond_fn, p_mean_var, x, t, model_kwargs=None):
        """Sohl-Dickstein conditioning (reference :418-433): p_mean_var["mean"] + p_mean_var["variance"] * cond_fn(x, t, ...).
        The product / sum run in the fused update kernel (identity mean rows: 1 * mean + 0 * x, then + variance * gradient,
        zero noise weight).  The variance is this diffusion's model variance at t -- what p_mean_variance put into the dict."""
        grad = E.f32c(self._call_cond_fn(cond_fn, x, t, model_kwargs or {}), "cond_fn gradient")
        mean = E.f32c(p_mean_var["mean"], "p_mean_var['mean']")
        assert grad.shape == mean.shape == x.shape
        tv = E.require_device(t, "t").reshape(-1).to(th.int64).contiguous()
        out = th.empty_like(mean)
        E.sampler_update(GDX_SAMPLER_P, self._identity_mean_table(mean.device), E.f32c(x, "x"), mean, out, t=tv,
                         noise=th.zeros_like(mean), cond_grad=grad)
        return out

    def condition_score(self, cond_fn, p_mean_var, x, t, model_kwargs=None):
        """Song et al. conditioning (reference :448-472): eps <- eps - sqrt(1 - alpha_bar) * cond_fn(x, t, ...), pred_xstart from
        it (gdx_plms_update kind 7), mean = posterior mean of the new pred_xstart.  Returns a copy of the dict."""
        xc = E.f32c(x, "x")
        grad = E.f32c(self._call_cond_fn(cond_fn, x, t, model_kwargs or {}), "cond_fn gradient")
        tv = E.require_device(t, "t").reshape(-1).to(th.int64).contiguous()
        out = dict(p_mean_var)
        out["pred_xstart"] = E.plms_update(7, self.coef_table(GDX_SAMPLER_DDIM, xc.device), tv, xc,
                                           E.f32c(p_mean_var["pred_xstart"], "pred_xstart"),
                                           eps=(grad, self._cond_coef(xc.device)))
        out["mean"], _, _ = self.q_posterior_mean_variance(x_start=out["pred_xstart"], x_t=xc, t=tv)
        return out

    # ------------------------------------------------------------------ one reverse step
    def _scale_timesteps(self, t):
        if self.rescale_timesteps:
            return t.float() * (1000.0 / self.num_timesteps)
        return t

    def _call_model(self, model, x, t, model_kwargs):
        return model(x, self._scale_timesteps(t), **model_kwargs)

    def _cond_coef(self, device):
        """(1 - alpha_bar).sqrt() in fp32, the factor of condition_score (reference :463-466)."""
        key = ("cond", str(device))
        if key not in self._coef_cache:
            ab = th.from_numpy(np.ascontiguousarray(self.alphas_cumprod, dtype=np.float64)).float()
            self._coef_cache[key] = (1 - ab).sqrt().to(device)
        return self._coef_cache[key]

    def _call_cond_fn(self, cond_fn, x, t, model_kwargs):
        """cond_fn(x, t, **model_kwargs) -> gradient of log p(y | x) (reference condition_mean / condition_score)."""
        return cond_fn(x, self._scale_timesteps(t), **model_kwargs)

    def _step(self, kind, model, x, t, clip_denoised, denoised_fn, cond_fn, model_kwargs, eta=0.0, const_noise=False,
              noise=None):
        if model_kwargs is None:
            model_kwargs = {}
        self._check_supported()
        B, C = x.shape[:2]
        assert t.shape == (B,)
        model_output = self._call_model(model, x, t, model_kwargs)
        y = model_kwargs["y"]                                             # KeyError like the reference (:307)
        mask = motion = None
        if "inpainting_mask" in y.keys() and "inpainted_motion" in y.keys():
            mask, motion = y["inpainting_mask"], y["inpainted_motion"]
            assert model_output.shape == mask.shape == motion.shape
        x0 = E.f32c(model_output, "model output")
        xc = E.f32c(x, "x")
        tt = t.to(th.int64).contiguous()
        mean_type = self.model_mean_type
        raw = None
        if mean_type != ModelMeanType.START_X:
            # EPSILON / PREVIOUS_X (reference :357-372): the x0 prediction is an element-wise function of the output and x_t
            # (gdx_plms_update kind 8); everything downstream (process_xstart, posterior mean, DDIM / PLMS) then sees x0
            # exactly as it does for START_X.  The inpainting blend supports START_X only, as in the reference (:309).
            assert mask is None, 'This feature supports only X_start pred for mow!'
            raw = x0
            x0 = (E.plms_update(8, self._xstart_table(x.device), tt, xc, raw) if mean_type == ModelMeanType.EPSILON
                  else E.plms_update(8, self._xstart_table(x.device), tt, raw, xc))
        if denoised_fn is not None:
            # rare path (every reference caller passes denoised_fn=None): the reference applies the inpainting blend, then
            # denoised_fn, then the clamp (:307-311, :349-355).  The blend runs in the update kernel (its pred_xstart output,
            # zero noise weight irrelevant), the user's callable on the result, the clamp in the update proper.
            if mask is not None:
                blended = th.empty_like(xc)
                E.sampler_update(kind, self.coef_table(kind, x.device, eta), xc, x0, th.empty_like(xc), t=tt,
                                 inpaint_mask=mask.contiguous(), inpaint_motion=E.f32c(motion, "inpainted_motion"),
                                 noise=th.zeros_like(xc), pred_xstart=blended)
                x0, mask, motion = blended, None, None
            x0 = E.f32c(denoised_fn(x0), "denoised_fn output")
        assert x0.shape == x.shape
        if noise is None:
            noise = th.randn_like(x)                                      # drawn even at t == 0 / eta == 0
        if const_noise:
            noise = noise[[0]].contiguous()
        out = th.empty_like(xc)
        pred = th.empty_like(xc)
        grad = gcoef = None
        if cond_fn is not None:
            # condition_mean (ancestral) / condition_score (DDIM), reference :418-494: the gradient is the user's callable,
            # its application to the mean / eps happens inside the fused update kernel
            if eta == "reverse":
                raise NotImplementedError("ddim_reverse_sample takes no cond_fn")
            grad = E.f32c(self._call_cond_fn(cond_fn, x, t, model_kwargs), "cond_fn gradient")
            assert grad.shape == x.shape
            gcoef = self._cond_coef(x.device) if kind == GDX_SAMPLER_DDIM else None
        if mean_type == ModelMeanType.PREVIOUS_X and kind == GDX_SAMPLER_P:
            # the posterior mean IS the output (:361); pred_xstart is only reported (and clamped by the same kernel's
            # pred_xstart output in a pass of its own, zero noise)
            if clip_denoised:
                E.sampler_update(kind, self.coef_table(kind, x.device, eta), xc, x0, th.empty_like(xc), t=tt,
                                 noise=th.zeros_like(xc), pred_xstart=pred, clip_denoised=True)
            else:
                pred = x0
            E.sampler_update(kind, self._identity_mean_table(x.device), xc, raw, out, t=tt, noise=E.f32c(noise, "noise"),
                             const_noise=const_noise, pred_xstart=th.empty_like(xc), cond_grad=grad, cond_coef=gcoef,
                             clip_denoised=False)
            return {"sample": out, "pred_xstart": pred}
        E.sampler_update(kind, self.coef_table(kind, x.device, eta), xc, x0, out, t=tt,
                         inpaint_mask=mask.contiguous() if mask is not None else None,
                         inpaint_motion=E.f32c(motion, "inpainted_motion") if motion is not None else None,
                         noise=E.f32c(noise, "noise"), const_noise=const_noise, pred_xstart=pred, cond_grad=grad,
                         cond_coef=gcoef, clip_denoised=clip_denoised)
        return {"sample": out, "pred_xstart": pred}

    def p_sample(self, model, x, t, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None,
                 const_noise=False):
        return self._step(GDX_SAMPLER_P, model, x, t, clip_denoised, denoised_fn, cond_fn, model_kwargs,
                          const_noise=const_noise)

    def ddim_sample(self, model, x, t, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None,
                    eta=0.0):
        return self._step(GDX_SAMPLER_DDIM, model, x, t, clip_denoised, denoised_fn, cond_fn, model_kwargs, eta=eta)

    def ddim_reverse_sample(self, model, x, t, clip_denoised=True, denoised_fn=None, model_kwargs=None, eta=0.0):
        """Sample x_{t+1} with the DDIM reverse ODE (reference :841-877): one gdx_ddim_reverse_step launch on the next-alpha
        coefficient rows, no noise operand.  A denoised_fn, or an EPSILON / PREVIOUS_X reading of the output, goes through the
        general update kernel with those rows and a zero noise tensor (_step), which gives the same values."""
        assert eta == 0.0, "Reverse ODE only for deterministic path"
        if denoised_fn is not None or self.model_mean_type != ModelMeanType.START_X:
            return self._step(GDX_SAMPLER_DDIM, model, x, t, clip_denoised, denoised_fn, None, model_kwargs, eta="reverse",
                              noise=th.zeros_like(x))
        if model_kwargs is None:
            model_kwargs = {}
        self._check_supported()
        assert t.shape == (x.shape[0],)
        model_output = self._call_model(model, x, t, model_kwargs)
        y = model_kwargs["y"]                                             # KeyError like the reference (:307)
        mask = motion = None
        if "inpainting_mask" in y.keys() and "inpainted_motion" in y.keys():
            mask, motion = y["inpainting_mask"], y["inpainted_motion"]
            assert model_output.shape == mask.shape == motion.shape
        x0 = E.f32c(model_output, "model output")
        xc = E.f32c(x, "x")
        assert x0.shape == x.shape
        out, pred = th.empty_like(xc), th.empty_like(xc)
        E.ddim_reverse_step(self.coef_table(GDX_SAMPLER_DDIM, x.device, "reverse"), xc, x0, out, t=t.to(th.int64).contiguous(),
                            inpaint_mask=mask.contiguous() if mask is not None else None,
                            inpaint_motion=E.f32c(motion, "inpainted_motion") if motion is not None else None,
                            clip_denoised=clip_denoised, pred_out=pred)
        return {"sample": out, "pred_xstart": pred}

    def _inversion_steps(self, eta, until):
        """The checks of the inversion loops -> the number of steps: indices 0 .. until - 1 are executed."""
        assert eta == 0.0, "Reverse ODE only for deterministic path"
        if until is None:
            until = self.num_timesteps - 1
        if isinstance(until, bool) or not isinstance(until, (int, np.integer)) or not 1 <= until <= self.num_timesteps:
            raise ValueError(f"until must be an int with 1 <= until <= num_timesteps = {self.num_timesteps}, got {until!r}")
        return int(until)

    def ddim_reverse_sample_loop(self, model, x_start, clip_denoised=True, denoised_fn=None, model_kwargs=None, device=None,
                                 progress=False, eta=0.0, *, until=None, fused=True):
        """DDIM inversion: x_start, read as the state at index 0 (abar_0, as ddim_reverse_sample reads it), is carried up the
        deterministic DDIM ODE through the indices 0 .. until - 1 -> the state at index `until`.  The default until =
        num_timesteps - 1 is the index whose state ddim_sample_loop(noise=...) takes as x_T; a state at index k is handed back
        with ddim_sample_loop(noise=state, skip_timesteps=num_timesteps - 1 - k, init_is_state=True).  A native START_X denoiser
        (or its ClassifierFreeSampleModel) without denoised_fn runs the whole loop inside libgdx (gdx_ddim_reverse_loop: one
        forward and one fused launch per step); every other case, and fused=False, goes step by step through
        ddim_reverse_sample.  Both give the same bits.  y['guidance_refresh'] > 1 is refused: the refresh is defined for the
        sampling direction.  `device` is accepted for the sampling loops' signature; the state stays where x_start is."""
        n = self._inversion_steps(eta, until)
        self._refuse_refresh(model, model_kwargs, "ddim_reverse_sample_loop (the inversion runs its indices ascending; the "
                                                  "refresh numbers guided calls of a descending loop)")
        if not self._runs_fused(fused, model, denoised_fn, None):
            return self._final_sample(self.ddim_reverse_sample_loop_progressive(
                model, x_start, clip_denoised=clip_denoised, denoised_fn=denoised_fn, model_kwargs=model_kwargs, device=device,
                progress=progress, eta=eta, until=n))
        x, eng, mode, scale, mask, motion = self._fused_setup(model, x_start, model_kwargs or {})
        coef, tmap = self.coef_table(GDX_SAMPLER_DDIM, x.device, "reverse"), self._timestep_map()
        self._issue_blocks(n, x.device, progress, lambda k, nb: eng.ddim_reverse_loop(
            x, mode, coef, tmap, k, nb, scale=scale, inpaint_mask=mask, inpaint_motion=motion, clip_denoised=clip_denoised))
        return x

    def ddim_reverse_sample_loop_progressive(self, model, x_start, clip_denoised=True, denoised_fn=None, model_kwargs=None,
                                             device=None, progress=False, eta=0.0, *, until=None):
        """The inversion step by step: yields ddim_reverse_sample's dict for each index 0 .. until - 1."""
        n = self._inversion_steps(eta, until)
        self._refuse_refresh(model, model_kwargs, "ddim_reverse_sample_loop_progressive")
        indices = range(n)
        if progress:
            from tqdm.auto import tqdm
            indices = tqdm(indices)
        img = x_start
        for i in indices:
            t = th.full((img.shape[0],), i, device=img.device, dtype=th.long)
            with th.no_grad():
                out = self.ddim_reverse_sample(model, img, t, clip_denoised=clip_denoised, denoised_fn=denoised_fn,
                                               model_kwargs=model_kwargs, eta=eta)
            yield out
            img = out["sample"]

    def p_mean_variance(self, model, x, t, clip_denoised=True, denoised_fn=None, model_kwargs=None):
        """Dict API of the reference (:277-388).  mean = update with zero noise; the variance
        entries are per-sample constants expanded to x's shape."""
        zero = th.zeros_like(x)
        r = self._step(GDX_SAMPLER_P, model, x, t, clip_denoised, denoised_fn, None, model_kwargs, noise=zero)
        var, logvar = self._model_variance_tables()
        ex = lambda a: th.from_numpy(a).to(x.device)[t].float().view(-1, *([1] * (x.dim() - 1))).expand(x.shape)  # noqa: E731
        return {"mean": r["sample"], "variance": ex(var), "log_variance": ex(logvar), "pred_xstart": r["pred_xstart"]}

    # ------------------------------------------------------------------ loops
    def _prepare_loop(self, model, shape, noise, device, skip_timesteps, init_image, rng, philox_seed, sample_offset,
                      noise_tape, init_is_state=False):
        """init_is_state: `noise` is the state at the loop's first index itself (an inverted latent) and is used as it is -- no
        q_sample, with or without skip_timesteps."""
        if device is None:
            device = next(model.parameters()).device
        assert isinstance(shape, (tuple, list))
        if noise is not None:
            img = noise
        elif noise_tape is not None:
            img = noise_tape[0]
        elif rng == "philox":
            img = E.randn(tuple(shape), device, philox_seed, sample_offset, 0)
        else:
            img = th.randn(*shape, device=device)
        if skip_timesteps and init_image is None and not init_is_state:
            init_image = th.zeros_like(img)
        indices = list(range(self.num_timesteps - skip_timesteps))[::-1]
        if init_image is not None:
            my_t = th.ones([shape[0]], device=device, dtype=th.long) * indices[0]
            img = self.q_sample(init_image, my_t, img)
        return device, img, indices

    def _loop(self, kind, model, shape, noise, clip_denoised, denoised_fn, cond_fn, model_kwargs, device, progress,
              eta, skip_timesteps, init_image, randomize_class, cond_fn_with_grad, const_noise, rng, philox_seed,
              sample_offset, noise_tape, dump_steps=None, every_step=False, init_is_state=False):
        """every_step: the caller consumes each step's dict (the *_progressive generators, or `fused=False`: the
        step-wise callable protocol model(x, t, **kw) + one gdx_sampler_update per step); otherwise only the final state
        is needed and the whole loop runs inside libgdx."""
        if cond_fn_with_grad or randomize_class:
            raise NotImplementedError("cond_fn_with_grad / randomize_class are outside the sampling hot path")
        if rng not in ("torch", "philox"):
            raise ValueError(f"rng must be 'torch' or 'philox', got {rng!r}")
        device, img, indices = self._prepare_loop(model, shape, noise, device, skip_timesteps, init_image, rng,
                                                  philox_seed, sample_offset, noise_tape, init_is_state)
        fused = self._runs_fused(not every_step, model, denoised_fn, cond_fn)
        if fused:
            yield from self._fused_loop(kind, model, img, indices, model_kwargs, eta, const_noise, rng, philox_seed,
                                        sample_offset, noise_tape, dump_steps, progress, clip_denoised)
            return
        self._refuse_refresh(model, model_kwargs, "a loop that runs step by step (fused=False, a progressive generator, "
                                                  "cond_fn, denoised_fn or a non-native model)")
        if progress:
            from tqdm.auto import tqdm
            indices = tqdm(indices)
        for k, i in enumerate(indices):
            t = th.full((shape[0],), i, device=device, dtype=th.long)
            z = None
            if noise_tape is not None:
                z = noise_tape[1 + k]
            elif rng == "philox":
                z = E.randn(tuple(shape), device, philox_seed, 0 if const_noise else sample_offset, k + 1)
            with th.no_grad():
                out = self._step(kind, model, img, t, clip_denoised, denoised_fn, cond_fn, model_kwargs, eta=eta,
                                 const_noise=const_noise, noise=z)
            yield out
            img = out["sample"]

    def _native_loop_setup(self, model, x, model_kwargs, window=None):
        """What every in-library loop does once in front: input checks, the engine prepared for x's shape and conditioned on
        y['seed'] / y['mfcc'] (and, for a use_text model, on the text features: MDM._text_features), and the loop's operands
        -> (engine, mode, scale, inpainting mask, inpainted motion).  window (parallel_sample_loop): the engine is prepared for
        window x batch samples and the conditioning repeated window-major (Engine.prepare_window)."""
        from ..model.cfg_sampler import ClassifierFreeSampleModel
        y = model_kwargs["y"]
        inner = model.model if isinstance(model, ClassifierFreeSampleModel) else model
        B, T = x.shape[0], x.shape[3]
        inner._check_inputs(x, y)
        if hasattr(inner, "cl_head") and T % 10 != 0:
            from ..model.mdm import _window_error
            raise _window_error(T, 10)
        guided = isinstance(model, ClassifierFreeSampleModel)
        options = sampling_options.read(y, guided=guided, num_layers=inner.num_layers, use_text=getattr(inner, "use_text", False),
                                        pag_only=getattr(model, "pag_only", False))
        options.refuse_conflicts(parallel=window is not None)
        eng = inner._get_engine(x.device)
        options.apply_before_condition(eng)
        if window is None:
            eng.prepare(B, T)
            eng.set_condition(y["seed"], y["mfcc"], text=inner._text_features(y, B), cache=False)
        else:
            eng.prepare_window(B, T, window, y["seed"], y["mfcc"], text=inner._text_features(y, B))
        options.apply_after_condition(eng)           # at every loop: every loop starts with a refresh and a full call
        if guided:
            mode, scale = GDX_CFG, E.f32c(options.scale_operand(y.get("scale") if model.pag_only else y["scale"]), "y['scale']")
        else:
            mode, scale = (GDX_UNCOND if y.get("uncond", False) else GDX_COND), None
        mask = motion = None
        if "inpainting_mask" in y and "inpainted_motion" in y:
            mask = E.require_device(y["inpainting_mask"], "inpainting_mask").to(th.bool).contiguous()
            motion = E.f32c(y["inpainted_motion"], "inpainted_motion")
            assert mask.shape == motion.shape == x.shape
        return eng, mode, scale, mask, motion

    @staticmethod
    def _refuse_refresh(model, model_kwargs, who):
        """A path that calls the model step by step, or whose calls are independent of one another, can serve neither
        y['guidance_refresh'] > 1 nor y['layer_cache'] with every > 1 (sampling_options.MEMORY)."""
        from ..model.cfg_sampler import ClassifierFreeSampleModel
        y = (model_kwargs or {}).get("y")
        if isinstance(y, dict):
            guided = isinstance(model, ClassifierFreeSampleModel)
            inner = getattr(model, "model", model) if guided else model
            layers = getattr(inner, "num_layers", 2**31)                           # a foreign model: keep cannot be judged
            sampling_options.read(y, guided=guided, num_layers=layers, use_text=False,
                                  options=sampling_options.MEMORY).refuse_memory(who)

    def _runs_fused(self, fused, model, denoised_fn, cond_fn):
        """The route of every sampling loop: inside libgdx for a native START_X denoiser (or its ClassifierFreeSampleModel)
        without cond_fn / denoised_fn when the caller allows it (`fused`), else step by step."""
        return (fused and _is_native(model) and denoised_fn is None and cond_fn is None
                and self.model_mean_type == ModelMeanType.START_X)

    @staticmethod
    def _issue_blocks(n, device, progress, issue, block=None):
        """A fused loop of n steps as calls issue(k, nb) -- nb steps from executed step k --, back to back with no host
        synchronisation in between; with `progress` one per block, to report it.  block: most steps per call (_step_noise's);
        None: the whole loop at once, or NOISE_BLOCK steps under `progress`."""
        if block is None:
            block = min(n, NOISE_BLOCK) if progress else n
        bar = None
        if progress:
            from tqdm.auto import tqdm
            bar = tqdm(total=n)
        k = 0
        while k < n:
            nb = min(block, n - k)
            issue(k, nb)
            k += nb
            if bar is not None:
                th.cuda.current_stream(device).synchronize()
                bar.update(nb)
        if bar is not None:
            bar.close()

    @staticmethod
    def _step_noise(tape, rng, n, x, const_noise=False):
        """The step noise of a fused loop of n steps on the state x -> (block, tape_of): tape_of(k, nb) is the noise tape
        of the block of nb steps from executed step k, slice 0 = step k (None: in-kernel Philox).  A recorded `tape` is sliced
        (block None: _issue_blocks chooses).  rng == "torch" without one: one `normal_()` per step in the reference's order
        (:532: randn_like(x) is empty_like(x).normal_()), drawn `block` = noise_block_steps ahead into a buffer the kernels
        read; under const_noise the full draw, sample 0 kept (:534-535)."""
        if tape is not None or rng != "torch":
            return None, lambda k, nb: tape[k:] if tape is not None else None
        rows = 1 if const_noise else x.shape[0]
        block = noise_block_steps(n, rows * math.prod(x.shape[1:]))
        buf = th.empty((block, rows, *x.shape[1:]), device=x.device, dtype=th.float32)
        full = th.empty_like(x) if const_noise else None

        def draw(k, nb):
            for j in range(nb):
                if const_noise:
                    buf[j].copy_(full.normal_()[:1])
                else:
                    buf[j].normal_()
            return buf
        return block, draw

    def _fused_loop(self, kind, model, img, indices, model_kwargs, eta, const_noise, rng, philox_seed, sample_offset,
                    noise_tape, dump_steps, progress, clip_denoised=False):
        """Whole loop inside libgdx (gdx_sample_loop); yields only the final state.  Noise: a recorded tape, in-kernel
        Philox, or torch's generator (_step_noise); issued block by block (_issue_blocks)."""
        self._check_supported()
        x = E.f32c(img, "x_T").clone()
        eng, mode, scale, mask, motion = self._native_loop_setup(model, x, model_kwargs)
        n = len(indices)
        tape = None
        if noise_tape is not None:
            tape = E.f32c(noise_tape[1:1 + n], "noise_tape")
            if const_noise:
                tape = tape[:, :1].contiguous()
        tmap = self._timestep_map()
        dump = None
        if dump_steps is not None:
            dump_steps = sorted({int(s) for s in dump_steps if 0 <= int(s) < n})     # `i in dump_steps`: each step once
            dump = th.empty(len(dump_steps), *x.shape, device=x.device, dtype=th.float32)
        if self.rescale_timesteps:
            raise NotImplementedError("rescale_timesteps=True is not used by the reference's sampler configuration")
        block, tape_of = self._step_noise(tape, rng, n, x, const_noise)
        coef = self.coef_table(kind, x.device, eta)
        self._issue_blocks(n, x.device, progress, lambda k, nb: eng.sample_loop(
            x, kind, mode, coef, tmap, indices[k], scale=scale, inpaint_mask=mask, inpaint_motion=motion,
            noise_tape=tape_of(k, nb), const_noise=const_noise, philox_seed=philox_seed, sample_offset=sample_offset, dump=dump,
            dump_steps=dump_steps, run_steps=nb, k_base=k, clip_denoised=clip_denoised), block)
        yield {"sample": x, "pred_xstart": None, "dump": dump, "fused": True}

    def _timestep_map(self):
        return list(range(self.num_timesteps))

    def guided_steps(self, guidance_interval):
        """Per-step guidance flags of a loop under y['guidance_interval'] = (lo, hi): entry i is True when the MODEL timestep
        of this diffusion's index i -- the respacing map's value, what the denoiser sees -- satisfies lo <= t <= hi (inclusive;
        lo > hi is the empty interval; None = every step).  A loop visits the indices in descending order.  The rule of
        gdx_set_guidance_interval, on the host."""
        tmap = self._timestep_map()
        if guidance_interval is None:
            return [True] * len(tmap)
        lo, hi = guidance_interval
        return [lo <= t <= hi for t in tmap]

    def guidance_plan(self, guidance_interval=None, guidance_refresh=1, plms=False, skip_timesteps=0):
        """What each denoiser call of a sampling loop does under y['guidance_interval'] / y['guidance_refresh'], in execution
        order: "off" (unguided: the conditional pass alone), "refresh" (guided, conditional and unconditional pass) or "reuse"
        (guided, conditional pass alone, the stored difference stands in for the unconditional one).  The loop visits this
        diffusion's indices num_timesteps - 1 - skip_timesteps .. 0; plms: step 0 makes a second call at the index below the
        first (modulo num_timesteps), as plms_sample_loop does.  The guided calls are numbered n = 0, 1, ... in this order and
        call n refreshes when n % guidance_refresh == 0: the rule of gdx_set_guidance_refresh, on the host."""
        every = E.guidance_refresh_value(guidance_refresh)
        flags = self.guided_steps(guidance_interval)
        n_t = self.num_timesteps
        calls = list(range(n_t - skip_timesteps))[::-1]
        if plms and calls:
            calls.insert(1, (calls[0] - 1) % n_t)
        plan, n = [], 0
        for i in calls:
            if not flags[i]:
                plan.append("off")
                continue
            plan.append("refresh" if n % every == 0 else "reuse")
            n += 1
        return plan

    def layer_cache_plan(self, layer_cache, guidance_interval=None, guidance_refresh=1, guided=True, mode=None, plms=False,
                         skip_timesteps=0):
        """What each denoiser call of a sampling loop does under y['layer_cache'] = (every, keep), in execution order: "full"
        (every encoder layer runs and the deep layers' change is stored) or "partial" (the first keep layers run and the
        stored change is added).  guided: the loop of a ClassifierFreeSampleModel, whose calls take the forward modes of
        guidance_plan (a refresh call runs as GDX_CFG; an unguided and a reuse call as GDX_COND); otherwise every call runs in
        `mode` (GDX_COND when None).  ALL calls are numbered m = 0, 1, ...; call m is full when m % every == 0 or when the
        mode stored by the most recent full call does not cover its own (the same mode, or GDX_CFG for a GDX_COND call): the
        rule of gdx_set_layer_cache, on the host.  The plan does not depend on keep."""
        every, _ = E.layer_cache_value(layer_cache, 2**31)
        if guided:
            calls = self.guidance_plan(guidance_interval, guidance_refresh, plms=plms, skip_timesteps=skip_timesteps)
            modes = [GDX_CFG if c == "refresh" else GDX_COND for c in calls]
        else:
            n = self.num_timesteps - skip_timesteps
            modes = [GDX_COND if mode is None else mode] * (n + (1 if plms and n > 0 else 0))
        plan, stored = [], None
        for m, c in enumerate(modes):
            full = m % every == 0 or not (stored == c or (stored == GDX_CFG and c == GDX_COND))
            if full:
                stored = c
            plan.append("full" if full else "partial")
        return plan

    def p_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                      model_kwargs=None, device=None, progress=False, skip_timesteps=0, init_image=None,
                      randomize_class=False, cond_fn_with_grad=False, dump_steps=None, const_noise=False,
                      rng="torch", philox_seed=0, sample_offset=0, noise_tape=None, fused=True):
        final = None
        dump = [] if dump_steps is not None else None
        for i, sample in enumerate(self._loop(GDX_SAMPLER_P, model, shape, noise, clip_denoised, denoised_fn, cond_fn,
                                              model_kwargs, device, progress, 0.0, skip_timesteps, init_image,
                                              randomize_class, cond_fn_with_grad, const_noise, rng, philox_seed,
                                              sample_offset, noise_tape, dump_steps, every_step=not fused)):
            if sample.get("fused"):
                if dump_steps is not None:
                    return [d.clone() for d in sample["dump"]]
                return sample["sample"]
            if dump_steps is not None and i in dump_steps:
                dump.append(sample["sample"].clone())
            final = sample
        if dump_steps is not None:
            return dump
        return final["sample"]

    def p_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                                  model_kwargs=None, device=None, progress=False, skip_timesteps=0, init_image=None,
                                  randomize_class=False, cond_fn_with_grad=False, const_noise=False):
        yield from self._loop(GDX_SAMPLER_P, model, shape, noise, clip_denoised, denoised_fn, cond_fn, model_kwargs,
                              device, progress, 0.0, skip_timesteps, init_image, randomize_class, cond_fn_with_grad,
                              const_noise, "torch", 0, 0, None, every_step=True)

    def ddim_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                         model_kwargs=None, device=None, progress=False, eta=0.0, skip_timesteps=0, init_image=None,
                         randomize_class=False, cond_fn_with_grad=False, dump_steps=None, const_noise=False,
                         rng="torch", philox_seed=0, sample_offset=0, noise_tape=None, fused=True, *, init_is_state=False):
        """init_is_state=True: `noise` IS the state at index num_timesteps - 1 - skip_timesteps -- what
        ddim_reverse_sample_loop(until=that index) returns -- and the loop starts from it as it is (no q_sample); init_image
        must then be None.  False (the default): the reference's behaviour, bit for bit."""
        if dump_steps is not None:
            raise NotImplementedError()                                   # reference :903-904
        if const_noise == True:  # noqa: E712
            raise NotImplementedError()                                   # reference :905-906
        if init_is_state and init_image is not None:
            raise ValueError("init_is_state=True takes the start state from `noise` as it is: init_image must be None")
        if init_is_state and noise is None:
            raise ValueError("init_is_state=True needs the state in `noise`")
        final = None
        for sample in self._loop(GDX_SAMPLER_DDIM, model, shape, noise, clip_denoised, denoised_fn, cond_fn,
                                 model_kwargs, device, progress, eta, skip_timesteps, init_image, randomize_class,
                                 cond_fn_with_grad, False, rng, philox_seed, sample_offset, noise_tape,
                                 every_step=not fused, init_is_state=init_is_state):
            final = sample
        return final["sample"]

    def ddim_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None,
                                     cond_fn=None, model_kwargs=None, device=None, progress=False, eta=0.0,
                                     skip_timesteps=0, init_image=None, randomize_class=False,
                                     cond_fn_with_grad=False):
        yield from self._loop(GDX_SAMPLER_DDIM, model, shape, noise, clip_denoised, denoised_fn, cond_fn,
                              model_kwargs, device, progress, eta, skip_timesteps, init_image, randomize_class,
                              cond_fn_with_grad, False, "torch", 0, 0, None, every_step=True)

    # ------------------------------------------------------------------ parallel-in-time sampling
    def parallel_threshold(self, tolerance):
        """threshold[i] = tolerance^2 * exp(posterior_log_variance_clipped[i]) in float64: the mean squared change a window
        plane may show at index i and still count as converged (ParaDiGMS's scaling; used for the DDIM kind as well)."""
        return float(tolerance) ** 2 * np.exp(np.asarray(self.posterior_log_variance_clipped, dtype=np.float64))

    def parallel_sample_loop(self, model, shape, noise=None, clip_denoised=True, model_kwargs=None, device=None, progress=False,
                             skip_timesteps=0, init_image=None, *, sampler="p", eta=0.0, window=16, tolerance=0.1,
                             philox_seed=0, sample_offset=0, noise_tape=None, report=None):
        """Parallel-in-time sampling (ParaDiGMS, Shih et al. 2023) of p_sample_loop (sampler="p") or ddim_sample_loop ("ddim",
        eta) inside libgdx (gdx_parallel_loop; the rule is in include/gdx.h): a window of `window` consecutive states goes through
        the denoiser as ONE batch of window x B samples, the update chain is re-run over the window with those predictions held
        fixed (gdx_window_sweep), and the window advances past every state whose mean squared change stayed within
        parallel_threshold(tolerance).  Fewer, fatter denoiser calls one after the other, for more denoiser work in total.
        x_T is `noise`, else entry 0 of `noise_tape`, else Philox draw 0, as p_sample_loop(rng="philox") forms it; the step noise is
        the tape's or Philox draw k + 1; init_image / skip_timesteps go through q_sample as in p_sample_loop.  tolerance = 0: the
        fp32 result has the bits of the sequential loop under the same noise.  window = 1 is the sequential loop.  tolerance > 0:
        the stride is decided by the batch's worst sample, so a sample's result depends on the batch it runs in (and on the shard
        under multi-GPU); at tolerance 0 it does not.  report (a dict) receives iterations, strides and forward_samples.
        ValueError for a non-native model, y['guidance_refresh'] > 1, y['layer_cache'] with every > 1 (both need memory across
        sequential calls), a window outside 1 .. 64, a negative or NaN tolerance and another sampler."""
        kinds = {"p": GDX_SAMPLER_P, "ddim": GDX_SAMPLER_DDIM}
        if sampler not in kinds:
            raise ValueError(f"parallel_sample_loop runs sampler 'p' or 'ddim', got {sampler!r}")
        if isinstance(window, bool) or not isinstance(window, (int, np.integer)) or not 1 <= window <= 64:
            raise ValueError(f"window must be an int with 1 <= window <= 64, got {window!r}")
        if isinstance(tolerance, bool) or not isinstance(tolerance, (int, float, np.floating, np.integer)) or not tolerance >= 0:
            raise ValueError(f"tolerance must be a number >= 0 (not NaN), got {tolerance!r}")
        if not _is_native(model) or self.model_mean_type != ModelMeanType.START_X:
            raise ValueError("parallel_sample_loop runs inside libgdx: it needs a native START_X denoiser (MDM / MDM_Old or its "
                             "ClassifierFreeSampleModel)")
        self._refuse_refresh(model, model_kwargs, "parallel_sample_loop (its window evaluates steps side by side)")
        if self.rescale_timesteps:
            raise NotImplementedError("rescale_timesteps=True is not used by the reference's sampler configuration")
        self._check_supported()
        window = int(window)
        device, img, indices = self._prepare_loop(model, shape, noise, device, skip_timesteps, init_image, "philox",
                                                  philox_seed, sample_offset, noise_tape)
        x = E.f32c(img, "x_T")
        n = len(indices)
        eng, mode, scale, mask, motion = self._native_loop_setup(model, x, model_kwargs, window=window)
        planes = x.unsqueeze(0).repeat(window + 1, 1, 1, 1, 1)
        tape = E.f32c(noise_tape[1:1 + n], "noise_tape") if noise_tape is not None else None
        coef, tmap, thr = self.coef_table(kinds[sampler], x.device, eta), self._timestep_map(), self.parallel_threshold(tolerance)
        before = eng.forward_samples()
        bar = None
        if progress:
            from tqdm.auto import tqdm
            bar = tqdm(total=n)
        anchor, strides = 0, []
        while anchor < n:
            new, s = eng.parallel_loop(planes, kinds[sampler], mode, coef, tmap, thr, indices[0], anchor=anchor, scale=scale,
                                       inpaint_mask=mask, inpaint_motion=motion, clip_denoised=clip_denoised, noise_tape=tape,
                                       philox_seed=philox_seed, sample_offset=sample_offset, max_iterations=1 if progress else 0)
            strides += s
            if bar is not None:
                bar.update(new - anchor)
            anchor = new
        if bar is not None:
            bar.close()
        if report is not None:
            report.update(iterations=len(strides), strides=strides, forward_samples=eng.forward_samples() - before)
        return planes[0].clone()

    # ------------------------------------------------------------------ resampling (RePaint)
    @staticmethod
    def _resample_args(jump, repeats):
        for name, v in (("jump", jump), ("repeats", repeats)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v <= 2**31 - 1:
                raise ValueError(f"{name} must be an int >= 1, got {v!r}")
        return int(jump), int(repeats)

    def resample_plan(self, jump, repeats, skip_timesteps=0):
        """The hops of a resampled loop in execution order: ("r", index) is the reverse step at this diffusion's index, ("f", l,
        l + jump) a forward hop between levels, where level L is the input of the reverse step at index L - 1 and level 0 the
        sample.  The loop starts at level N = num_timesteps - skip_timesteps; the jump levels are 0, jump, 2 jump, ... with
        l + jump < N, each with repeats - 1 jumps left; on arriving at one with jumps left the walk uses one up, hops forward and
        descends again.  Denoiser calls: N + n_levels * (repeats - 1) * jump.  The rule of gdx_set_resample
        (csrc/gdx_resample_plan.h), on the host."""
        jump, repeats = self._resample_args(jump, repeats)
        n = self.num_timesteps - skip_timesteps
        left = {l: repeats - 1 for l in range(0, max(n - jump, 0), jump)}
        plan, level = [], n
        while level > 0:
            level -= 1
            plan.append(("r", level))
            if left.get(level, 0) > 0:
                left[level] -= 1
                plan.append(("f", level, level + jump))
                level += jump
        return plan

    def resample_coef(self, plan):
        """The fp32 rows (a, b) of the plan's forward hops, one per hop in execution order, [n_forward, 2]: a = sqrt(r), b =
        sqrt(1 - r) with r = abar[to] / abar[from] and abar = [1, alphas_cumprod ...] by level, computed in float64 and rounded
        once: x <- a x + b z is `to - from` steps of the forward process in one."""
        abar = np.append(1.0, np.asarray(self.alphas_cumprod, dtype=np.float64))
        r = np.array([abar[h[2]] / abar[h[1]] for h in plan if h[0] == "f"], dtype=np.float64)
        return np.stack([np.sqrt(r), np.sqrt(1.0 - r)], axis=1).astype(np.float32).reshape(-1, 2)

    def repaint_sample_loop(self, model, shape, noise=None, clip_denoised=True, model_kwargs=None, device=None, progress=False,
                            skip_timesteps=0, init_image=None, *, sampler="p", eta=0.0, jump=10, repeats=10, rng="torch",
                            philox_seed=0, sample_offset=0, noise_tape=None, fused=True):
        """p_sample_loop (sampler="p") or ddim_sample_loop ("ddim", eta) with RePaint's resampling (Lugmayr et al. 2022,
        arXiv:2201.09865, section 4.2): after the chain has come down `jump` steps it is diffused forward `jump` steps again and
        comes down again, `repeats` times in all (resample_plan), so that the part generated beside y['inpainting_mask'] /
        y['inpainted_motion'] catches up with the known part.  The known part itself is handled as in every loop here -- it
        replaces the x0 prediction of each step --, not noised and pasted into the state as RePaint does.  Without a mask the
        loop still runs, as a plain stochastic resampler of the unconstrained chain.
        Executed hops of both kinds are numbered k = 0, 1, ...: hop k takes entry 1 + k of noise_tape (entry 0 is x_T, so a tape
        holds 1 + len(resample_plan(...)) entries), Philox draw k + 1 (rng="philox"), or one draw from torch's generator in
        execution order.  fused=True on a native START_X denoiser runs inside libgdx (gdx_sample_loop under gdx_set_resample) in
        blocks of at most NOISE_BLOCK hops, the progress bar advancing per block; fused=False, and any other model, runs hop by
        hop -- the model call and gdx_sampler_update, or the noise and gdx_q_sample -- with the same bits.  repeats = 1 is
        p_sample_loop / ddim_sample_loop itself.
        ValueError for jump / repeats that are not ints >= 1, another sampler, y['guidance_refresh'] > 1 or y['layer_cache'] with
        every > 1 (a forward hop invalidates what they carry), a tape of another length than 1 + hops and a tape whose entries do
        not have `shape` (no const_noise-style broadcast)."""
        kinds = {"p": GDX_SAMPLER_P, "ddim": GDX_SAMPLER_DDIM}
        if sampler not in kinds:
            raise ValueError(f"repaint_sample_loop runs sampler 'p' or 'ddim', got {sampler!r}")
        jump, repeats = self._resample_args(jump, repeats)
        if rng not in ("torch", "philox"):
            raise ValueError(f"rng must be 'torch' or 'philox', got {rng!r}")
        if model_kwargs is None:
            model_kwargs = {}
        self._refuse_memory_under_resampling(model, model_kwargs)
        plan =self.resample_plan(jump, repeats, skip_timesteps)
        hops = len(plan)
        if noise_tape is not None:
            if len(noise_tape) != 1 + hops:
                raise ValueError(f"noise_tape must hold x_T and one entry per hop, 1 + {hops}, got {len(noise_tape)}")
            if tuple(noise_tape.shape[1:]) != tuple(shape):
                raise ValueError(f"every noise_tape entry must have the sample's shape {tuple(shape)} (no const_noise-style "
                                 f"broadcast), got {tuple(noise_tape.shape[1:])}")
        kind = kinds[sampler]
        if self.rescale_timesteps:
            raise NotImplementedError("rescale_timesteps=True is not used by the reference's sampler configuration")
        self._check_supported()
        device, img, indices = self._prepare_loop(model, shape, noise, device, skip_timesteps, init_image, rng, philox_seed,
                                                  sample_offset, noise_tape)
        if self._runs_fused(fused, model, None, None):
            return self._fused_repaint_loop(kind, model, img, indices, plan, model_kwargs, eta, jump, repeats, rng, philox_seed,
                                            sample_offset, noise_tape, progress, clip_denoised)
        rows = self.resample_coef(plan)
        ftab = th.zeros(max(len(rows), 1), 8, dtype=th.float32)
        ftab[:len(rows), 5:7] = th.from_numpy(rows)
        ftab = ftab.to(device)
        if progress:
            from tqdm.auto import tqdm
            plan = tqdm(plan)
        n_forward = 0
        for k, hop in enumerate(plan):
            z = None
            if noise_tape is not None:
                z = noise_tape[1 + k]
            elif rng == "philox":
                z = E.randn(tuple(shape), device, philox_seed, sample_offset, k + 1)
            if hop[0] == "r":
                t = th.full((shape[0],), hop[1], device=device, dtype=th.long)
                with th.no_grad():
                    img = self._step(kind, model, img, t, clip_denoised, None, None, model_kwargs, eta=eta, noise=z)["sample"]
            else:
                if z is None:
                    z = th.randn_like(img)
                img = E.q_sample(E.f32c(img, "x"), E.f32c(z, "noise"), ftab, n_forward)
                n_forward += 1
        return img

    @staticmethod
    def _refuse_memory_under_resampling(model, model_kwargs):
        """y['guidance_refresh'] > 1 and y['layer_cache'] with every > 1 (sampling_options.MEMORY) carry a result from one denoiser
        call to the next; a forward hop in between invalidates it, so neither route of repaint_sample_loop serves them."""
        from ..model.cfg_sampler import ClassifierFreeSampleModel
        y = (model_kwargs or {}).get("y")
        if not isinstance(y, dict):
            return
        guided = isinstance(model, ClassifierFreeSampleModel)
        inner = getattr(model, "model", model) if guided else model
        values = sampling_options.read(y, guided=guided, num_layers=getattr(inner, "num_layers", 2**31), use_text=False,
                                       options=sampling_options.MEMORY).values
        for o in sampling_options.MEMORY:
            if o.name in values and o.memory[0](values[o.name]) > 1:
                raise ValueError(f"y['{o.keys[0]}'] = {values[o.name]} does not combine with repaint_sample_loop: a forward hop "
                                 f"invalidates {o.memory[1]}")

    def _fused_repaint_loop(self, kind, model, img, indices, plan, model_kwargs, eta, jump, repeats, rng, philox_seed,
                            sample_offset, noise_tape, progress, clip_denoised):
        """The resampled loop inside libgdx: gdx_sample_loop under gdx_set_resample, issued in blocks of at most NOISE_BLOCK hops
        (_issue_blocks; k_base / run_steps count hops, first_index is the whole loop's); the setter is switched off again whatever
        happens.  repeats = 1: the plain fused loop."""
        if repeats == 1:
            return next(self._fused_loop(kind, model, img, indices, model_kwargs, eta, False, rng, philox_seed, sample_offset,
                                         noise_tape, None, progress, clip_denoised))["sample"]
        x = E.f32c(img, "x_T").clone()
        eng, mode, scale, mask, motion = self._native_loop_setup(model, x, model_kwargs)
        hops = len(plan)
        tape = E.f32c(noise_tape[1:1 + hops], "noise_tape") if noise_tape is not None else None
        block, tape_of = self._step_noise(tape, rng, hops, x)
        coef, tmap = self.coef_table(kind, x.device, eta), self._timestep_map()
        eng.set_resample(jump, repeats, self.alphas_cumprod)
        try:
            self._issue_blocks(hops, x.device, progress, lambda k, nb: eng.sample_loop(
                x, kind, mode, coef, tmap, indices[0], scale=scale, inpaint_mask=mask, inpaint_motion=motion,
                noise_tape=tape_of(k, nb), philox_seed=philox_seed, sample_offset=sample_offset, run_steps=nb, k_base=k,
                clip_denoised=clip_denoised), min(hops, NOISE_BLOCK, block or hops))
        finally:
            eng.set_resample(1, 1)
        return x

    # ------------------------------------------------------------------ explicitly out of scope
    def masked_l2(self, a, b, mask):
        """reference :201-213; a, b [B,J,1,T], mask bool [B,1,1,T] -> [B]."""
        return E.masked_l2(E.f32c(a, "a"), E.f32c(b, "b"), mask)

    def training_losses(self, model, x_start, t, model_kwargs=None, noise=None, dataset=None):
        """FORWARD half of the reference's training_losses (:1227-1352) in its configured mode (LossType.MSE, START_X,
        fixed variance, lambda_vel = lambda_rcxyz = lambda_fc = 0): x_t = q_sample(x_start, t, noise), the model's x0
        prediction, terms['rot_mse'] = masked_l2(x_start, prediction, y['mask']), terms['loss'] = rot_mse.  Under LossType.KL /
        RESCALED_KL (:1258-1268) terms['loss'] is the bound's term at t from _vb_terms_bpd (times num_timesteps when rescaled).
        The values are those the reference would log; there is no autograd graph behind them (training is out of scope,
        SURVEY 2.1)."""
        from . import gaussian_diffusion as _gd
        vb_loss = self.loss_type in (_gd.LossType.KL, _gd.LossType.RESCALED_KL)
        if not vb_loss and self.loss_type not in (_gd.LossType.MSE, _gd.LossType.RESCALED_MSE):
            raise NotImplementedError(self.loss_type)
        self._check_supported()
        for lam in ("lambda_vel", "lambda_rcxyz", "lambda_fc"):
            if getattr(self, lam, 0.0) and not vb_loss:
                raise NotImplementedError(f"{lam} > 0 needs the xyz / velocity terms, which are not on the path")
        mask = model_kwargs["y"]["mask"]                       # KeyError / TypeError like the reference (:1243)
        if noise is None:
            noise = th.randn_like(x_start)
        x_t = self.q_sample(x_start, t, noise=noise)
        if vb_loss:
            # LossType.KL / RESCALED_KL (reference :1258-1268): the bound's term at t, times num_timesteps when rescaled
            loss = self._vb_terms_bpd(model=model, x_start=x_start, x_t=x_t, t=t, clip_denoised=False,
                                      model_kwargs=model_kwargs)["output"]
            if self.loss_type == _gd.LossType.RESCALED_KL:
                loss = loss * self.num_timesteps
            return {"loss": loss}
        with th.no_grad():
            model_output = self._call_model(model, x_t, t, model_kwargs)
        assert model_output.shape == x_start.shape
        terms = {"rot_mse": self.masked_l2(x_start, model_output, mask)}
        terms["loss"] = terms["rot_mse"]
        return terms

    # ------------------------------------------------------------------ variational bound (reference :1192-1225, :1519-1592)
    def bpd_table(self, device):
        """[num_timesteps, 8] fp32 rows consumed by gdx_bpd_terms / gdx_bpd_loop (include/gdx.h), each the fp64 table rounded
        once (.float(), reference :1595-1608): posterior_mean_coef1, posterior_mean_coef2, posterior_log_variance_clipped,
        the model log-variance of _model_variance_tables(), sqrt_recip_alphas_cumprod, sqrt_alphas_cumprod,
        sqrt_one_minus_alphas_cumprod, sqrt_recipm1_alphas_cumprod."""
        key = ("bpd", self.model_var_type, str(device))
        if key not in self._coef_cache:
            f32 = lambda a: th.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).float()   # noqa: E731
            c = th.zeros(self.num_timesteps, 8, dtype=th.float32)
            for col, tab in enumerate((self.posterior_mean_coef1, self.posterior_mean_coef2,
                                       self.posterior_log_variance_clipped, self._model_variance_tables()[1],
                                       self.sqrt_recip_alphas_cumprod, self.sqrt_alphas_cumprod,
                                       self.sqrt_one_minus_alphas_cumprod, self.sqrt_recipm1_alphas_cumprod)):
                c[:, col] = f32(tab)
            self._coef_cache[key] = c.to(device)
        return self._coef_cache[key]

    def _prior_log_variance(self):
        """log_one_minus_alphas_cumprod at the last step, rounded to fp32 as _extract_into_tensor would."""
        return float(np.float32(self.log_one_minus_alphas_cumprod[self.num_timesteps - 1]))

    def _bpd_step(self, model, x_start, x_t, t, clip_denoised, model_kwargs, noise=None):
        """One denoiser call + gdx_bpd_terms -> (vb [B], xstart_mse [B], mse [B] or None, pred_xstart)."""
        if model_kwargs is None:
            model_kwargs = {}
        self._check_supported()
        E.require_device(x_t, "x_t")
        xs, xt = E.f32c(x_start, "x_start"), E.f32c(x_t, "x_t")
        assert xs.shape == xt.shape and t.shape == (xs.shape[0],)
        tt = E.require_device(t, "t").to(th.int64).contiguous()
        with th.no_grad():
            raw = E.f32c(self._call_model(model, xt, t, model_kwargs), "model output")
        assert raw.shape == xt.shape
        y = model_kwargs["y"]                                             # KeyError like the reference (:307)
        mask = motion = None
        if "inpainting_mask" in y.keys() and "inpainted_motion" in y.keys():
            mask = E.require_device(y["inpainting_mask"], "inpainting_mask").to(th.bool).contiguous()
            motion = E.f32c(y["inpainted_motion"], "inpainted_motion")
            assert raw.shape == mask.shape == motion.shape
        x0, mean = raw, None
        if self.model_mean_type != ModelMeanType.START_X:
            # EPSILON / PREVIOUS_X (reference :357-372): the x0 prediction comes from gdx_plms_update kind 8; PREVIOUS_X also
            # hands the raw output over as the model's posterior mean (:361)
            assert mask is None, 'This feature supports only X_start pred for mow!'
            if self.model_mean_type == ModelMeanType.EPSILON:
                x0 = E.plms_update(8, self._xstart_table(xt.device), tt, xt, raw)
            else:
                x0, mean = E.plms_update(8, self._xstart_table(xt.device), tt, raw, xt), raw
        return E.bpd_terms(self.bpd_table(xt.device), xs, xt, x0, noise=E.f32c(noise, "noise") if noise is not None else None,
                           t=tt, inpaint_mask=mask, inpaint_motion=motion, model_mean=mean, clip_denoised=clip_denoised)

    def _vb_terms_bpd(self, model, x_start, x_t, t, clip_denoised=True, model_kwargs=None):
        """A term of the variational bound in bits/dim (reference :1192-1225): the decoder NLL where t == 0, else
        KL(q(x_{t-1} | x_t, x_0) || p(x_{t-1} | x_t)); {'output': [B], 'pred_xstart'}.  One fused kernel pass (gdx_bpd_terms)."""
        vb, _, _, pred = self._bpd_step(model, x_start, x_t, t, clip_denoised, model_kwargs)
        return {"output": vb, "pred_xstart": pred}

    def _prior_bpd(self, x_start):
        """The prior term KL(q(x_T | x_0) || N(0, 1)) in bits/dim (reference :1519-1535) -> [B]."""
        xs = E.f32c(x_start, "x_start")
        return E.bpd_prior(self.bpd_table(xs.device), xs, self.num_timesteps - 1, self._prior_log_variance())

    def calc_bpd_loop(self, model, x_start, clip_denoised=True, model_kwargs=None, *, rng="torch", philox_seed=0,
                      sample_offset=0, noise_tape=None, progress=False, fused=True):
        """The whole variational bound in bits/dim with the per-timestep x0 / eps error curves (reference :1537-1592):
        {'total_bpd' [B], 'prior_bpd' [B], 'vb' / 'xstart_mse' / 'mse' [B, num_timesteps]}, columns in descending t.
        A native denoiser (or its ClassifierFreeSampleModel) read as START_X runs the loop inside libgdx (gdx_bpd_loop);
        any other callable, EPSILON / PREVIOUS_X, or fused=False go step by step through _vb_terms_bpd's kernel.  Noise:
        rng="torch" draws one normal_() per step in the reference's order (:1563), rng="philox" is counter-based (draw number
        = executed step k, keyed by sample_offset + b), noise_tape [num_timesteps, B, J, 1, T] replays recorded draws."""
        if rng not in ("torch", "philox"):
            raise ValueError(f"rng must be 'torch' or 'philox', got {rng!r}")
        if model_kwargs is None:
            model_kwargs = {}
        self._refuse_refresh(model, model_kwargs, "calc_bpd_loop (its steps draw independent x_t)")
        self._check_supported()
        xs = E.f32c(x_start, "x_start")
        B, n, dev_ = xs.shape[0], self.num_timesteps, xs.device
        tape = E.f32c(noise_tape, "noise_tape") if noise_tape is not None else None
        if tape is not None:
            assert tuple(tape.shape) == (n, *xs.shape), "noise_tape must be [num_timesteps, B, J, 1, T]"
        if self._runs_fused(fused, model, None, None):
            vb, xm, em, prior = self._fused_bpd_loop(model, xs, clip_denoised, model_kwargs, rng, philox_seed, sample_offset,
                                                     tape, progress)
        else:
            vb, xm, em = (th.empty(B, n, device=dev_, dtype=th.float32) for _ in range(3))
            steps = range(n)
            if progress:
                from tqdm.auto import tqdm
                steps = tqdm(steps)
            for k in steps:
                t = th.full((B,), n - 1 - k, device=dev_, dtype=th.long)
                if tape is not None:
                    z = tape[k]
                elif rng == "philox":
                    z = E.randn(tuple(xs.shape), dev_, philox_seed, sample_offset, k)
                else:
                    z = th.randn_like(xs)
                x_t = self.q_sample(xs, t, noise=z)
                vb[:, k], xm[:, k], em[:, k], _ = self._bpd_step(model, xs, x_t, t, clip_denoised, model_kwargs, noise=z)
            prior = self._prior_bpd(xs)
        return {"total_bpd": vb.sum(dim=1) + prior, "prior_bpd": prior, "vb": vb, "xstart_mse": xm, "mse": em}

    def _fused_bpd_loop(self, model, xs, clip_denoised, model_kwargs, rng, philox_seed, sample_offset, tape, progress):
        """gdx_bpd_loop, issued block by block like _fused_loop (torch-generator noise is drawn NOISE_BLOCK steps ahead)."""
        if self.rescale_timesteps:
            raise NotImplementedError("rescale_timesteps=True is not used by the reference's sampler configuration")
        eng, mode, scale, mask, motion = self._native_loop_setup(model, xs, model_kwargs)
        B, n = xs.shape[0], self.num_timesteps
        vb, xm, em = (th.empty(B, n, device=xs.device, dtype=th.float32) for _ in range(3))
        prior = th.empty(B, device=xs.device, dtype=th.float32)
        block, tape_of = self._step_noise(tape, rng, n, xs)
        coef, tmap = self.bpd_table(xs.device), self._timestep_map()
        self._issue_blocks(n, xs.device, progress, lambda k, nb: eng.bpd_loop(
            xs, mode, coef, tmap, vb, xm, em, scale=scale, inpaint_mask=mask, inpaint_motion=motion, noise_tape=tape_of(k, nb),
            philox_seed=philox_seed, sample_offset=sample_offset, clip_denoised=clip_denoised, run_steps=nb, k_base=k,
            prior_bpd=prior if k + nb == n else None, prior_log_variance=self._prior_log_variance()), block)
        return vb, xm, em, prior

    # ------------------------------------------------------------------ PLMS (reference :995-1190)
    def _pred_xstart(self, model, x, t, clip_denoised, denoised_fn, model_kwargs):
        """p_mean_variance's pred_xstart (model output after CFG / inpainting / clipping)."""
        return self._step(GDX_SAMPLER_P, model, x, t, clip_denoised, denoised_fn, None, model_kwargs,
                          noise=th.zeros_like(x))["pred_xstart"]

    def _condition_score_xstart(self, cond_fn, x, t, pred, model_kwargs):
        """pred_xstart under condition_score (reference :452-472), or `pred` itself without a cond_fn."""
        if cond_fn is None:
            return pred
        grad = E.f32c(self._call_cond_fn(cond_fn, x, t, model_kwargs), "cond_fn gradient")
        return E.plms_update(7, self.coef_table(GDX_SAMPLER_DDIM, x.device, 0.0), t, x, pred,
                             eps=[grad, self._cond_coef(x.device)])

    @staticmethod
    def _uniform_t(who, x, t):
        """The operands of a DPM-Solver++ step `who` -> (x, t, i): t must be the index i for the whole batch (the history
        belongs to one index sequence)."""
        xc = E.f32c(x, "x")
        tt = E.require_device(t, "t").to(th.int64).contiguous()
        rows = set(tt.tolist())
        if len(rows) != 1:
            raise ValueError(f"{who}: t must be the same for the whole batch")
        return xc, tt, rows.pop()

    @staticmethod
    def _history_step(order, old_out, i, used, step):
        """The history protocol of the DPM-Solver++ steps: sample = step(cur, hist) with cur = min(order, predictions kept
        + 1, i + 1) and hist the cur - 1 newest of old_out["old_pred"], newest first -> (sample, the old_pred to hand on:
        oldest first, at most order - 1 kept)."""
        old_pred = list(old_out["old_pred"]) if old_out is not None else []
        cur = min(order, len(old_pred) + 1, i + 1)
        sample = step(cur, old_pred[::-1][:cur - 1])
        old_pred.append(used)
        return sample, old_pred[-(order - 1):] if order > 1 else []

    def plms_sample(self, model, x, t, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None,
                    cond_fn_with_grad=False, order=2, old_out=None):
        """Pseudo linear multistep step (reference :995-1079): eps from the x0 prediction, pseudo improved Euler on
        the first step (one extra model call at t-1), Adams-Bashforth of order <= `order` afterwards.  The
        element-wise arithmetic runs in gdx_plms_update with the reference's op order."""
        if not int(order) or not 1 <= order <= 4:
            raise ValueError('order is invalid (should be int from 1-4).')
        if cond_fn_with_grad:
            raise NotImplementedError("cond_fn_with_grad needs autograd through the denoiser (outside the hot path)")
        coef = self.coef_table(GDX_SAMPLER_DDIM, x.device, 0.0)
        xc = E.f32c(x, "x")
        tt = t.to(th.int64).contiguous()

        def get_model_output(xx, ts):
            """(eps, pred_xstart used downstream, original pred_xstart), reference get_model_output :1015-1041."""
            orig = self._pred_xstart(model, xx, ts, clip_denoised, denoised_fn, model_kwargs)
            used = self._condition_score_xstart(cond_fn, xx, ts, orig, model_kwargs)
            return E.plms_update(0, coef, ts, xx, used), used, orig
        eps, x0, x0_orig = get_model_output(xc, tt)
        if order > 1 and old_out is None:
            old_eps = [eps]
            mean_pred = E.plms_update(6, coef, tt, None, x0, eps=[eps])
            t2 = (tt - 1) % self.num_timesteps            # t - 1 (a negative index wraps in the reference's table gather)
            eps_2, _, _ = get_model_output(mean_pred, t2)
            sample = E.plms_update(5, coef, tt, xc, x0, eps=[eps, eps_2])
        else:
            old_eps = old_out["old_eps"]                  # TypeError on the first step with order == 1, like the reference
            old_eps.append(eps)
            cur = min(order, len(old_eps))
            sample = E.plms_update(cur, coef, tt, xc, x0, eps=old_eps[::-1][:cur])
        if len(old_eps) >= order:
            old_eps.pop(0)
        return {"sample": sample, "pred_xstart": x0_orig, "old_eps": old_eps}

    def plms_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                         model_kwargs=None, device=None, progress=False, skip_timesteps=0, init_image=None,
                         randomize_class=False, cond_fn_with_grad=False, order=2, *, fused=True, rng="torch", philox_seed=0,
                         sample_offset=0):
        """plms_sample_loop of the reference (:1081-1134).  A native START_X denoiser (or its ClassifierFreeSampleModel)
        without cond_fn / denoised_fn runs the whole loop inside libgdx (gdx_plms_loop: one forward and one fused update
        launch per step); every other case, and fused=False, goes step by step through plms_sample.  Both give the same
        bits.  rng / philox_seed / sample_offset choose how x_T is drawn when `noise` is None (the sampler draws nothing else)."""
        if rng not in ("torch", "philox"):
            raise ValueError(f"rng must be 'torch' or 'philox', got {rng!r}")
        if self._runs_fused(fused, model, denoised_fn, cond_fn) and not cond_fn_with_grad and not randomize_class:
            if not int(order) or not 1 <= order <= 4:
                raise ValueError('order is invalid (should be int from 1-4).')
            if order == 1:          # the reference subscripts old_out = None on the first step (:1053)
                raise TypeError("'NoneType' object is not subscriptable")
            if model_kwargs is None:
                model_kwargs = {}
            device, img, indices = self._prepare_loop(model, shape, noise, device, skip_timesteps, init_image, rng,
                                                      philox_seed, sample_offset, None)
            return self._fused_plms_loop(model, img, indices, model_kwargs, int(order), progress, clip_denoised)
        return self._final_sample(self.plms_sample_loop_progressive(
            model, shape, noise=noise, clip_denoised=clip_denoised, denoised_fn=denoised_fn, cond_fn=cond_fn,
            model_kwargs=model_kwargs, device=device, progress=progress, skip_timesteps=skip_timesteps, init_image=init_image,
            randomize_class=randomize_class, cond_fn_with_grad=cond_fn_with_grad, order=order, rng=rng, philox_seed=philox_seed,
            sample_offset=sample_offset))

    @staticmethod
    def _final_sample(steps):
        final = None
        for sample in steps:
            final = sample
        return final["sample"]

    def _fused_setup(self, model, img, model_kwargs):
        """The front of a fused multistep loop -> (x, engine, mode, scale, mask, motion): x = a private copy of the start
        state, updated in place by the loop; the rest from _native_loop_setup."""
        self._check_supported()
        if self.rescale_timesteps:
            raise NotImplementedError("rescale_timesteps=True is not used by the reference's sampler configuration")
        x = E.f32c(img, "x_T").clone()
        return (x, *self._native_loop_setup(model, x, model_kwargs))

    def _stepwise(self, step, model, shape, noise, device, progress, skip_timesteps, init_image, rng, philox_seed,
                  sample_offset, noise_tape=None, step_noise=False, **step_kw):
        """The step-by-step form of a multistep sampling loop: yields step(model, x, t, old_out=previous, **step_kw) per
        index.  step_noise: the steps take noise -- entry 1 + k of the tape, or the Philox draw k + 1 (rng == "philox"), or
        the step's own draw from torch's generator."""
        self._refuse_refresh(model, step_kw.get("model_kwargs"), "a loop that runs step by step (fused=False, a progressive "
                                                                 "generator, cond_fn, denoised_fn or a non-native model)")
        device, img, indices = self._prepare_loop(model, shape, noise, device, skip_timesteps, init_image, rng,
                                                  philox_seed, sample_offset, noise_tape)
        if progress:
            from tqdm.auto import tqdm
            indices = tqdm(indices)
        old_out = None
        for k, i in enumerate(indices):
            t = th.full((shape[0],), i, device=device, dtype=th.long)
            if step_noise:
                z = noise_tape[1 + k] if noise_tape is not None else None
                step_kw.update(noise=z, philox_seed=philox_seed, sample_offset=sample_offset,
                               rng_step=k + 1 if z is None and rng == "philox" else None)
            with th.no_grad():
                out = step(model, img, t, old_out=old_out, **step_kw)
            yield out
            old_out = out
            img = out["sample"]

    def _fused_plms_loop(self, model, img, indices, model_kwargs, order, progress, clip_denoised):
        """Whole loop inside libgdx (gdx_plms_loop).  The eps history and the first step's predictor live in two tensors of
        this call; with `progress` the loop is issued in blocks of NOISE_BLOCK steps, one synchronisation per block."""
        x, eng, mode, scale, mask, motion = self._fused_setup(model, img, model_kwargs)
        coef, tmap = self.coef_table(GDX_SAMPLER_DDIM, x.device, 0.0), self._timestep_map()
        hist = th.empty((order, *x.shape), device=x.device, dtype=th.float32)
        scratch = th.empty_like(x)
        self._issue_blocks(len(indices), x.device, progress, lambda k, nb: eng.plms_loop(
            x, mode, order, coef, tmap, indices[k], hist, scratch, scale=scale, inpaint_mask=mask, inpaint_motion=motion,
            clip_denoised=clip_denoised, run_steps=nb, k_base=k))
        return x

    def plms_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None,
                                     cond_fn=None, model_kwargs=None, device=None, progress=False, skip_timesteps=0,
                                     init_image=None, randomize_class=False, cond_fn_with_grad=False, order=2, *,
                                     rng="torch", philox_seed=0, sample_offset=0):
        if randomize_class:
            raise NotImplementedError("randomize_class is outside the sampling hot path")
        yield from self._stepwise(self.plms_sample, model, shape, noise, device, progress, skip_timesteps, init_image, rng,
                                  philox_seed, sample_offset, clip_denoised=clip_denoised, denoised_fn=denoised_fn,
                                  cond_fn=cond_fn, model_kwargs=model_kwargs, cond_fn_with_grad=cond_fn_with_grad, order=order)

    # ------------------------------------------------------------------ DPM-Solver++ multistep (no counterpart in the reference)
    def dpm_coef_rows(self):
        """The fp64 rows behind dpm_coef_table: [num_timesteps, 8] = (a, w1_0, w2_0, w2_1, w3_0, w3_1, w3_2, 0), the
        DPM-Solver++ multistep update of order 1..3 (Lu et al. 2022, arXiv:2211.01095) collected into weights of the x0
        predictions m0 (this step), m1, m2 (the two executed before it, at indices i + 1, i + 2): x' = a*x + sum_j w_j*m_j.
        Formulas, special rows and the order rule: include/gdx.h at gdx_dpm_step / gdx_dpm_loop."""
        n = self.num_timesteps
        ab, abp = self.alphas_cumprod, self.alphas_cumprod_prev
        lam = 0.5 * np.log(ab / (1.0 - ab))
        rows = np.zeros((n, 8), dtype=np.float64)
        rows[0, 1] = 1.0                                  # abar_p = 1: sigma_p = 0, h = inf, a = 0, phi = 1
        for i in range(1, n):
            alpha_p = math.sqrt(abp[i])
            h = 0.5 * math.log(abp[i] / (1.0 - abp[i])) - lam[i]
            em1 = math.expm1(-h)
            phi = -alpha_p * em1
            rows[i, 0] = math.sqrt(1.0 - abp[i]) / math.sqrt(1.0 - ab[i])
            rows[i, 1] = phi
            if i + 1 < n:
                r0 = (lam[i] - lam[i + 1]) / h
                rows[i, 2] = phi + 0.5 * phi / r0
                rows[i, 3] = -0.5 * phi / r0
            if i + 2 < n:
                r1 = (lam[i + 1] - lam[i + 2]) / h
                c1 = alpha_p * (em1 / h + 1.0)
                c2 = alpha_p * ((em1 + h) / (h * h) - 0.5)
                rho = r0 / (r0 + r1)
                d10 = c1 * (1.0 + rho) - c2 / (r0 + r1)   # weight of D1_0 = (m0 - m1) / r0
                d11 = c2 / (r0 + r1) - c1 * rho           # weight of D1_1 = (m1 - m2) / r1
                rows[i, 4] = phi + d10 / r0
                rows[i, 5] = d11 / r1 - d10 / r0
                rows[i, 6] = -d11 / r1
        return rows

    def dpm_coef_table(self, device):
        """[num_timesteps, 8] fp32 rows consumed by gdx_dpm_step / gdx_dpm_loop: dpm_coef_rows rounded once (.float(), the
        convention of every other table here)."""
        key = ("dpm", str(device))
        if key not in self._coef_cache:
            self._coef_cache[key] = th.from_numpy(self.dpm_coef_rows()).float().to(device)
        return self._coef_cache[key]

    def dpm_solver_sample(self, model, x, t, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None, order=2,
                          old_out=None):
        """One DPM-Solver++ multistep step (gdx_dpm_step): the x0 prediction from _pred_xstart (so EPSILON / PREVIOUS_X /
        denoised_fn work as elsewhere; cond_fn through condition_score), then the update of order min(order, predictions
        kept + 1, t + 1) over it and old_out["old_pred"] (oldest first, at most order - 1 kept).  t must be the same for the
        whole batch: the history belongs to one index sequence.  Returns {"sample", "pred_xstart", "old_pred"}."""
        if order not in (1, 2, 3):
            raise ValueError('order is invalid (should be int from 1-3).')
        xc, tt, i = self._uniform_t("dpm_solver_sample", x, t)
        pred = self._pred_xstart(model, xc, tt, clip_denoised, denoised_fn, model_kwargs)
        used = self._condition_score_xstart(cond_fn, xc, tt, pred, model_kwargs or {})
        sample, old_pred = self._history_step(order, old_out, i, used, lambda cur, hist: E.dpm_step(
            cur, self.dpm_coef_table(xc.device), xc, used, th.empty_like(xc), hist=hist, step_index=i))
        return {"sample": sample, "pred_xstart": pred, "old_pred": old_pred}

    def dpm_solver_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                               model_kwargs=None, device=None, progress=False, skip_timesteps=0, init_image=None,
                               randomize_class=False, cond_fn_with_grad=False, order=2, *, fused=True, rng="torch",
                               philox_seed=0, sample_offset=0):
        """DPM-Solver++ multistep sampling (2M by default) with plms_sample_loop's signature.  A native START_X denoiser (or
        its ClassifierFreeSampleModel) without cond_fn / denoised_fn runs the whole loop inside libgdx (gdx_dpm_loop: one
        forward and one fused update launch per step); every other case, and fused=False, goes step by step through
        dpm_solver_sample.  Both give the same bits.  The solver gains its order only on steps spaced evenly in log-SNR:
        use the "logsnrN" respacing.  rng / philox_seed / sample_offset choose how x_T is drawn when `noise` is None (the
        sampler draws nothing else)."""
        if rng not in ("torch", "philox"):
            raise ValueError(f"rng must be 'torch' or 'philox', got {rng!r}")
        if order not in (1, 2, 3):
            raise ValueError('order is invalid (should be int from 1-3).')
        if cond_fn_with_grad or randomize_class:
            raise NotImplementedError("cond_fn_with_grad / randomize_class are outside the sampling hot path")
        if self._runs_fused(fused, model, denoised_fn, cond_fn):
            if model_kwargs is None:
                model_kwargs = {}
            device, img, indices = self._prepare_loop(model, shape, noise, device, skip_timesteps, init_image, rng,
                                                      philox_seed, sample_offset, None)
            return self._fused_dpm_loop(model, img, indices, model_kwargs, int(order), progress, clip_denoised)
        return self._final_sample(self.dpm_solver_sample_loop_progressive(
            model, shape, noise=noise, clip_denoised=clip_denoised, denoised_fn=denoised_fn, cond_fn=cond_fn,
            model_kwargs=model_kwargs, device=device, progress=progress, skip_timesteps=skip_timesteps, init_image=init_image,
            order=order, rng=rng, philox_seed=philox_seed, sample_offset=sample_offset))

    def _fused_dpm_loop(self, model, img, indices, model_kwargs, order, progress, clip_denoised):
        """Whole loop inside libgdx (gdx_dpm_loop).  The history of x0 predictions lives in a tensor of this call; with
        `progress` the loop is issued in blocks of NOISE_BLOCK steps, one synchronisation per block."""
        x, eng, mode, scale, mask, motion = self._fused_setup(model, img, model_kwargs)
        coef, tmap = self.dpm_coef_table(x.device), self._timestep_map()
        hist = th.empty((order, *x.shape), device=x.device, dtype=th.float32) if order > 1 else None
        self._issue_blocks(len(indices), x.device, progress, lambda k, nb: eng.dpm_loop(
            x, mode, order, coef, tmap, indices[k], hist, scale=scale, inpaint_mask=mask, inpaint_motion=motion,
            clip_denoised=clip_denoised, run_steps=nb, k_base=k))
        return x

    def dpm_solver_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None,
                                           cond_fn=None, model_kwargs=None, device=None, progress=False, skip_timesteps=0,
                                           init_image=None, randomize_class=False, cond_fn_with_grad=False, order=2, *,
                                           rng="torch", philox_seed=0, sample_offset=0):
        if cond_fn_with_grad or randomize_class:
            raise NotImplementedError("cond_fn_with_grad / randomize_class are outside the sampling hot path")
        yield from self._stepwise(self.dpm_solver_sample, model, shape, noise, device, progress, skip_timesteps, init_image, rng,
                                  philox_seed, sample_offset, clip_denoised=clip_denoised, denoised_fn=denoised_fn,
                                  cond_fn=cond_fn, model_kwargs=model_kwargs, order=order)

    # ------------------------------------------------------------------ SDE-DPM-Solver++ multistep (no counterpart in the reference)
    def dpm_sde_coef_rows(self, eta=1.0):
        """The fp64 rows behind dpm_sde_coef_table: [num_timesteps, 8] = (a, w1_0, w2_0, w2_1, 0, 0, 0, s), the stochastic
        DPM-Solver++ multistep update of order 1..2 (Lu et al. 2022, arXiv:2211.01095, at eta = 1; eta scales the injected
        noise): x' = a*x + sum_j w_j*m_j + s*z.  The layout of dpm_coef_rows with the noise scale in column 7; at eta = 0
        columns 0..3 are dpm_coef_rows bit for bit (the expressions below are those, with the factors eta adds written so
        that they are exact there) and s = 0.  Formulas and special rows: include/gdx.h at gdx_dpm_sde_step."""
        eta = float(eta)
        if not eta >= 0.0:
            raise ValueError(f"eta must be >= 0, got {eta!r}")
        n = self.num_timesteps
        ab, abp = self.alphas_cumprod, self.alphas_cumprod_prev
        lam = 0.5 * np.log(ab / (1.0 - ab))
        rows = np.zeros((n, 8), dtype=np.float64)
        rows[0, 1] = 1.0                                  # abar_p = 1: sigma_p = 0, h = inf, a = 0, phi = 1, s = 0
        for i in range(1, n):
            alpha_p = math.sqrt(abp[i])
            h = 0.5 * math.log(abp[i] / (1.0 - abp[i])) - lam[i]
            em1 = math.expm1(-((1.0 + eta) * h))
            phi = -alpha_p * em1
            rows[i, 0] = math.sqrt(1.0 - abp[i]) / math.sqrt(1.0 - ab[i]) * math.exp(-eta * h)
            rows[i, 1] = phi
            if i + 1 < n:
                r0 = (lam[i] - lam[i + 1]) / h
                rows[i, 2] = phi + 0.5 * phi / r0
                rows[i, 3] = -0.5 * phi / r0
            rows[i, 7] = math.sqrt(1.0 - abp[i]) * math.sqrt(-math.expm1(-2.0 * eta * h))
        return rows

    def dpm_sde_coef_table(self, device, eta=1.0):
        """[num_timesteps, 8] fp32 rows consumed by gdx_dpm_sde_step / gdx_dpm_sde_loop: dpm_sde_coef_rows(eta) rounded once
        (.float()), cached per (device, eta)."""
        key = ("dpm_sde", str(device), float(eta))
        if key not in self._coef_cache:
            self._coef_cache[key] = th.from_numpy(self.dpm_sde_coef_rows(eta)).float().to(device)
        return self._coef_cache[key]

    def dpm_solver_sde_sample(self, model, x, t, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None, order=2,
                              eta=1.0, old_out=None, *, noise=None, philox_seed=0, sample_offset=0, rng_step=None):
        """One SDE-DPM-Solver++ multistep step (gdx_dpm_sde_step): dpm_solver_sample's x0 prediction and history protocol, then
        the update of order min(order, predictions kept + 1, t + 1) with noise.  z is `noise` if given, else the in-kernel
        Philox draw (philox_seed, sample_offset + b, rng_step) if rng_step is given, else th.empty_like(x).normal_().  t must
        be the same for the whole batch.  Returns {"sample", "pred_xstart", "old_pred"}."""
        if order not in (1, 2):
            raise ValueError('order is invalid (should be int from 1-2).')
        xc, tt, i = self._uniform_t("dpm_solver_sde_sample", x, t)
        coef = self.dpm_sde_coef_table(xc.device, eta)
        pred = self._pred_xstart(model, xc, tt, clip_denoised, denoised_fn, model_kwargs)
        used = self._condition_score_xstart(cond_fn, xc, tt, pred, model_kwargs or {})
        if noise is not None:
            noise = E.f32c(noise, "noise")
            assert noise.shape == xc.shape
        elif rng_step is None:
            noise = th.empty_like(xc).normal_()
        sample, old_pred = self._history_step(order, old_out, i, used, lambda cur, hist: E.dpm_sde_step(
            cur, coef, xc, used, th.empty_like(xc), hist=hist, step_index=i, noise=noise, philox_seed=philox_seed,
            sample_offset=sample_offset, rng_step=0 if rng_step is None else int(rng_step)))
        return {"sample": sample, "pred_xstart": pred, "old_pred": old_pred}

    def dpm_solver_sde_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                                   model_kwargs=None, device=None, progress=False, skip_timesteps=0, init_image=None,
                                   randomize_class=False, cond_fn_with_grad=False, order=2, eta=1.0, *, fused=True, rng="torch",
                                   philox_seed=0, sample_offset=0, noise_tape=None):
        """SDE-DPM-Solver++ multistep sampling (second order by default; eta = 1 injects the ancestral sampler's noise, eta =
        0 is dpm_solver_sample_loop): dpm_solver_sample_loop's signature and routes.  A native START_X denoiser (or its
        ClassifierFreeSampleModel) without cond_fn / denoised_fn runs inside libgdx (gdx_dpm_sde_loop: one forward and one
        fused update launch per step); every other case, and fused=False, goes step by step through dpm_solver_sde_sample.
        Noise as in p_sample_loop: a recorded noise_tape (entry 0 = x_T, entry 1 + k = step k), in-kernel Philox (draw 0 = x_T,
        draw k + 1 = step k), or torch's generator (one normal_() per step in step order).  Both routes give the same bits."""
        if rng not in ("torch", "philox"):
            raise ValueError(f"rng must be 'torch' or 'philox', got {rng!r}")
        if order not in (1, 2):
            raise ValueError('order is invalid (should be int from 1-2).')
        if not float(eta) >= 0.0:
            raise ValueError(f"eta must be >= 0, got {eta!r}")
        if cond_fn_with_grad or randomize_class:
            raise NotImplementedError("cond_fn_with_grad / randomize_class are outside the sampling hot path")
        if self._runs_fused(fused, model, denoised_fn, cond_fn):
            if model_kwargs is None:
                model_kwargs = {}
            device, img, indices = self._prepare_loop(model, shape, noise, device, skip_timesteps, init_image, rng,
                                                      philox_seed, sample_offset, noise_tape)
            return self._fused_dpm_sde_loop(model, img, indices, model_kwargs, int(order), float(eta), progress, clip_denoised,
                                            rng, philox_seed, sample_offset, noise_tape)
        return self._final_sample(self.dpm_solver_sde_sample_loop_progressive(
            model, shape, noise=noise, clip_denoised=clip_denoised, denoised_fn=denoised_fn, cond_fn=cond_fn,
            model_kwargs=model_kwargs, device=device, progress=progress, skip_timesteps=skip_timesteps, init_image=init_image,
            order=order, eta=eta, rng=rng, philox_seed=philox_seed, sample_offset=sample_offset, noise_tape=noise_tape))

    def _fused_dpm_sde_loop(self, model, img, indices, model_kwargs, order, eta, progress, clip_denoised, rng, philox_seed,
                            sample_offset, noise_tape):
        """Whole loop inside libgdx (gdx_dpm_sde_loop).  The history of x0 predictions lives in a tensor of this call.  Noise: a
        recorded tape, in-kernel Philox, or torch's generator, exactly as in _fused_loop (_step_noise); issued block by block
        (_issue_blocks)."""
        x, eng, mode, scale, mask, motion = self._fused_setup(model, img, model_kwargs)
        n = len(indices)
        tape = E.f32c(noise_tape[1:1 + n], "noise_tape") if noise_tape is not None else None
        coef, tmap = self.dpm_sde_coef_table(x.device, eta), self._timestep_map()
        hist = th.empty((order, *x.shape), device=x.device, dtype=th.float32) if order > 1 else None
        block, tape_of = self._step_noise(tape, rng, n, x)
        self._issue_blocks(n, x.device, progress, lambda k, nb: eng.dpm_sde_loop(
            x, mode, order, coef, tmap, indices[k], hist, scale=scale, inpaint_mask=mask, inpaint_motion=motion,
            clip_denoised=clip_denoised, run_steps=nb, k_base=k, noise_tape=tape_of(k, nb), philox_seed=philox_seed,
            sample_offset=sample_offset), block)
        return x

    def dpm_solver_sde_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None,
                                               cond_fn=None, model_kwargs=None, device=None, progress=False, skip_timesteps=0,
                                               init_image=None, randomize_class=False, cond_fn_with_grad=False, order=2,
                                               eta=1.0, *, rng="torch", philox_seed=0, sample_offset=0, noise_tape=None):
        if cond_fn_with_grad or randomize_class:
            raise NotImplementedError("cond_fn_with_grad / randomize_class are outside the sampling hot path")
        yield from self._stepwise(self.dpm_solver_sde_sample, model, shape, noise, device, progress, skip_timesteps, init_image,
                                  rng, philox_seed, sample_offset, noise_tape, step_noise=True, clip_denoised=clip_denoised,
                                  denoised_fn=denoised_fn, cond_fn=cond_fn, model_kwargs=model_kwargs, order=order, eta=eta)

    # ------------------------------------------------------------------ UniPC (no counterpart in the reference)
    def unipc_coef_rows(self):
        """The fp64 rows behind unipc_coef_tables -> (pred [num_timesteps, 8], corr [num_timesteps, 16]): UniPC (Zhao et al.
        2023, arXiv:2302.04867; data prediction, B(h) = expm1(-h)) collected into weights of the state and the x0 predictions.
        pred has dpm_coef_rows' layout (a, w1_0, w2_0, w2_1, w3_0, w3_1, w3_2, 0): columns 0..3 are taken from dpm_coef_rows
        itself (UniP-1 is DDIM, UniP-2 is 2M), columns 4..6 hold UniP-3.  corr row b, columns 4(q-1) .. 4(q-1)+3 = (cn, c0, c1,
        c2) of UniC-q with base b: the weights of the new prediction (made at b's target) and of m_b, m_{b+1}, m_{b+2}.
        Formulas, special rows and the order rule: include/gdx.h at gdx_unipc_step / gdx_unipc_loop."""
        n = self.num_timesteps
        ab, abp = self.alphas_cumprod, self.alphas_cumprod_prev
        lam = 0.5 * np.log(ab / (1.0 - ab))
        pred = self.dpm_coef_rows().copy()
        pred[:, 4:7] = 0.0
        corr = np.zeros((n, 16), dtype=np.float64)
        for b in range(1, n):                             # row 0: abar_p = 1, h = inf -- pred (0, 1, 0, ...), corr 0
            h = 0.5 * math.log(abp[b] / (1.0 - abp[b])) - lam[b]
            em1 = math.expm1(-h)
            k = -math.sqrt(abp[b]) * em1                  # -alpha_p*E: what every weight set sums to
            hh, g, fact, beta = -h, math.expm1(-h) / -h - 1.0, 1.0, []
            for q in (1, 2, 3):
                beta.append(g * fact / em1)
                fact *= q + 1
                g = g / hh - 1.0 / fact
            r = [(lam[b + j] - lam[b]) / h for j in (1, 2) if b + j < n]
            if len(r) == 2:                               # UniP-3: the leading 2x2 block of R against (beta_1, beta_2)
                rho = np.linalg.solve(np.array([[1.0, 1.0], r]), np.array(beta[:2]))
                w = [k * rho[j] / r[j] for j in (0, 1)]
                pred[b, 4:7] = k - w[0] - w[1], w[0], w[1]
            for q in range(1, len(r) + 2):                # UniC-q reads m_b .. m_{b+q-1}
                rq = r[:q - 1] + [1.0]
                rho = np.array([0.5]) if q == 1 else np.linalg.solve(np.array([[v ** p for v in rq] for p in range(q)]),
                                                                     np.array(beta[:q]))
                w = [k * rho[j] / rq[j] for j in range(q)]
                corr[b, 4 * (q - 1):4 * (q - 1) + q + 1] = [w[-1], k - sum(w)] + w[:-1]
        return pred, corr

    def unipc_coef_tables(self, device):
        """(coef [num_timesteps, 8], coef_c [num_timesteps, 16]) fp32, consumed by gdx_unipc_step / gdx_unipc_loop:
        unipc_coef_rows rounded once (.float(), the convention of every other table here)."""
        key = ("unipc", str(device))
        if key not in self._coef_cache:
            self._coef_cache[key] = tuple(th.from_numpy(r).float().to(device) for r in self.unipc_coef_rows())
        return self._coef_cache[key]

    def unipc_sample(self, model, x, t, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None, order=2,
                     old_out=None):
        """One UniPC step (gdx_unipc_step).  x is the denoiser's input (on the first step x_T, afterwards the previous step's
        "sample"); the x0 prediction comes from _pred_xstart (so EPSILON / PREVIOUS_X / denoised_fn work as elsewhere; cond_fn
        through condition_score).  With k = the steps made so far (old_out is None: 0) the corrector of order min(order, k) --
        none on the first step and at t = 0 -- moves old_out["base"] to the corrected state of this index, and the predictor of
        order min(order, k + 1, t + 1) takes that to the next input.  old_out["old_pred"]: oldest first, at most `order` kept.
        t must be the same for the whole batch.  Returns {"sample", "pred_xstart", "old_pred", "base"}."""
        if order not in (1, 2, 3):
            raise ValueError('order is invalid (should be int from 1-3).')
        xc, tt, i = self._uniform_t("unipc_sample", x, t)
        pred = self._pred_xstart(model, xc, tt, clip_denoised, denoised_fn, model_kwargs)
        used = self._condition_score_xstart(cond_fn, xc, tt, pred, model_kwargs or {})
        old_pred = list(old_out["old_pred"]) if old_out is not None else []
        qc = len(old_pred) if i > 0 else 0
        qp = min(order, len(old_pred) + 1, i + 1)
        coef, coef_c = self.unipc_coef_tables(xc.device)
        base = th.empty_like(xc)
        sample = E.unipc_step(qc, qp, coef, coef_c, E.f32c(old_out["base"], "base") if qc else xc, used, th.empty_like(xc), base,
                              hist=old_pred[::-1][:max(qc, qp - 1)], step_index=i)
        return {"sample": sample, "pred_xstart": pred, "old_pred": (old_pred + [used])[-order:], "base": base}

    def unipc_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                          model_kwargs=None, device=None, progress=False, skip_timesteps=0, init_image=None,
                          randomize_class=False, cond_fn_with_grad=False, order=2, *, fused=True, rng="torch",
                          philox_seed=0, sample_offset=0):
        """UniPC sampling (second order by default) with dpm_solver_sample_loop's signature and routes: one forward per step,
        whose prediction both corrects the step just made and predicts the next.  A native START_X denoiser (or its
        ClassifierFreeSampleModel) without cond_fn / denoised_fn runs the whole loop inside libgdx (gdx_unipc_loop: one forward
        and one fused launch per step); every other case, and fused=False, goes step by step through unipc_sample.  Both give
        the same bits.  Like DPM-Solver++ it gains its order only on steps spaced evenly in log-SNR ("logsnrN"), and at about
        10 steps or fewer it is no better than dpm_solver_sample_loop."""
        if rng not in ("torch", "philox"):
            raise ValueError(f"rng must be 'torch' or 'philox', got {rng!r}")
        if order not in (1, 2, 3):
            raise ValueError('order is invalid (should be int from 1-3).')
        if cond_fn_with_grad or randomize_class:
            raise NotImplementedError("cond_fn_with_grad / randomize_class are outside the sampling hot path")
        if self._runs_fused(fused, model, denoised_fn, cond_fn):
            if model_kwargs is None:
                model_kwargs = {}
            device, img, indices = self._prepare_loop(model, shape, noise, device, skip_timesteps, init_image, rng,
                                                      philox_seed, sample_offset, None)
            return self._fused_unipc_loop(model, img, indices, model_kwargs, int(order), progress, clip_denoised)
        return self._final_sample(self.unipc_sample_loop_progressive(
            model, shape, noise=noise, clip_denoised=clip_denoised, denoised_fn=denoised_fn, cond_fn=cond_fn,
            model_kwargs=model_kwargs, device=device, progress=progress, skip_timesteps=skip_timesteps, init_image=init_image,
            order=order, rng=rng, philox_seed=philox_seed, sample_offset=sample_offset))

    def _fused_unipc_loop(self, model, img, indices, model_kwargs, order, progress, clip_denoised):
        """Whole loop inside libgdx (gdx_unipc_loop).  The ring of x0 predictions (order + 1 deep) and the corrected state live
        in two tensors of this call; with `progress` the loop is issued in blocks of NOISE_BLOCK steps."""
        x, eng, mode, scale, mask, motion = self._fused_setup(model, img, model_kwargs)
        (coef, coef_c), tmap = self.unipc_coef_tables(x.device), self._timestep_map()
        hist = th.empty((order + 1, *x.shape), device=x.device, dtype=th.float32)
        base = th.empty_like(x)
        self._issue_blocks(len(indices), x.device, progress, lambda k, nb: eng.unipc_loop(
            x, mode, order, coef, coef_c, tmap, indices[k], hist, base, scale=scale, inpaint_mask=mask, inpaint_motion=motion,
            clip_denoised=clip_denoised, run_steps=nb, k_base=k))
        return x

    def unipc_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None,
                                      cond_fn=None, model_kwargs=None, device=None, progress=False, skip_timesteps=0,
                                      init_image=None, randomize_class=False, cond_fn_with_grad=False, order=2, *,
                                      rng="torch", philox_seed=0, sample_offset=0):
        if cond_fn_with_grad or randomize_class:
            raise NotImplementedError("cond_fn_with_grad / randomize_class are outside the sampling hot path")
        yield from self._stepwise(self.unipc_sample, model, shape, noise, device, progress, skip_timesteps, init_image, rng,
                                  philox_seed, sample_offset, clip_denoised=clip_denoised, denoised_fn=denoised_fn,
                                  cond_fn=cond_fn, model_kwargs=model_kwargs, order=order)


def _extract_into_tensor(arr, timesteps, broadcast_shape):
    """Kept for API parity (reference :1595-1608)."""
    res = th.from_numpy(arr).to(device=timesteps.device)[timesteps].float()
    while len(res.shape) < len(broadcast_shape):
        res = res[..., None]
    return res.expand(broadcast_shape)
