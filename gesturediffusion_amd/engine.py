"""Thin PyTorch-ROCm <-> libgdx.so glue: PyTorch supplies device memory and the stream,
the C ABI (include/gdx.h) does all the arithmetic.  No torch compute happens here."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import GDX_ARCH_MDM, GDX_ARCH_MDM_OLD, GDX_CFG, GDX_COND, GDX_UNCOND, GdxError  # noqa: F401

MFCC_DIM = 26


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _p(t):
    """A tensor's address for a ctypes pointer field; None (NULL) for an absent operand."""
    return t.data_ptr() if t is not None else None


def _bpd_chunks(per_sample):
    """Chunks of GDX_BPD_CHUNK elements per sample: the unit the chunked sums' workspaces are sized in (include/gdx.h)."""
    return (per_sample + _lib.GDX_BPD_CHUNK - 1) // _lib.GDX_BPD_CHUNK


def _loop_fields(coef, timestep_map, scale, inpaint_mask, inpaint_motion, clip_denoised, run_steps, k_base):
    """The fields every in-library loop's argument struct shares, as keywords, and the host timestep map they point into
    (the caller keeps it alive while the loop is enqueued)."""
    tmap = np.ascontiguousarray(np.asarray(timestep_map, dtype=np.int64))
    return dict(num_steps=len(tmap), coef=coef.data_ptr(), timestep_map=tmap.ctypes.data, scale=_p(scale),
                inpaint_mask=_p(inpaint_mask), inpaint_motion=_p(inpaint_motion), clip_denoised=int(bool(clip_denoised)),
                run_steps=run_steps, k_base=k_base), tmap


def _step_fields(shape, coef, t, step_index, x0_cond, x0_uncond, scale, inpaint_mask, inpaint_motion, clip_denoised):
    """The fields every pose-layout step struct shares, as keywords; shape = the [B, J, F, T] of the operands."""
    B, J, F, T = shape
    return dict(batch=B, njoints=J * F, frames=T, coef=coef.data_ptr(), t=_p(t), step_index=step_index,
                x0_cond=x0_cond.data_ptr(), x0_uncond=_p(x0_uncond), scale=_p(scale), inpaint_mask=_p(inpaint_mask),
                inpaint_motion=_p(inpaint_motion), clip_denoised=int(bool(clip_denoised)))


def require_device(t, what):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what} must be a torch.Tensor")
    if t.device.type != "cuda":
        raise GdxError(f"{what} is on {t.device}: the MI355X HIP path needs device tensors "
                       f"(there is no CPU fallback in gesturediffusion_amd)")
    return t


def f32c(t, what):
    require_device(t, what)
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


# gdx.h GDX_DTYPE_*: "fp32" = exact fp32 MFMA everywhere (default); "fp16" / "bf16" = 16-bit GEMM / attention operands and
# activation stream, fp32 accumulate (bf16: fp32's exponent range, 8 significant bits)
COMPUTE_DTYPES = {"fp32": _lib.GDX_DTYPE_F32, "fp16": _lib.GDX_DTYPE_F16, "bf16": _lib.GDX_DTYPE_BF16}


def check_condition_entry(text_dim, have_text):
    """The refusals of the two conditioning entries (gdx.h), made before anything touches the device: a handle with text_dim > 0
    is conditioned by gdx_set_condition_text, one without by gdx_set_condition."""
    if text_dim > 0 and not have_text:
        raise GdxError("gdx_set_condition: this handle has text_dim > 0: call gdx_set_condition_text "
                       "(Engine.set_condition(seed, mfcc, text=...))")
    if text_dim <= 0 and have_text:
        raise GdxError("gdx_set_condition_text: this handle has no text (text_dim = 0): call gdx_set_condition "
                       "(Engine.set_condition(seed, mfcc))")


class Engine:
    """One libgdx handle = one model instance on one device/stream."""

    def __init__(self, arch, njoints, latent_dim, ff_size, num_layers, num_heads, seed_poses, cl_head=8, window=10,
                 compute_dtype="fp32", text_dim=0, clip_dim=0):
        self.lib = _lib.load()
        if compute_dtype not in COMPUTE_DTYPES:
            raise ValueError(f"compute_dtype must be one of {sorted(COMPUTE_DTYPES)}, got {compute_dtype!r}")
        self.compute_dtype = compute_dtype
        self.cfg = _lib.Config(arch=arch, njoints=njoints, latent_dim=latent_dim, ff_size=ff_size,
                               num_layers=num_layers, num_heads=num_heads, seed_poses=seed_poses, mfcc_dim=MFCC_DIM,
                               cl_head=cl_head, window=window, compute_dtype=COMPUTE_DTYPES[compute_dtype],
                               text_dim=text_dim, clip_dim=clip_dim)
        self.handle = C.c_void_p()
        _lib.check(self.lib.gdx_create(C.byref(self.cfg), C.byref(self.handle)), self.lib)
        self.device = None
        self.shape = None          # (B, T) the workspace is sized for
        self._cond_key = None
        self._weights_key = None
        self._compose = _lib.GDX_GUIDE_JOINT   # the handle's gdx_set_guidance_compose mode
        self._attention = (_lib.GDX_PAG_OFF, 0)   # ... and its gdx_set_attention_guidance (kind, layer mask)
        self._keep = []            # tensors that must outlive enqueued work

    def __del__(self):
        try:
            if getattr(self, "handle", None) and self.handle.value:
                self.lib.gdx_destroy(self.handle)
                self.handle = C.c_void_p()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass

    def set_graph_replay(self, on):
        """hipGraph replay of the step inside sample_loop (off by default; see include/gdx.h)."""
        _lib.check(self.lib.gdx_set_graph_replay(self.handle, int(bool(on))), self.lib)

    # ------------------------------------------------------------------ weights
    def set_weight(self, name, t):
        t = f32c(t, name)
        shape = (C.c_int64 * t.dim())(*t.shape)
        _lib.check(self.lib.gdx_set_weight(self.handle, name.encode(), _ptr(t), shape, t.dim(), _stream(t.device)),
                   self.lib)
        self.device = t.device
        self._cond_key = None

    def load_tensors(self, named):
        for name, t in named.items():
            self.set_weight(name, t)
        _lib.check(self.lib.gdx_weights_ready(self.handle), self.lib)

    def export_packed(self, device):
        """The handle's packed operand layout as one bytes object (gdx_export_packed)."""
        n = C.c_int64()
        _lib.check(self.lib.gdx_packed_bytes(self.handle, C.byref(n)), self.lib)
        buf = (C.c_char * n.value)()
        _lib.check(self.lib.gdx_export_packed(self.handle, buf, n.value, _stream(device)), self.lib)
        return bytes(buf)

    def import_packed(self, blob, device):
        """Upload a blob written by export_packed; raises GdxError (handle untouched) if it was built for another
        configuration, compute dtype or shape."""
        if torch.device(device).type != "cuda":
            raise GdxError(f"packed image target is {device}: the MI355X HIP path needs a device (no CPU fallback)")
        _lib.check(self.lib.gdx_import_packed(self.handle, blob, len(blob), _stream(device)), self.lib)
        self.device = device
        self._cond_key = None

    # ------------------------------------------------------------------ shapes / conditioning
    def prepare(self, batch, frames):
        if self.shape != (batch, frames):
            _lib.check(self.lib.gdx_prepare(self.handle, batch, frames), self.lib)
            self.shape = (batch, frames)
            self._cond_key = None

    def set_condition(self, seed, mfcc, text=None, cache=True):
        """seed [B,J,1,P], mfcc [B,26,1,T], and for a handle with text_dim > 0 text [B, clip_dim] (gdx_set_condition_text).
        The step-wise callable protocol model(x, t, y=...) calls this on every
        step, so the step-invariant work is skipped when the SAME tensors come back: the key is (storage pointer,
        version counter, shape, strides, dtype) of each and the engine keeps references to the caller's own tensors while the
        key is live -- their storage can therefore not be freed and handed to a different tensor with an equal key (a view
        such as sample_out[..., -seed_poses:] shares its base's storage and version counter).  `cache=False` (the
        fused loop: one call per 1000 steps) always recomputes."""
        check_condition_entry(self.cfg.text_dim, text is not None)
        given = (seed, mfcc) if text is None else (seed, mfcc, text)
        key = tuple((t.data_ptr(), t._version, tuple(t.shape), tuple(t.stride()), t.dtype) for t in given)
        if cache and key == self._cond_key:
            return
        seed_c, mfcc_c = f32c(seed, "y['seed']"), f32c(mfcc, "y['mfcc']")
        if text is None:
            _lib.check(self.lib.gdx_set_condition(self.handle, _ptr(seed_c), _ptr(mfcc_c), _stream(seed_c.device)),
                       self.lib)
            self._keep = [seed, mfcc, seed_c, mfcc_c]
        else:
            text_c = f32c(text, "y['text_embed']")
            if tuple(text_c.shape) != (seed_c.shape[0], self.cfg.clip_dim):
                raise ValueError(f"y['text_embed'] must be [batch, clip_dim] = [{seed_c.shape[0]}, {self.cfg.clip_dim}], "
                                 f"got {list(text_c.shape)}")
            _lib.check(self.lib.gdx_set_condition_text(self.handle, _ptr(seed_c), _ptr(mfcc_c), _ptr(text_c),
                                                       _stream(seed_c.device)), self.lib)
            self._keep = [seed, mfcc, text, seed_c, mfcc_c, text_c]
        self._cond_key = key if cache else None

    def set_guidance_interval(self, interval=None):
        """(lo, hi): GDX_CFG guides only model timesteps lo <= t <= hi (gdx_set_guidance_interval); None = every timestep."""
        lo, hi = interval if interval is not None else (_lib.INT64_MIN, _lib.INT64_MAX)
        _lib.check(self.lib.gdx_set_guidance_interval(self.handle, lo, hi), self.lib)

    def set_guidance_compose(self, mode=_lib.GDX_GUIDE_JOINT, attention=(_lib.GDX_PAG_OFF, 0)):
        """Which passes a guided call contrasts (gdx_set_guidance_compose; GDX_GUIDE_*, JOINT = today's cond / uncond pair), and
        `attention` = (kind, layer mask), whether one of them is the perturbed-attention pass (set_attention_guidance).  Set
        in front of prepare / set_condition on every call, so a handle never keeps an earlier call's mode or kind; a change clears
        the conditioning (the rows depend on both), the same mode again is no call at all."""
        self.set_attention_guidance(*attention)
        if mode == self._compose:
            return
        _lib.check(self.lib.gdx_set_guidance_compose(self.handle, int(mode)), self.lib)
        self._compose = mode
        self._cond_key = None

    def set_attention_guidance(self, kind=_lib.GDX_PAG_OFF, layer_mask=0):
        """Perturbed-attention guidance (gdx_set_attention_guidance): GDX_PAG_ONLY contrasts the conditional pass with one whose
        self-attention map is the identity in the encoder layers of layer_mask (bit l = layer l), GDX_PAG_CFG adds that pass to
        the cond / uncond pair as a third; GDX_PAG_OFF = neither.  A change clears the conditioning; the same setting again is no
        call at all.  A refused call leaves handle and engine as they were."""
        if (kind, layer_mask) == self._attention:
            return
        _lib.check(self.lib.gdx_set_attention_guidance(self.handle, int(kind), int(layer_mask)), self.lib)
        self._attention = (kind, layer_mask)
        self._cond_key = None

    def set_guidance_rescale(self, phi=0.0):
        """phi in [0, 1]: guided x0 predictions are rescaled to the conditional output's per-sample standard deviation and mixed
        with the unscaled ones by phi (gdx_set_guidance_rescale); 0 = off."""
        _lib.check(self.lib.gdx_set_guidance_rescale(self.handle, float(phi)), self.lib)

    def set_guidance_refresh(self, every=1):
        """every >= 1: the in-library sampling loops run the unconditional pass on every `every`-th guided denoiser call and
        reuse the stored cond-uncond difference in between (gdx_set_guidance_refresh); 1 = off.  Clears the stored difference."""
        _lib.check(self.lib.gdx_set_guidance_refresh(self.handle, int(every)), self.lib)

    def set_layer_cache(self, every=1, keep=0):
        """every >= 1: the in-library sampling loops run every `every`-th denoiser call in full and, in between, recompute only
        the first `keep` encoder layers and add the stored change of the deeper ones (gdx_set_layer_cache); 1 = off, keep is
        then not looked at.  Clears the stored change."""
        _lib.check(self.lib.gdx_set_layer_cache(self.handle, int(every), int(keep)), self.lib)

    def set_resample(self, jump=1, repeats=1, alpha_bar=None):
        """repeats > 1: sample_loop executes the resampling walk (gdx_set_resample; the rule is in include/gdx.h) with forward hops
        of `jump` levels built from alpha_bar, the float64 alphas_cumprod of the loop's own schedule; 1 = off, alpha_bar is then
        not looked at.  The other loops refuse while it is on."""
        ab = np.ascontiguousarray(np.asarray(alpha_bar, dtype=np.float64)) if repeats > 1 and alpha_bar is not None else None
        _lib.check(self.lib.gdx_set_resample(self.handle, int(jump), int(repeats), ab.ctypes.data if ab is not None else None,
                                             len(ab) if ab is not None else 0), self.lib)

    @staticmethod
    def layer_delta(op, inp, outc, delta):
        """The stand-alone gdx_layer_delta (the module's layer_delta)."""
        return layer_delta(op, inp, outc, delta)

    def cfg_rescale(self, c, u, scale, phi, t=None, interval=None, out=None):
        """The stand-alone gdx_cfg_rescale on [B,J,1,T] device tensors -> (out, factor [B]); t (int64 [B]) with interval (lo, hi)
        marks the guided samples (None: all); out may be c itself.  Operands are taken as they are (no copies): tests hand it
        misaligned views."""
        B, J, F, T = c.shape
        dev = c.device
        if out is None:
            out = torch.empty_like(c)
        factor = torch.empty(B, device=dev, dtype=torch.float32)
        ws = torch.empty(4 * B * _bpd_chunks(J * F * T), device=dev, dtype=torch.float64)
        lo, hi = interval if interval is not None else (_lib.INT64_MIN, _lib.INT64_MAX)
        a = _lib.CfgRescaleArgs(batch=B, njoints=J * F, frames=T, x0_cond=c.data_ptr(), x0_uncond=u.data_ptr(),
                                scale=scale.data_ptr(), phi=float(phi), t=t.data_ptr() if t is not None else None, lo=lo, hi=hi,
                                workspace=ws.data_ptr(), factor=factor.data_ptr(), out=out.data_ptr())
        _lib.check(self.lib.gdx_cfg_rescale(C.byref(a), _stream(dev)), self.lib)
        return out, factor

    def forward_samples(self):
        """Samples pushed through the denoiser since the handle was created (gdx_forward_samples; host-side counter)."""
        n = C.c_int64()
        _lib.check(self.lib.gdx_forward_samples(self.handle, C.byref(n)), self.lib)
        return n.value

    def forward_layer_samples(self):
        """Samples x encoder layers launched since the handle was created (gdx_forward_layer_samples; host-side counter)."""
        n = C.c_int64()
        _lib.check(self.lib.gdx_forward_layer_samples(self.handle, C.byref(n)), self.lib)
        return n.value

    # ------------------------------------------------------------------ compute
    def forward(self, x, timesteps, mode=GDX_COND, scale=None):
        x = f32c(x, "x")
        t = require_device(timesteps, "timesteps").to(torch.int64).contiguous()
        out = torch.empty_like(x)
        sc = f32c(scale, "y['scale']") if scale is not None else None
        _lib.check(self.lib.gdx_forward(self.handle, _ptr(x), _ptr(t), mode, _ptr(sc), _ptr(out), _stream(x.device)),
                   self.lib)
        return out

    def keep_taps(self, keep=True):
        _lib.check(self.lib.gdx_set_keep_taps(self.handle, int(keep)), self.lib)
        self._cond_key = None if keep else self._cond_key

    def set_guards(self, on=True):
        """Test aid: canary zones behind every workspace buffer (gdx_set_guards)."""
        _lib.check(self.lib.gdx_set_guards(self.handle, int(bool(on))), self.lib)
        self._cond_key = None            # the workspace was re-allocated: conditioning must be set again

    def check_guards(self, device):
        bad, first = C.c_int64(), C.c_int32()
        _lib.check(self.lib.gdx_check_guards(self.handle, C.byref(bad), C.byref(first), _stream(device)), self.lib)
        return bad.value, first.value

    def tap(self, which, rows, d, device):
        """which 0 .. L: the residual stream [Beff * (T + 1), d]; L + 1: the output GEMM's operand [Beff * T, d] (gdx_get_tap)."""
        out = torch.empty(rows, d, device=device, dtype=torch.float32)
        _lib.check(self.lib.gdx_get_tap(self.handle, which, _ptr(out), out.numel(), _stream(device)), self.lib)
        return out

    def _run_loop(self, fn, args, device, *keep):
        _lib.check(fn(self.handle, C.byref(args), _stream(device)), self.lib)
        self._keep_loop = keep

    def sample_loop(self, x, kind, mode, coef, timestep_map, first_index, scale=None, inpaint_mask=None,
                    inpaint_motion=None, noise_tape=None, const_noise=False, philox_seed=0, sample_offset=0,
                    dump=None, dump_steps=None, run_steps=0, k_base=0, clip_denoised=False):
        """x is updated in place (x_T in, final sample out).  run_steps / k_base: one block of a loop (gdx.h)."""
        kw, tmap = _loop_fields(coef, timestep_map, scale, inpaint_mask, inpaint_motion, clip_denoised, run_steps, k_base)
        ds = np.ascontiguousarray(np.asarray(dump_steps if dump_steps is not None else [], dtype=np.int32))
        a = _lib.LoopArgs(kind=kind, mode=mode, first_index=first_index, x=x.data_ptr(), noise_tape=_p(noise_tape),
                          const_noise=int(const_noise), philox_seed=philox_seed, sample_offset=sample_offset, dump=_p(dump),
                          dump_steps=ds.ctypes.data if len(ds) else None, n_dump=len(ds), **kw)
        self._run_loop(self.lib.gdx_sample_loop, a, x.device, tmap, ds)

    def bpd_loop(self, x_start, mode, coef, timestep_map, vb, xstart_mse, mse, scale=None, inpaint_mask=None,
                 inpaint_motion=None, noise_tape=None, philox_seed=0, sample_offset=0, clip_denoised=True, run_steps=0,
                 k_base=0, prior_bpd=None, prior_log_variance=0.0):
        """gdx_bpd_loop: steps k_base .. of the variational bound into column k of vb / xstart_mse / mse [B, num_steps]."""
        kw, tmap = _loop_fields(coef, timestep_map, scale, inpaint_mask, inpaint_motion, clip_denoised, run_steps, k_base)
        a = _lib.BpdLoopArgs(mode=mode, x_start=x_start.data_ptr(), noise_tape=_p(noise_tape), philox_seed=philox_seed,
                             sample_offset=sample_offset, prior_log_variance=prior_log_variance, vb=vb.data_ptr(),
                             xstart_mse=xstart_mse.data_ptr(), mse=mse.data_ptr(), prior_bpd=_p(prior_bpd), **kw)
        self._run_loop(self.lib.gdx_bpd_loop, a, x_start.device, tmap)

    def plms_loop(self, x, mode, order, coef, timestep_map, first_index, eps_hist, scratch, scale=None, inpaint_mask=None,
                  inpaint_motion=None, clip_denoised=False, run_steps=0, k_base=0):
        """gdx_plms_loop: x is updated in place; eps_hist [order, B, J, 1, T] and scratch [B, J, 1, T] are the caller's and
        carry the multistep history from one block (run_steps / k_base) to the next."""
        kw, tmap = _loop_fields(coef, timestep_map, scale, inpaint_mask, inpaint_motion, clip_denoised, run_steps, k_base)
        a = _lib.PlmsLoopArgs(mode=mode, order=order, first_index=first_index, x=x.data_ptr(), eps_hist=eps_hist.data_ptr(),
                              scratch=scratch.data_ptr(), **kw)
        self._run_loop(self.lib.gdx_plms_loop, a, x.device, tmap)

    def dpm_loop(self, x, mode, order, coef, timestep_map, first_index, hist=None, scale=None, inpaint_mask=None,
                 inpaint_motion=None, clip_denoised=False, run_steps=0, k_base=0):
        """gdx_dpm_loop: x is updated in place; hist [order, B, J, 1, T] (order > 1) is the caller's and carries the x0
        predictions of the multistep history from one block (run_steps / k_base) to the next."""
        kw, tmap = _loop_fields(coef, timestep_map, scale, inpaint_mask, inpaint_motion, clip_denoised, run_steps, k_base)
        a = _lib.DpmLoopArgs(mode=mode, order=order, first_index=first_index, x=x.data_ptr(), hist=_p(hist), **kw)
        self._run_loop(self.lib.gdx_dpm_loop, a, x.device, tmap)

    def dpm_sde_loop(self, x, mode, order, coef, timestep_map, first_index, hist=None, scale=None, inpaint_mask=None,
                     inpaint_motion=None, clip_denoised=False, run_steps=0, k_base=0, noise_tape=None, philox_seed=0,
                     sample_offset=0):
        """gdx_dpm_sde_loop: dpm_loop with noise -- noise_tape [steps of this call, B, J, 1, T] (slice 0 = this call's first
        step) or, without one, Philox draw k + 1 at executed step k."""
        kw, tmap = _loop_fields(coef, timestep_map, scale, inpaint_mask, inpaint_motion, clip_denoised, run_steps, k_base)
        a = _lib.DpmSdeLoopArgs(mode=mode, order=order, first_index=first_index, x=x.data_ptr(), hist=_p(hist),
                                noise_tape=_p(noise_tape), philox_seed=philox_seed, sample_offset=sample_offset, **kw)
        self._run_loop(self.lib.gdx_dpm_sde_loop, a, x.device, tmap)

    def unipc_loop(self, x, mode, order, coef, coef_c, timestep_map, first_index, hist, base, scale=None, inpaint_mask=None,
                   inpaint_motion=None, clip_denoised=False, run_steps=0, k_base=0):
        """gdx_unipc_loop: x (the denoiser's input) is updated in place; hist [order + 1, B, J, 1, T] and base [B, J, 1, T] are
        the caller's and carry the x0 predictions and the corrected state from one block (run_steps / k_base) to the next."""
        kw, tmap = _loop_fields(coef, timestep_map, scale, inpaint_mask, inpaint_motion, clip_denoised, run_steps, k_base)
        a = _lib.UnipcLoopArgs(mode=mode, order=order, first_index=first_index, x=x.data_ptr(), hist=_p(hist), base=_p(base),
                               coef_c=coef_c.data_ptr(), **kw)
        self._run_loop(self.lib.gdx_unipc_loop, a, x.device, tmap)

    def ddim_reverse_loop(self, x, mode, coef, timestep_map, first_index, run_steps, scale=None, inpaint_mask=None,
                          inpaint_motion=None, clip_denoised=False):
        """gdx_ddim_reverse_loop: x (the state at index first_index) is updated in place to the state at first_index + run_steps;
        the indices ascend, and nothing but x is carried from one block to the next."""
        kw, tmap = _loop_fields(coef, timestep_map, scale, inpaint_mask, inpaint_motion, clip_denoised, run_steps, 0)
        # plain arguments in gdx.h's order (this entry has no argument struct, and an ascending loop no k_base)
        _lib.check(self.lib.gdx_ddim_reverse_loop(self.handle, mode, kw["num_steps"], first_index, kw["run_steps"], kw["coef"],
                                                  kw["timestep_map"], x.data_ptr(), kw["scale"], kw["inpaint_mask"],
                                                  kw["inpaint_motion"], kw["clip_denoised"], _stream(x.device)), self.lib)
        self._keep_loop = (tmap,)

    def prepare_window(self, batch, frames, window, seed, mfcc, text=None):
        """The handle of gdx_parallel_loop: prepared for window x batch samples and conditioned on seed / mfcc (and text)
        repeated window-major, row j * batch + b = sample b."""
        rep = lambda t: t.repeat(window, *([1] * (t.dim() - 1))) if t is not None else None   # noqa: E731
        self.prepare(window * batch, frames)
        self.set_condition(rep(seed), rep(mfcc), text=rep(text), cache=False)

    def parallel_loop(self, planes, kind, mode, coef, timestep_map, threshold, first_index, anchor=0, scale=None,
                      inpaint_mask=None, inpaint_motion=None, clip_denoised=False, noise_tape=None, philox_seed=0,
                      sample_offset=0, max_iterations=0):
        """gdx_parallel_loop on planes [window + 1, B, J, 1, T] (updated in place; planes[0] is the sample once the anchor has
        reached first_index + 1) -> (anchor, this call's strides).  threshold: float64 [num_steps] on the host.  The call
        synchronises the stream once per iteration (gdx.h); max_iterations > 0 issues a block and carries nothing but the planes
        and the anchor to the next."""
        kw, tmap = _loop_fields(coef, timestep_map, scale, inpaint_mask, inpaint_motion, clip_denoised, 0, 0)
        thr = np.ascontiguousarray(np.asarray(threshold, dtype=np.float64))
        if thr.shape != (len(tmap),):
            raise ValueError(f"threshold must hold one float64 per step ({len(tmap)}), got shape {thr.shape}")
        window = planes.shape[0] - 1
        cap = first_index + 1
        a, its, strides = C.c_int32(anchor), C.c_int32(0), (C.c_int32 * cap)()
        # plain arguments in gdx.h's order (this entry has no argument struct)
        _lib.check(self.lib.gdx_parallel_loop(self.handle, kind, mode, kw["num_steps"], first_index, kw["coef"], kw["timestep_map"],
                                              thr.ctypes.data, window, planes.data_ptr(), kw["scale"], kw["inpaint_mask"],
                                              kw["inpaint_motion"], kw["clip_denoised"], _p(noise_tape), philox_seed, sample_offset,
                                              C.byref(a), max_iterations, strides, cap, C.byref(its), _stream(planes.device)),
                   self.lib)
        return a.value, list(strides[:its.value])

    def forward_flops(self, mode=GDX_COND):
        f = C.c_double()
        _lib.check(self.lib.gdx_forward_flops(self.handle, mode, C.byref(f)), self.lib)
        return f.value

    def profile_begin(self, max_launches):
        _lib.check(self.lib.gdx_profile_begin(self.handle, max_launches), self.lib)

    def profile_end(self):
        us, n = C.c_float(), C.c_int32()
        _lib.check(self.lib.gdx_profile_end(self.handle, C.byref(us), C.byref(n)), self.lib)
        return us.value, n.value

    def bench_ffn_gemm(self, iters, device):
        us = C.c_float()
        _lib.check(self.lib.gdx_bench_ffn_gemm(self.handle, iters, C.byref(us), _stream(device)), self.lib)
        return us.value


def guidance_interval_of(y, guided_model):
    """y['guidance_interval'] validated -> (lo, hi) Python ints in MODEL timesteps, bounds inclusive (lo > hi: the empty
    interval), or None when the key is absent.  ValueError for anything but two ints -- a tensor is refused because reading it
    would synchronise -- and for a key on a model that is not a ClassifierFreeSampleModel (`guided_model` False)."""
    if "guidance_interval" not in y:
        return None
    iv = y["guidance_interval"]
    if not guided_model:
        raise ValueError("y['guidance_interval'] needs a ClassifierFreeSampleModel: this model runs no guidance to limit")
    ok = (isinstance(iv, (tuple, list)) and len(iv) == 2
          and all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in iv))
    if not ok:
        raise ValueError(f"y['guidance_interval'] must be two Python ints (lo, hi) in model timesteps, got {iv!r}"
                         if not isinstance(iv, torch.Tensor) else
                         "y['guidance_interval'] must be two Python ints (lo, hi), not a tensor: reading it would synchronise")
    lo, hi = int(iv[0]), int(iv[1])
    if not (_lib.INT64_MIN <= lo <= _lib.INT64_MAX and _lib.INT64_MIN <= hi <= _lib.INT64_MAX):
        raise ValueError(f"y['guidance_interval'] bounds must fit 64 bits, got {iv!r}")
    return lo, hi


GUIDANCE_DROPS = {"both": _lib.GDX_GUIDE_JOINT, "text": _lib.GDX_GUIDE_TEXT, "seed": _lib.GDX_GUIDE_SEED}
GUIDANCE_ORDERS = {"seed_text": _lib.GDX_GUIDE_SEED_TEXT, "text_seed": _lib.GDX_GUIDE_TEXT_SEED}
COMPOSE_KEYS = ("guidance_drop", "text_scale", "guidance_order")


def guidance_compose_of(y, guided_model, use_text=True):
    """y['guidance_drop'] / y['text_scale'] / y['guidance_order'] validated -> (mode, text_scale): the GDX_GUIDE_* mode of
    gdx_set_guidance_compose and the text scales, a floating device tensor [B], or None outside the 3-pass modes.  Without any
    of the keys: (GDX_GUIDE_JOINT, None).  guidance_drop names what the contrast pass drops, "both" (JOINT), "text" or "seed",
    under the one scale y['scale'].  text_scale selects a 3-pass mode, in which y['scale'] is the seed scale and guidance_order
    says which condition is stepped to first: "seed_text" (default) or "text_seed".  ValueError for a key on a model that is not a
    ClassifierFreeSampleModel (`guided_model` False) or has no use_text, for text_scale together with guidance_drop, for
    guidance_order without text_scale, and for a wrong type or shape (text_scale must match y['scale'] entry for entry)."""
    present = [k for k in COMPOSE_KEYS if k in y]
    if not present:
        return _lib.GDX_GUIDE_JOINT, None
    if not guided_model:
        raise ValueError(f"y['{present[0]}'] needs a ClassifierFreeSampleModel: this model runs no guidance to compose")
    if not use_text:
        raise ValueError(f"y['{present[0]}'] needs a use_text model: without text the seed poses are the one condition that "
                         f"can be dropped, and there is nothing to compose")
    if "text_scale" not in y:
        if "guidance_order" in y:
            raise ValueError("y['guidance_order'] needs y['text_scale']: with one scale there is one stage and no order")
        drop = y["guidance_drop"]
        if not isinstance(drop, str) or drop not in GUIDANCE_DROPS:
            raise ValueError(f"y['guidance_drop'] must be one of {sorted(GUIDANCE_DROPS)}, got {drop!r}")
        return GUIDANCE_DROPS[drop], None
    if "guidance_drop" in y:
        raise ValueError("y['text_scale'] and y['guidance_drop'] exclude each other: text_scale runs both contrast passes, "
                         "guidance_drop chooses the one that runs")
    order = y.get("guidance_order", "seed_text")
    if not isinstance(order, str) or order not in GUIDANCE_ORDERS:
        raise ValueError(f"y['guidance_order'] must be one of {sorted(GUIDANCE_ORDERS)}, got {order!r}")
    ts = y["text_scale"]
    if not isinstance(ts, torch.Tensor) or not ts.is_floating_point():
        raise ValueError(f"y['text_scale'] must be a floating tensor [batch], got {type(ts).__name__ if not isinstance(ts, torch.Tensor) else ts.dtype}")
    scale = y.get("scale")
    if ts.dim() != 1 or (isinstance(scale, torch.Tensor) and ts.numel() != scale.numel()):
        raise ValueError(f"y['text_scale'] must be [batch] like y['scale'], got {list(ts.shape)}")
    return GUIDANCE_ORDERS[order], require_device(ts, "y['text_scale']")


PAG_KEYS = ("pag_scale", "pag_layers")
PAG_OFF = (_lib.GDX_PAG_OFF, 0, None)


def attention_guidance_of(y, guided_model, num_layers, pag_only=False):
    """y['pag_scale'] / y['pag_layers'] validated -> (kind, layer_mask, pag_scale): the arguments of gdx_set_attention_guidance and
    the PAG scales w, a floating device tensor [B].  Without either key: PAG_OFF.  pag_scale turns perturbed-attention guidance on;
    pag_layers, a tuple or list of distinct Python ints in 0 .. num_layers - 1, names the encoder layers whose attention map the
    contrast pass replaces by the identity (default: the middle layer, num_layers // 2).  Under a ClassifierFreeSampleModel
    (`guided_model` True) the kind is GDX_PAG_CFG, three passes; under a PerturbedAttentionSampleModel (`pag_only`) it is
    GDX_PAG_ONLY, pag_scale is required and the keys of classifier-free guidance are refused.  ValueError for a key on a plain
    MDM / MDM_Old, for pag_layers without pag_scale, for pag_scale together with guidance_drop other than "both" or with text_scale,
    and for a wrong type, shape or layer."""
    present = [k for k in PAG_KEYS if k in y]
    if not present:
        if pag_only:
            raise ValueError("PerturbedAttentionSampleModel needs y['pag_scale'], a floating tensor [batch]: it runs no other guidance")
        return PAG_OFF
    if not guided_model:
        raise ValueError(f"y['{present[0]}'] needs a PerturbedAttentionSampleModel or a ClassifierFreeSampleModel: this model runs no "
                         f"guidance")
    if "pag_scale" not in y:
        raise ValueError("y['pag_layers'] needs y['pag_scale']: the layers say where the pass is perturbed, the scale turns it on")
    if pag_only:
        for key in ("scale", "guidance_drop", "text_scale", "guidance_order"):
            if key in y:
                raise ValueError(f"y['{key}'] belongs to classifier-free guidance, which a PerturbedAttentionSampleModel does not run: "
                                 f"wrap the model in ClassifierFreeSampleModel to stack both (y['scale'] and y['pag_scale'])")
    else:
        if y.get("guidance_drop", "both") != "both":
            raise ValueError("y['pag_scale'] and y['guidance_drop'] other than 'both' exclude each other: the perturbed pass takes the "
                             "place of the pass with one condition dropped")
        if "text_scale" in y:
            raise ValueError("y['pag_scale'] and y['text_scale'] exclude each other: each adds a third pass, and four are not supported")
    ps = y["pag_scale"]
    if not isinstance(ps, torch.Tensor) or not ps.is_floating_point():
        raise ValueError(f"y['pag_scale'] must be a floating tensor [batch], got {type(ps).__name__ if not isinstance(ps, torch.Tensor) else ps.dtype}")
    like = y.get("seed") if pag_only else y.get("scale")
    batch = (like.shape[0] if pag_only else like.numel()) if isinstance(like, torch.Tensor) else None
    if ps.dim() != 1 or (batch is not None and ps.numel() != batch):
        raise ValueError(f"y['pag_scale'] must be [batch], got {list(ps.shape)}")
    layers = y.get("pag_layers", (num_layers // 2,))
    if isinstance(layers, torch.Tensor):
        raise ValueError("y['pag_layers'] must be a tuple or list of Python ints, not a tensor: reading it would synchronise")
    ok = (isinstance(layers, (tuple, list)) and len(layers) > 0
          and all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in layers))
    if not ok:
        raise ValueError(f"y['pag_layers'] must be a non-empty tuple or list of Python ints, got {layers!r}")
    if len(set(int(v) for v in layers)) != len(layers) or not all(0 <= v < min(num_layers, 64) for v in layers):
        raise ValueError(f"y['pag_layers'] must name distinct encoder layers in 0 .. num_layers - 1 = {num_layers - 1}, got {layers!r}")
    mask = sum(1 << int(v) for v in layers)
    return (_lib.GDX_PAG_ONLY if pag_only else _lib.GDX_PAG_CFG), mask, require_device(ps, "y['pag_scale']")


def guidance_rescale_of(y, guided_model):
    """y['guidance_rescale'] validated -> phi, a Python float with 0 <= phi <= 1 (0.0 when the key is absent: off).  ValueError
    for anything but a finite Python float or int in that range -- a bool is refused, and a tensor because reading it would
    synchronise -- and for a key on a model that is not a ClassifierFreeSampleModel (`guided_model` False)."""
    if "guidance_rescale" not in y:
        return 0.0
    phi = y["guidance_rescale"]
    if not guided_model:
        raise ValueError("y['guidance_rescale'] needs a ClassifierFreeSampleModel: this model runs no guidance to rescale")
    if isinstance(phi, torch.Tensor):
        raise ValueError("y['guidance_rescale'] must be a Python float, not a tensor: reading it would synchronise")
    if isinstance(phi, bool) or not isinstance(phi, (int, float)):
        raise ValueError(f"y['guidance_rescale'] must be a Python float in [0, 1], got {phi!r}")
    if not 0 <= phi <= 1:                                    # False for NaN and the infinities too
        raise ValueError(f"y['guidance_rescale'] must be finite and satisfy 0 <= phi <= 1, got {phi!r}")
    return float(phi)


def guidance_refresh_of(y, guided_model):
    """y['guidance_refresh'] validated -> every, a Python int >= 1 (1 when the key is absent: off).  ValueError for anything but
    a Python int >= 1 -- a bool and a float are refused, and a tensor because reading it would synchronise -- and for a key on
    a model that is not a ClassifierFreeSampleModel (`guided_model` False)."""
    if "guidance_refresh" not in y:
        return 1
    if not guided_model:
        raise ValueError("y['guidance_refresh'] needs a ClassifierFreeSampleModel: this model runs no guidance to refresh")
    return guidance_refresh_value(y["guidance_refresh"])


def guidance_refresh_value(every):
    """guidance_refresh_of's rule for the value itself (GaussianDiffusion.guidance_plan takes it as an argument)."""
    if isinstance(every, torch.Tensor):
        raise ValueError("y['guidance_refresh'] must be a Python int, not a tensor: reading it would synchronise")
    if isinstance(every, bool) or not isinstance(every, (int, np.integer)):
        raise ValueError(f"y['guidance_refresh'] must be a Python int >= 1, got {every!r}")
    if not 1 <= every <= 2**31 - 1:
        raise ValueError(f"y['guidance_refresh'] must satisfy 1 <= every < 2**31, got {every!r}")
    return int(every)


def layer_cache_of(y, num_layers):
    """y['layer_cache'] validated -> (every, keep), two Python ints ((1, 0) when the key is absent: off).  ValueError for anything
    but two Python ints -- a bool and a float are refused, and a tensor because reading it would synchronise --, for every < 1,
    and, when every > 1, for keep outside 1 .. num_layers - 1.  At every = 1 keep is not looked at.  Needs no
    ClassifierFreeSampleModel: the cache sits inside the denoiser."""
    return layer_cache_value(y["layer_cache"], num_layers) if "layer_cache" in y else (1, 0)


def layer_cache_value(lc, num_layers):
    """layer_cache_of's rule for the value itself (GaussianDiffusion.layer_cache_plan takes it as an argument)."""
    if isinstance(lc, torch.Tensor) or (isinstance(lc, (tuple, list)) and any(isinstance(v, torch.Tensor) for v in lc)):
        raise ValueError("y['layer_cache'] must be two Python ints (every, keep), not a tensor: reading it would synchronise")
    ok = (isinstance(lc, (tuple, list)) and len(lc) == 2
          and all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in lc))
    if not ok:
        raise ValueError(f"y['layer_cache'] must be two Python ints (every, keep), got {lc!r}")
    every, keep = int(lc[0]), int(lc[1])
    if not 1 <= every <= 2**31 - 1:
        raise ValueError(f"y['layer_cache'] must satisfy 1 <= every < 2**31, got {lc!r}")
    if every == 1:
        return 1, 0
    if not 1 <= keep <= num_layers - 1:
        raise ValueError(f"y['layer_cache'] must satisfy 1 <= keep <= num_layers - 1 = {num_layers - 1}, got {lc!r}")
    return every, keep


# ---------------------------------------------------------------------- standalone kernels
def cfg_delta(a, b, out=None, count=None):
    """The stand-alone gdx_cfg_delta: out = a - b (fp32) over the first `count` elements (default: all of a) of device tensors
    taken as they are (no copies: tests hand it misaligned views); out may be b itself."""
    lib = _lib.load()
    if out is None:
        out = torch.empty_like(a)
    args = _lib.CfgDeltaArgs(count=a.numel() if count is None else count, a=a.data_ptr(), b=b.data_ptr(), out=out.data_ptr())
    _lib.check(lib.gdx_cfg_delta(C.byref(args), _stream(a.device)), lib)
    return out


def attention_identity(qkv, ctx):
    """The stand-alone gdx_attention_identity on device tensors taken as they are (no copies: tests hand it misaligned views):
    qkv [rows, 3 * d] -> ctx [rows, d] = the V third, a bit copy in the tensors' element size.  Synchronous with the device."""
    lib = _lib.load()
    rows, d = ctx.shape
    _lib.check(lib.gdx_attention_identity(ctx.element_size(), rows, d, qkv.data_ptr(), ctx.data_ptr()), lib)
    return ctx


def layer_delta(op, inp, outc, delta):
    """The stand-alone gdx_layer_delta on device tensors taken as they are (no copies: tests hand it misaligned views): inp
    [B, T + 1, d], outc [B, T, d], delta [B, T, d] fp32.  op 0 (store): delta = outc - inp[:, 1:]; op 1 (apply): outc = inp[:, 1:]
    + delta.  The element types of (inp, outc) select the pairing; the library refuses any but its three."""
    lib = _lib.load()
    code = {torch.float32: _lib.GDX_DTYPE_F32, torch.float16: _lib.GDX_DTYPE_F16, torch.bfloat16: _lib.GDX_DTYPE_BF16}
    B, T, d = outc.shape
    _lib.check(lib.gdx_layer_delta(int(op), code[inp.dtype], code[outc.dtype], B, T, d, inp.data_ptr(), outc.data_ptr(),
                                   delta.data_ptr(), _stream(outc.device)), lib)
    return delta if op == 0 else outc


def sampler_update(kind, coef, x, x0_cond, out, t=None, step_index=0, x0_uncond=None, scale=None, inpaint_mask=None,
                   inpaint_motion=None, noise=None, const_noise=False, philox_seed=0, sample_offset=0, rng_step=0,
                   pred_xstart=None, cond_grad=None, cond_coef=None, clip_denoised=False):
    lib = _lib.load()
    kw = _step_fields(x.shape, coef, t, step_index, x0_cond, x0_uncond, scale, inpaint_mask, inpaint_motion, clip_denoised)
    a = _lib.UpdateArgs(kind=kind, x=x.data_ptr(), noise=_p(noise), const_noise=int(const_noise), philox_seed=philox_seed,
                        sample_offset=sample_offset, rng_step=rng_step, out=out.data_ptr(), pred_xstart=_p(pred_xstart),
                        cond_grad=_p(cond_grad), cond_coef=_p(cond_coef), **kw)
    _lib.check(lib.gdx_sampler_update(C.byref(a), _stream(x.device)), lib)
    return out


def bpd_workspace(batch, per_sample, device):
    """Chunk-sum scratch of gdx_bpd_terms (include/gdx.h): 4 floats per (sample, GDX_BPD_CHUNK-element chunk)."""
    return torch.empty(max(1, 4 * batch * _bpd_chunks(per_sample)), device=device, dtype=torch.float32)


def bpd_terms(coef, x_start, x_t, x0_cond, noise=None, t=None, step_index=0, x0_uncond=None, scale=None, inpaint_mask=None,
              inpaint_motion=None, model_mean=None, clip_denoised=True, want_pred=True, want_mse=True):
    """gdx_bpd_terms on [B,J,1,T] tensors -> (vb [B], xstart_mse [B], mse [B] or None, pred_xstart or None)."""
    lib = _lib.load()
    B, J, F, T = x_start.shape
    dev = x_start.device
    out = torch.empty(3, B, device=dev, dtype=torch.float32)
    pred = torch.empty_like(x_start) if want_pred else None
    ws = bpd_workspace(B, J * F * T, dev)
    want_mse = want_mse and noise is not None
    kw = _step_fields(x_start.shape, coef, t, step_index, x0_cond, x0_uncond, scale, inpaint_mask, inpaint_motion, clip_denoised)
    a = _lib.BpdArgs(x_start=x_start.data_ptr(), x_t=x_t.data_ptr(), noise=_p(noise), model_mean=_p(model_mean), prior=0,
                     prior_log_variance=0.0, vb=out[0].data_ptr(), xstart_mse=out[1].data_ptr(),
                     mse=out[2].data_ptr() if want_mse else None, ld=1, col=0, pred_xstart=_p(pred), workspace=ws.data_ptr(), **kw)
    _lib.check(lib.gdx_bpd_terms(C.byref(a), _stream(dev)), lib)
    return out[0], out[1], (out[2] if want_mse else None), pred


def bpd_prior(coef, x_start, step_index, prior_log_variance):
    """The prior term of the bound (gdx_bpd_terms, prior mode) -> [B]."""
    lib = _lib.load()
    B, J, F, T = x_start.shape
    out = torch.empty(B, device=x_start.device, dtype=torch.float32)
    ws = bpd_workspace(B, J * F * T, x_start.device)
    a = _lib.BpdArgs(batch=B, njoints=J * F, frames=T, step_index=step_index, coef=coef.data_ptr(),
                     x_start=x_start.data_ptr(), prior=1, prior_log_variance=prior_log_variance, vb=out.data_ptr(), ld=1,
                     col=0, workspace=ws.data_ptr())
    _lib.check(lib.gdx_bpd_terms(C.byref(a), _stream(x_start.device)), lib)
    return out


def plms_update(kind, coef, t, x, pred_xstart, eps=(), out=None):
    """gdx_plms_update: kind 0 eps, 6 Euler predictor, 1..4 Adams-Bashforth, 5 Euler corrector (include/gdx.h)."""
    lib = _lib.load()
    ref = pred_xstart
    if out is None:
        out = torch.empty_like(ref)
    a = _lib.PlmsArgs(kind=kind, batch=ref.shape[0], per_sample=ref.numel() // ref.shape[0], coef=coef.data_ptr(),
                      t=t.data_ptr(), step_index=0, x=x.data_ptr() if x is not None else None,
                      pred_xstart=pred_xstart.data_ptr(), out=out.data_ptr())
    for i, e in enumerate(eps):
        a.eps[i] = e.data_ptr()
    _lib.check(lib.gdx_plms_update(C.byref(a), _stream(ref.device)), lib)
    return out


def plms_step(kind, coef, x, x0_cond, out, eps_out=None, eps_hist=(), t=None, step_index=0, x0_uncond=None, scale=None,
              inpaint_mask=None, inpaint_motion=None, clip_denoised=False, pred_xstart=None, x_eps=None, t_eps=None,
              step_index_eps=0, pred_prev=None):
    """gdx_plms_step: one whole PLMS step in one pass (include/gdx.h).  kind 1..4 Adams-Bashforth over the eps formed here
    and eps_hist (older, newest first), 5 the first step's corrector (x_eps / t_eps / pred_prev), 6 its predictor."""
    lib = _lib.load()
    kw = _step_fields(x0_cond.shape, coef, t, step_index, x0_cond, x0_uncond, scale, inpaint_mask, inpaint_motion, clip_denoised)
    a = _lib.PlmsStepArgs(kind=kind, t_eps=_p(t_eps), step_index_eps=step_index_eps, x=x.data_ptr(), x_eps=_p(x_eps),
                          pred_prev=_p(pred_prev), eps_out=_p(eps_out), out=out.data_ptr(), pred_xstart=_p(pred_xstart), **kw)
    for i, e in enumerate(eps_hist):
        a.eps_hist[i] = e.data_ptr()
    _lib.check(lib.gdx_plms_step(C.byref(a), _stream(x0_cond.device)), lib)
    return out


def dpm_step(order, coef, x, x0_cond, out, hist=(), t=None, step_index=0, x0_uncond=None, scale=None, inpaint_mask=None,
             inpaint_motion=None, clip_denoised=False, pred_out=None):
    """gdx_dpm_step: one DPM-Solver++ multistep step in one pass (include/gdx.h).  order 1..3 over the x0 prediction formed
    here and hist (older predictions, newest first; order - 1 of them are read); coef = dpm_coef_table rows."""
    lib = _lib.load()
    kw = _step_fields(x0_cond.shape, coef, t, step_index, x0_cond, x0_uncond, scale, inpaint_mask, inpaint_motion, clip_denoised)
    a = _lib.DpmStepArgs(order=order, x=x.data_ptr(), out=out.data_ptr(), pred_out=_p(pred_out), **kw)
    for i, m in enumerate(hist):
        a.hist[i] = _p(m)
    _lib.check(lib.gdx_dpm_step(C.byref(a), _stream(x0_cond.device)), lib)
    return out


def dpm_sde_step(order, coef, x, x0_cond, out, hist=(), t=None, step_index=0, x0_uncond=None, scale=None, inpaint_mask=None,
                 inpaint_motion=None, clip_denoised=False, pred_out=None, noise=None, philox_seed=0, sample_offset=0, rng_step=0):
    """gdx_dpm_sde_step: one SDE-DPM-Solver++ multistep step in one pass (include/gdx.h).  order 1..2 over the x0 prediction
    formed here and hist (the previous prediction, read at order 2); coef = dpm_sde_coef_table rows of one eta; z = noise, or
    the in-kernel Philox draw (philox_seed, sample_offset + b, rng_step) when noise is None."""
    lib = _lib.load()
    kw = _step_fields(x0_cond.shape, coef, t, step_index, x0_cond, x0_uncond, scale, inpaint_mask, inpaint_motion, clip_denoised)
    a = _lib.DpmSdeStepArgs(order=order, x=x.data_ptr(), out=out.data_ptr(), pred_out=_p(pred_out), noise=_p(noise),
                            philox_seed=philox_seed, sample_offset=sample_offset, rng_step=rng_step, **kw)
    for i, m in enumerate(hist):
        a.hist[i] = _p(m)
    _lib.check(lib.gdx_dpm_sde_step(C.byref(a), _stream(x0_cond.device)), lib)
    return out


def unipc_step(corr_order, pred_order, coef, coef_c, x, x0_cond, out, base_out, hist=(), t=None, step_index=0, x0_uncond=None,
               scale=None, inpaint_mask=None, inpaint_motion=None, clip_denoised=False, pred_out=None):
    """gdx_unipc_step: one UniPC step in one pass (include/gdx.h) -- the corrector of order corr_order (0: none) on the base
    state x with the x0 prediction formed here as the new one, then the predictor of order pred_order from the corrected state
    (-> base_out) into out.  hist: older predictions, newest first; coef / coef_c = unipc_coef_tables."""
    lib = _lib.load()
    kw = _step_fields(x0_cond.shape, coef, t, step_index, x0_cond, x0_uncond, scale, inpaint_mask, inpaint_motion, clip_denoised)
    a = _lib.UnipcStepArgs(corr_order=corr_order, pred_order=pred_order, coef_c=_p(coef_c), x=x.data_ptr(),
                           base_out=base_out.data_ptr(), out=out.data_ptr(), pred_out=_p(pred_out), **kw)
    for i, m in enumerate(hist):
        a.hist[i] = _p(m)
    _lib.check(lib.gdx_unipc_step(C.byref(a), _stream(x0_cond.device)), lib)
    return out


def ddim_reverse_step(coef, x, x0_cond, out, t=None, step_index=0, x0_uncond=None, scale=None, inpaint_mask=None,
                      inpaint_motion=None, clip_denoised=False, pred_out=None, eps_out=None):
    """gdx_ddim_reverse_step: one DDIM reverse-ODE step x_i -> x_{i+1} in one pass (include/gdx.h); coef = the rows of
    coef_table(GDX_SAMPLER_DDIM, device, "reverse").  out may be x; pred_out / eps_out receive the x0 prediction and eps."""
    lib = _lib.load()
    kw = _step_fields(x0_cond.shape, coef, t, step_index, x0_cond, x0_uncond, scale, inpaint_mask, inpaint_motion, clip_denoised)
    # plain arguments in gdx.h's order (this entry has no argument struct)
    _lib.check(lib.gdx_ddim_reverse_step(kw["batch"], kw["njoints"], kw["frames"], kw["coef"], kw["t"], kw["step_index"], x.data_ptr(),
                                         kw["x0_cond"], kw["x0_uncond"], kw["scale"], kw["inpaint_mask"], kw["inpaint_motion"],
                                         kw["clip_denoised"], out.data_ptr(), _p(pred_out), _p(eps_out), _stream(x0_cond.device)), lib)
    return out


def window_sweep(kind, coef, first_index, planes, x0, n_slots=None, inpaint_mask=None, inpaint_motion=None, clip_denoised=False,
                 noise=None, philox_seed=0, sample_offset=0, rng_step=1):
    """gdx_window_sweep: the update chain over planes [>= n + 1, B, J, 1, T] (in place; plane 0 is only read) with the predictions
    x0 [>= n, B, J, 1, T] held fixed, slot j at index first_index - j with noise[j] or Philox draw rng_step + j (include/gdx.h)
    -> err, float64 [n, B]: each slot's mean squared change per sample.  n_slots: n (default: every slot of x0).  Operands are taken
    as they are (no copies: tests hand it misaligned views)."""
    lib = _lib.load()
    n = x0.shape[0] if n_slots is None else n_slots
    _, B, J, F, T = planes.shape
    err = torch.empty(max(n, 1), B, device=planes.device, dtype=torch.float64)
    ws = torch.empty(max(n, 1) * B * _bpd_chunks(J * F * T), device=planes.device, dtype=torch.float64)
    # plain arguments in gdx.h's order (this entry has no argument struct)
    _lib.check(lib.gdx_window_sweep(kind, B, J * F, T, n, coef.data_ptr(), first_index, planes.data_ptr(), x0.data_ptr(),
                                    _p(inpaint_mask), _p(inpaint_motion), int(bool(clip_denoised)), _p(noise), philox_seed,
                                    sample_offset, rng_step, err.data_ptr(), ws.data_ptr(), _stream(planes.device)), lib)
    return err


def postprocess(sample, mean, std):
    """inv_transform + position / rotation split of a generated chunk on the device (reference
    sample/generate.py:132-146): sample [B, 6*nj, 1, T] -> (positions, rotations), each [B, nj, 3, T]."""
    lib = _lib.load()
    x = f32c(sample, "sample")
    B, J, F, T = x.shape
    if F != 1 or J % 6:
        raise ValueError(f"expected [B, 6*n_joints, 1, T], got {tuple(x.shape)}")
    mean = torch.as_tensor(mean, dtype=torch.float64, device=x.device).contiguous()
    std = torch.as_tensor(std, dtype=torch.float64, device=x.device).contiguous()
    if mean.numel() != J or std.numel() != J:
        raise ValueError("mean / std must have one entry per feature")
    pos = torch.empty(B, J // 6, 3, T, device=x.device, dtype=torch.float32)
    rot = torch.empty_like(pos)
    _lib.check(lib.gdx_postprocess(_ptr(x), _ptr(mean), _ptr(std), _ptr(pos), _ptr(rot), B, J // 6, T, _stream(x.device)), lib)
    return pos, rot


def q_sample(x_start, noise, coef, idx):
    lib = _lib.load()
    out = torch.empty_like(x_start)
    _lib.check(lib.gdx_q_sample(_ptr(x_start), _ptr(noise), _ptr(coef), idx, x_start.numel(), _ptr(out),
                                _stream(x_start.device)), lib)
    return out


def q_sample_t(x_start, noise, coef, t):
    """q_sample with per-sample timesteps (int64 [B] on the device)."""
    lib = _lib.load()
    out = torch.empty_like(x_start)
    B = x_start.shape[0]
    _lib.check(lib.gdx_q_sample_t(_ptr(x_start), _ptr(noise), _ptr(coef), _ptr(t), B, x_start.numel() // B, _ptr(out),
                                  _stream(x_start.device)), lib)
    return out


def masked_l2(a, b, mask):
    """Per-sample masked mean squared error (reference masked_l2); mask bool [B,1,1,T]."""
    lib = _lib.load()
    B, J, F, T = a.shape
    m = require_device(mask, "mask").to(torch.bool).reshape(B, T).contiguous()
    out = torch.empty(B, device=a.device, dtype=torch.float32)
    _lib.check(lib.gdx_masked_l2(_ptr(a), _ptr(b), _ptr(m), _ptr(out), B, J * F, T, _stream(a.device)), lib)
    return out


def randn(shape, device, philox_seed, sample_offset=0, rng_step=0):
    lib = _lib.load()
    out = torch.empty(shape, device=device, dtype=torch.float32)
    per = out.numel() // shape[0]
    _lib.check(lib.gdx_randn(_ptr(out), shape[0], per, philox_seed, sample_offset, rng_step, _stream(out.device)), lib)
    return out
