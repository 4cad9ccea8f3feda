"""Classifier-free-guidance sampling wrapper: drop-in for reference `model/cfg_sampler.py`.

The reference runs the inner model twice per step (cond, then a deep copy of `y` with
`uncond=True`) and blends `u + scale * (c - u)` (`model/cfg_sampler.py:23-28`).  Here both
passes run as ONE double batch through the HIP kernels (only the seed-pose embedding differs
between them; the MFCC conditioning feeds both, as in the reference) and the blend is a fused
kernel.  Nothing is deep-copied.

`y['guidance_interval'] = (lo, hi)` (additive) limits guidance to model timesteps lo <= t <= hi; a sample outside it gets
the conditional output itself.  `y['guidance_rescale'] = phi` (additive, 0 <= phi <= 1) rescales a guided output to the
conditional output's per-sample standard deviation and mixes it with the unscaled one by phi (include/gdx.h).
`y['guidance_refresh'] = k` (additive, int >= 1) belongs to the in-library loops, which remember the cond-uncond difference
between guided calls; this forward has no memory and raises ValueError for k > 1, and likewise for
`y['layer_cache'] = (every, keep)` with every > 1 (the deep encoder layers' change reused between calls).
For a use_text model `y['guidance_drop']` ("both" | "text" | "seed") names what the contrast pass drops, and `y['text_scale']`
([B], with `y['guidance_order']`) steers the two conditions on their own in three passes (engine.guidance_compose_of).
Every key is one entry of sampling_options.OPTIONS, the table through which this forward and the loops read them.
Perturbed-attention guidance (pag_scale, pag_layers: engine.attention_guidance_of) is read beside the table: with it this
wrapper runs three passes, model/pag_sampler.py's subclass the conditional and the perturbed pass alone.
"""
import torch.nn as nn

from .. import sampling_options
from ..engine import GDX_CFG
from .mdm import _NativeDenoiser


class ClassifierFreeSampleModel(nn.Module):
    pag_only = False               # model/pag_sampler.py: the subclass whose one contrast pass is the perturbed-attention pass

    def __init__(self, model):
        super().__init__()
        self.model = model
        assert self.pag_only or self.model.cond_mask_prob > 0, \
            'Cannot run a guided diffusion on a model that has not been trained with no conditions'
        if not isinstance(model, _NativeDenoiser):
            raise TypeError("ClassifierFreeSampleModel wraps gesturediffusion_amd MDM / MDM_Old instances")
        self.rot2xyz = self.model.rot2xyz
        self.njoints = self.model.njoints
        self.nfeats = self.model.nfeats
        self.data_rep = self.model.data_rep

    def forward(self, x, timesteps, y=None):
        m = self.model
        m._check_inputs(x, y)
        bs, njoints, nfeats, nframes = x.shape
        scale = y.get("scale") if self.pag_only else y["scale"]     # the subclass reads y['pag_scale'] instead (scale_operand)
        y_c = dict(y)
        y_c.pop("uncond", None)
        # argument validation identical to a plain forward (raises the same errors)
        if getattr(m, "_arch", None) is None:
            raise TypeError("inner model has no native engine")
        seed, mfcc = y["seed"], y["mfcc"]
        if hasattr(m, "cl_head") and nframes % 10 != 0:
            from .mdm import _window_error
            raise _window_error(nframes, 10)
        if m.data_rep != "genea_vec":
            raise NotImplementedError
        options = sampling_options.read(y, guided=True, num_layers=m.num_layers, use_text=getattr(m, "use_text", False),
                                        pag_only=self.pag_only)
        options.refuse_memory("the step-wise forward of ClassifierFreeSampleModel")
        eng = m._get_engine(x.device)
        options.apply_before_condition(eng)
        eng.prepare(bs, nframes)
        eng.set_condition(seed, mfcc, text=m._text_features(y, bs))
        # the interval is a per-sample choice in the blend kernel: guided where lo <= timesteps[b] <= hi, else the conditional output
        options.apply_after_condition(eng)
        out = eng.forward(x, timesteps, GDX_CFG, options.scale_operand(scale))
        return out.view(bs, njoints, nfeats, nframes)
