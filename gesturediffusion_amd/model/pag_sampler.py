"""Perturbed-attention guidance sampling wrapper (PAG; Ahn et al. 2024, arXiv:2403.17377; no counterpart in the reference).

The contrast pass is the conditional forward itself with the self-attention map of a few encoder layers replaced by the identity
(every token attends to itself alone); the guided prediction is F + w (F - P).  Nothing is dropped, so the model needs no
condition dropout at training time: `cond_mask_prob` may be 0.  Both passes run as ONE double batch through the HIP kernels; in
the perturbed layers the rows of P skip QK^T, the softmax and PV for a copy of V (include/gdx.h, gdx_set_attention_guidance).

`y['pag_scale']` (required): w, a floating device tensor [batch].  `y['pag_layers']`: the perturbed encoder layers, distinct
Python ints (default: the middle layer).  The keys of classifier-free guidance (scale, guidance_drop, text_scale,
guidance_order) are a ValueError here; to stack both, wrap the model in ClassifierFreeSampleModel and give it y['scale'] and
y['pag_scale'] (three passes).  guidance_interval, guidance_rescale, guidance_refresh and layer_cache apply as they do to
classifier-free guidance, with the perturbed pass in the unconditional pass's place.
"""
from .cfg_sampler import ClassifierFreeSampleModel


class PerturbedAttentionSampleModel(ClassifierFreeSampleModel):
    """A ClassifierFreeSampleModel in every route (isinstance), whose guided call is GDX_PAG_ONLY: row groups (F, P) under the
    scale operand fl32(1 + pag_scale), so that the library's blend P + s (F - P) reads F + w (F - P)."""
    pag_only = True
