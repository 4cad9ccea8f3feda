"""The sampling options a caller puts into `y`, read once: one table (OPTIONS), one record of validated values (read), one
refusal for the paths that cannot serve an option, one place that calls the handle's setters.  A new `y` option is one entry in
OPTIONS (and one in KWARG_TO_Y for sample_chunks); every path that reads `y` picks it up.  The `*_of` validators in engine.py
stay the single statement of each key's type rule."""
from collections import namedtuple

import torch

from . import _lib
from . import engine as E

# keys: the option's y keys.  validate(y, guided, num_layers, use_text) -> value, under read()'s model-kind arguments.  off: the
# value of absent keys.  guided: the keys need a ClassifierFreeSampleModel.  memory: None, or (every_of(value), what a call would
# have to carry to the next): at every > 1 the option needs memory across denoiser calls, which only the in-library loops have.
# setter(eng, value): the Engine setter it feeds, set on every call so that a handle never keeps an earlier call's value.
# before: the setter goes in front of prepare / set_condition (the conditioning rows depend on it), else behind them.
# The order is the one in which errors are reported and, among the setters behind the conditioning, the one they are called in.
Option = namedtuple("Option", "name keys validate off guided memory setter before")
OPTIONS = (
    Option("interval", ("guidance_interval",), lambda y, guided, L, text: E.guidance_interval_of(y, guided), None, True, None,
           lambda eng, v: eng.set_guidance_interval(v), False),
    Option("rescale", ("guidance_rescale",), lambda y, guided, L, text: E.guidance_rescale_of(y, guided), 0.0, True, None,
           lambda eng, v: eng.set_guidance_rescale(v), False),
    Option("compose", E.COMPOSE_KEYS, lambda y, guided, L, text: E.guidance_compose_of(y, guided, text),
           (_lib.GDX_GUIDE_JOINT, None), True, None,
           lambda eng, v, attention=E.PAG_OFF[:2]: eng.set_guidance_compose(v[0], attention=attention), True),
    Option("refresh", ("guidance_refresh",), lambda y, guided, L, text: E.guidance_refresh_of(y, guided), 1, True,
           (lambda v: v, "the guidance difference"), lambda eng, v: eng.set_guidance_refresh(v), False),
    Option("layer_cache", ("layer_cache",), lambda y, guided, L, text: E.layer_cache_of(y, L), (1, 0), False,
           (lambda v: v[0], "the deep layers' change"), lambda eng, v: eng.set_layer_cache(*v), False),
)
KEYS = frozenset(k for o in OPTIONS for k in o.keys)
OFF = {o.name: o.off for o in OPTIONS}
BEFORE, AFTER = tuple(o for o in OPTIONS if o.before), tuple(o for o in OPTIONS if not o.before)
MEMORY = tuple(o for o in OPTIONS if o.memory)                       # what _refuse_refresh looks at
AFTER_WITHOUT_MEMORY = tuple(o for o in AFTER if not o.memory)
PLAIN_FORWARD = tuple(o for o in OPTIONS if o.name != "refresh")    # MDM / MDM_Old.forward never looked at y['guidance_refresh']


# Perturbed-attention guidance, y['pag_scale'] / y['pag_layers'], is read beside the table: what the keys mean depends on the
# wrapper (ClassifierFreeSampleModel: a third pass; PerturbedAttentionSampleModel: the only contrast, `pag_only`), which the
# table's validators are not told, and its setting travels with the compose mode's setter call (Engine.set_guidance_compose), the
# other half of "which passes a guided call runs".  A reader of a part of the table (`options`) reads it too unless the part is
# MEMORY: the plain forwards refuse the keys like every other key of a guided model.
ATTENTION_KEYS = frozenset(E.PAG_KEYS)


def read(y, *, guided, num_layers, use_text, options=OPTIONS, pag_only=False):
    """`options` of y validated, in the table's order -> Record.  guided: the model is a ClassifierFreeSampleModel; num_layers,
    use_text: its denoiser's; pag_only: it is a PerturbedAttentionSampleModel.  ValueError as the validators raise it; nothing is
    read from the device.  A y without any of the keys, the usual one of a step-wise loop's thousand calls, is every option "off"
    without a validator call."""
    values = OFF if KEYS.isdisjoint(y) else {o.name: o.validate(y, guided, num_layers, use_text) for o in options}
    attention = E.PAG_OFF
    if options is not MEMORY and (pag_only or not ATTENTION_KEYS.isdisjoint(y)):
        attention = E.attention_guidance_of(y, guided, num_layers, pag_only)
    return Record(values, attention)


class Record:
    """values: option name -> validated value (interval (lo, hi) or None, rescale phi, compose (mode, text_scale), refresh
    every, layer_cache (every, keep)) of the options that were read; never written to."""
    after = AFTER                                  # the options apply_after_condition sets

    def __init__(self, values, attention=E.PAG_OFF):
        self.values = values
        self.attention = attention                 # (kind, layer mask, pag_scale) of engine.attention_guidance_of

    def refuse_memory(self, who):
        """For `who`, a path that makes every denoiser call on its own: ValueError for an option that needs memory across calls.
        Such a path then leaves the handle's memory settings alone; the in-library loops set them at their start."""
        for o in MEMORY:
            if o.name in self.values and o.memory[0](self.values[o.name]) > 1:
                raise ValueError(f"y['{o.keys[0]}'] = {self.values[o.name]} needs the in-library loop (p_sample_loop, "
                                 f"ddim_sample_loop, plms_sample_loop, dpm_solver_sample_loop, dpm_solver_sde_sample_loop or "
                                 f"unipc_sample_loop with fused=True on a native model, without cond_fn / denoised_fn): {who} cannot "
                                 f"carry {o.memory[1]} from one call to the next")
        self.after = AFTER_WITHOUT_MEMORY

    def refuse_conflicts(self, parallel=False):
        """A 3-pass mode runs three row groups; the guidance refresh and the layer cache are written for two, and the window of
        parallel_sample_loop (`parallel`) repeats one scale per slot (gdx.h)."""
        if self.attention[0] == _lib.GDX_PAG_CFG:
            if parallel:
                raise ValueError("y['pag_scale'] with y['scale'] (3-pass guidance) is not supported by parallel_sample_loop, whose "
                                 "window repeats one scale per slot: use a PerturbedAttentionSampleModel")
            if self.values["refresh"] > 1:
                raise ValueError("y['pag_scale'] with y['scale'] (3-pass guidance) and y['guidance_refresh'] > 1 exclude each other: "
                                 "the refresh stores one cond-uncond difference")
            if self.values["layer_cache"][0] > 1:
                raise ValueError("y['pag_scale'] with y['scale'] (3-pass guidance) and y['layer_cache'] with every > 1 exclude each "
                                 "other: the cache holds two row groups")
        if self.values["compose"][0] < _lib.GDX_GUIDE_SEED_TEXT:
            return
        if parallel:
            raise ValueError("y['text_scale'] (3-pass guidance) is not supported by parallel_sample_loop, whose window repeats one "
                             "scale per slot: use y['guidance_drop']")
        if self.values["refresh"] > 1:
            raise ValueError("y['text_scale'] (3-pass guidance) and y['guidance_refresh'] > 1 exclude each other: the refresh stores "
                             "one cond-uncond difference")
        if self.values["layer_cache"][0] > 1:
            raise ValueError("y['text_scale'] (3-pass guidance) and y['layer_cache'] with every > 1 exclude each other: the cache "
                             "holds two row groups")

    def apply_before_condition(self, eng):
        """In front of prepare / set_condition, for a record of all OPTIONS; absent keys set JOINT and no perturbed pass."""
        for o in BEFORE:
            o.setter(eng, self.values[o.name], attention=self.attention[:2])

    def apply_after_condition(self, eng):
        """Behind set_condition; absent keys set "off" (every timestep, phi 0, every 1), so a reused handle is reset."""
        for o in self.after:
            o.setter(eng, self.values[o.name])

    def scale_operand(self, scale):
        """The `scale` operand of a guided call: y['scale'] flattened [B], or in a 3-pass mode [2, B] in stage order -- row 0 the
        scale of the condition stepped to first, row 1 the other's (gdx_set_guidance_compose).  Under perturbed-attention guidance
        (gdx_set_attention_guidance): 1 + y['pag_scale'] alone (`scale` is not read), or [y['scale'], y['pag_scale']] stacked."""
        kind, _, pag_scale = self.attention
        if kind == _lib.GDX_PAG_ONLY:                       # g = P + (1 + w)(F - P) = F + w(F - P); fl32(1 + w), computed once
            return (1.0 + pag_scale.reshape(-1).float()).contiguous()
        mode, text_scale = self.values["compose"]
        scale = scale.reshape(-1).float()
        if kind == _lib.GDX_PAG_CFG:                        # [2, B]: row 0 the CFG scale s0, row 1 the PAG scale s1
            return torch.stack([scale, pag_scale.reshape(-1).float()]).contiguous()
        if text_scale is None:
            return scale.contiguous()
        text_scale = text_scale.reshape(-1).float()
        first, second = (scale, text_scale) if mode == _lib.GDX_GUIDE_SEED_TEXT else (text_scale, scale)
        return torch.stack([first, second]).contiguous()


# sample_chunks keyword -> (y key, written(value), to_y(value, batch, device))
_given = lambda v: v is not None                                                  # noqa: E731
_same = lambda v, b, dev: v                                                       # noqa: E731
_pair = lambda v, b, dev: (int(v[0]), int(v[1]))                                  # noqa: E731
KWARG_TO_Y = {
    "guidance_interval": ("guidance_interval", _given, _pair),
    "guidance_rescale": ("guidance_rescale", lambda v: v > 0, lambda v, b, dev: float(v)),
    "guidance_refresh": ("guidance_refresh", lambda v: v > 1, _same),
    "text_guidance_param": ("text_scale", _given, lambda v, b, dev: torch.ones(b, device=dev) * v),
    "guidance_order": ("guidance_order", _given, _same),
    "guidance_drop": ("guidance_drop", _given, _same),
    "layer_cache": ("layer_cache", _given, _pair),
}


def y_of_kwargs(kwargs, batch, device):
    """The option keys of a y for `batch` samples on `device` from sample_chunks' keyword values; every keyword must be there."""
    return {key: to_y(kwargs[kw], batch, device) for kw, (key, written, to_y) in KWARG_TO_Y.items() if written(kwargs[kw])}
