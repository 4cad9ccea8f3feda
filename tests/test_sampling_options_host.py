"""The table of y's sampling options (gesturediffusion_amd/sampling_options.py) walked over the paths that read y, without a
GPU: an engine stand-in records the calls that the guided step-wise forward and _native_loop_setup (plain and windowed) make.
Every option of the table needs a sample below, so a new entry is tested on every path or this module fails."""
import inspect
import re

import pytest
import torch

from gesturediffusion_amd import _lib
from gesturediffusion_amd import engine as E
from gesturediffusion_amd import sampling_options as SO
from gesturediffusion_amd.diffusion.gaussian_diffusion import GaussianDiffusion
from gesturediffusion_amd.model import cfg_sampler
from gesturediffusion_amd.model.cfg_sampler import ClassifierFreeSampleModel
from gesturediffusion_amd.model.mdm import MDM
from gesturediffusion_amd.model.mdm_old import MDM_Old

# option name -> (y keys of a valid value that is not "off", the setter call an absent key makes, the call that value makes)
SAMPLES = {
    "interval": ({"guidance_interval": (300, 700)}, ("set_guidance_interval", (None,)), ("set_guidance_interval", ((300, 700),))),
    "rescale": ({"guidance_rescale": 0.5}, ("set_guidance_rescale", (0.0,)), ("set_guidance_rescale", (0.5,))),
    "compose": ({"guidance_drop": "text"}, ("set_guidance_compose", (_lib.GDX_GUIDE_JOINT,)),
                ("set_guidance_compose", (_lib.GDX_GUIDE_TEXT,))),
    "refresh": ({"guidance_refresh": 3}, ("set_guidance_refresh", (1,)), ("set_guidance_refresh", (3,))),
    "layer_cache": ({"layer_cache": (2, 1)}, ("set_layer_cache", (1, 0)), ("set_layer_cache", (2, 1))),
}
EVERY_ONE = {"refresh": {"guidance_refresh": 1}, "layer_cache": {"layer_cache": (1, 5)}}     # a memory option at every = 1
NEEDS_GUIDED = "needs a ClassifierFreeSampleModel"


class X:                                 # passes _check_inputs without a device
    device = torch.device("cuda")
    shape = (2, 16, 1, 20)

    def dim(self):
        return 4


class Recorder:
    """Stands in for an Engine: every method call is recorded as (name, positional arguments)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args, **kw):
            self.calls.append((name, args))
            return torch.zeros(X.shape) if name == "forward" else None
        return call


def _stub(model):
    model.__dict__["_get_engine"] = lambda device: model.__dict__["recorder"]
    model.__dict__["_text_features"] = lambda y, bs: None
    return model.eval()


@pytest.fixture(scope="module")
def models():
    kw = dict(njoints=16, nfeats=1, pose_rep="rot6d", data_rep="genea_vec", latent_dim=64, ff_size=64, num_layers=3,
              cond_mask_prob=0.1, seed_poses=10)
    plain = _stub(MDM(text_dim=16, clip_dim=8, use_text=True, mfcc_input=True, **kw))
    old = _stub(MDM_Old(translation=True, glob=True, glob_rot=True, **kw))
    return plain, old, ClassifierFreeSampleModel(plain)


def _y(**keys):
    return dict({"seed": torch.zeros(2, 16, 1, 10), "mfcc": torch.zeros(2, 26, 1, 20), "scale": torch.ones(2)}, **keys)


def _forward(model, y):
    model(X(), torch.zeros(2, dtype=torch.long), y=y)


def _loop_setup(window):
    def run(model, y):
        if isinstance(model, ClassifierFreeSampleModel):         # the setters are behind it; the scale operand needs a device
            with pytest.raises(E.GdxError, match=r"y\['scale'\] is on cpu"):
                GaussianDiffusion._native_loop_setup(None, model, X(), {"y": y}, window=window)
        else:
            GaussianDiffusion._native_loop_setup(None, model, X(), {"y": y}, window=window)
    return run


# path -> (how it runs, the options it sets, the calls between the compose setter and the others)
PATHS = {
    "guided forward": (_forward, [o for o in SO.OPTIONS if not o.memory], ["prepare", "set_condition"]),
    "loop setup": (_loop_setup(None), list(SO.OPTIONS), ["prepare", "set_condition"]),
    "windowed loop setup": (_loop_setup(4), list(SO.OPTIONS), ["prepare_window"]),
}


def _calls(model, run, y):
    inner = getattr(model, "model", model)
    inner.__dict__["recorder"] = Recorder()
    run(model, y)
    return inner.__dict__["recorder"].calls


def test_every_option_has_a_sample():
    assert set(SAMPLES) == {o.name for o in SO.OPTIONS} and set(EVERY_ONE) == {o.name for o in SO.MEMORY}
    for o in SO.OPTIONS:
        keys, off_call, _ = SAMPLES[o.name]
        assert set(keys) <= set(o.keys)
        assert o.validate({}, True, 3, True) == o.off and o.validate(keys, True, 3, True) != o.off
        rec = Recorder()
        o.setter(rec, o.off)
        assert rec.calls == [off_call]
    assert [o.name for o in SO.OPTIONS if o.before] == ["compose"]
    assert [o.name for o in SO.OPTIONS if not o.guided] == ["layer_cache"]
    assert [o.name for o in SO.MEMORY] == ["refresh", "layer_cache"]


@pytest.mark.parametrize("path", sorted(PATHS))
def test_setters_get_off_or_the_value_in_order(models, path):
    guided = models[2]
    run, sets, between = PATHS[path]
    tail = ["forward"] if path == "guided forward" else []
    order = ([SAMPLES[o.name][1][0] for o in sets if o.before] + between
             + [SAMPLES[o.name][1][0] for o in sets if not o.before] + tail)
    today = ["set_guidance_compose"] + between + ["set_guidance_interval", "set_guidance_rescale"]
    today += (["set_guidance_refresh", "set_layer_cache"] if path != "guided forward" else []) + tail
    known = {call[0] for _, call, _ in SAMPLES.values()} | set(between + tail)
    assert [name for name in order if name in known] == today
    # absent keys: "off" reaches every setter this path calls
    calls = _calls(guided, run, _y())
    assert [c[0] for c in calls] == order
    for o in sets:
        assert SAMPLES[o.name][1] in calls, o.name
    # one valid value at a time: it reaches its setter, the others still get "off"
    for o in sets:
        keys, off_call, value_call = SAMPLES[o.name]
        calls = _calls(guided, run, _y(**keys))
        assert [c[0] for c in calls] == order, o.name
        assert value_call in calls and off_call not in calls, o.name
        for other in sets:
            assert other is o or SAMPLES[other.name][1] in calls, (o.name, other.name)
    # a plain model on the loop paths: same order, "off" everywhere
    if path != "guided forward":
        calls = _calls(models[0], run, _y())
        assert [c[0] for c in calls] == order and all(SAMPLES[o.name][1] in calls for o in sets)


def test_the_guided_forward_leaves_the_memory_setters_alone(models):
    names = [c[0] for c in _calls(models[2], _forward, _y(**EVERY_ONE["refresh"], **EVERY_ONE["layer_cache"]))]
    assert names == ["set_guidance_compose", "prepare", "set_condition", "set_guidance_interval", "set_guidance_rescale", "forward"]


def test_options_that_need_memory_are_refused_by_every_path_without(models):
    plain, _, guided = models
    refuse = GaussianDiffusion._refuse_refresh
    paths = (("forward", guided, lambda y: _calls(guided, _forward, _y(**y))),
             ("guided", guided, lambda y: refuse(guided, {"y": y}, "calc_bpd_loop")),
             ("plain", plain, lambda y: refuse(plain, {"y": y}, "calc_bpd_loop")),
             ("foreign", None, lambda y: refuse(lambda x, t, **kw: x, {"y": y}, "calc_bpd_loop")))
    for o in SO.MEMORY:
        many, one = SAMPLES[o.name][0], EVERY_ONE[o.name]
        for name, model, run in paths:
            if o.guided and model is not guided:                 # the key itself is refused, at any value
                for y in (many, one):
                    with pytest.raises(ValueError, match=NEEDS_GUIDED):
                        run(y)
                continue
            with pytest.raises(ValueError, match="needs the in-library loop") as e:
                run(many)
            assert f"y['{o.keys[0]}'] = " in str(e.value) and o.memory[1] in str(e.value), (o.name, name)
            run(one)
    for bad in (None, {}, {"y": None}, {"y": 3}):                # no y, or one that is not a dict: nothing to refuse
        refuse(guided, bad, "x")


def test_options_that_need_a_guided_model_are_refused_by_plain_models(models):
    plain, old, _ = models
    for o in SO.OPTIONS:
        if not o.guided:
            continue
        y = _y(**SAMPLES[o.name][0])
        for run in (_loop_setup(None), _loop_setup(4)):
            with pytest.raises(ValueError, match=NEEDS_GUIDED):
                run(plain, y)
        for model in (plain, old):
            if o in SO.PLAIN_FORWARD:
                with pytest.raises(ValueError, match=NEEDS_GUIDED):
                    _forward(model, y)
    # the plain forwards do not look at y['guidance_refresh'], and they call no option's setter but MDM's bare JOINT
    assert [o.name for o in SO.OPTIONS if o not in SO.PLAIN_FORWARD] == ["refresh"]
    y = _y(guidance_refresh=3)
    assert [c[0] for c in _calls(plain, _forward, y)] == ["set_guidance_compose", "prepare", "set_condition", "forward"]
    assert [c[0] for c in _calls(old, _forward, y)] == ["prepare", "set_condition", "forward"]
    for model, name in ((plain, "MDM"), (old, "MDM_Old")):
        with pytest.raises(ValueError, match=f"the step-wise forward of {name} cannot carry"):
            _forward(model, _y(layer_cache=(2, 1)))


def test_the_tables_keys_are_those_sample_chunks_writes_and_the_docstring_names():
    from gesturediffusion_amd.sample.generate import sample_chunks
    keys = {k for o in SO.OPTIONS for k in o.keys}
    assert len(keys) == sum(len(o.keys) for o in SO.OPTIONS)
    assert {key for key, _, _ in SO.KWARG_TO_Y.values()} == keys
    assert set(re.findall(r"y\['(\w+)'\]", cfg_sampler.__doc__)) == keys
    params = inspect.signature(sample_chunks).parameters
    defaults = {kw: params[kw].default for kw in SO.KWARG_TO_Y}       # KeyError: a keyword sample_chunks does not take
    assert SO.y_of_kwargs(defaults, 2, "cpu") == {}
    given = dict(guidance_interval=(300.0, 700), guidance_rescale=0.5, guidance_refresh=3, text_guidance_param=2.0,
                 guidance_order="text_seed", guidance_drop="text", layer_cache=[2, 1.0])
    y = SO.y_of_kwargs(given, 2, "cpu")
    assert set(y) == keys and torch.equal(y.pop("text_scale"), torch.full((2,), 2.0))
    assert y == {"guidance_interval": (300, 700), "guidance_rescale": 0.5, "guidance_refresh": 3, "guidance_order": "text_seed",
                 "guidance_drop": "text", "layer_cache": (2, 1)}
    assert all(type(v) is int for v in y["guidance_interval"] + y["layer_cache"])
    src = inspect.getsource(sample_chunks)
    assert all(f"{kw}={kw}" in src for kw in SO.KWARG_TO_Y)
