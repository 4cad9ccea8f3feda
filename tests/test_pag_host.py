"""Perturbed-attention guidance without a GPU: the CPU restatement (tests/pag_restatement.py) against what the reference's own
MDM and MDM_Old computed under an identity attention mask (tests/golden/forward_pag.npz, tools/make_golden_pag.py), the operation
order of both rules, the y validation, the conflicts, the CLI and every refusal of the C ABI that needs no device.

Measured on the CPU (fp32, relative to max|reference|): forwards F / P / U at most 5.5e-7 over the three cases, the two loops
1.4e-6 (GDX_PAG_ONLY) and 9.9e-7 (GDX_PAG_CFG).  The bounds are ten times the measured value where that is tighter than the bound
tests/test_compose_host.py uses for the same comparison (2e-6 forwards, 2e-5 loops), else that bound."""
import ctypes as C

import pytest
import torch

import pag_restatement as pr
from conftest import load_golden, rel_err
from gesturediffusion_amd import _lib, numerics
from gesturediffusion_amd import engine as E
from gesturediffusion_amd import sampling_options
from oracle import sampler as osamp
from oracle import schedule as osch

FORWARD_BOUND, LOOP_BOUND = 2e-6, 1.4e-5


@pytest.fixture(scope="module")
def g():
    return load_golden("forward_pag.npz")


# ------------------------------------------------------------------------------------------- the restatement vs the reference
@pytest.mark.parametrize("name", sorted(pr.CASES))
def test_restatement_passes_equal_the_reference(g, name):
    cfg, sd, x, t, y, layers = pr.case(g, name)
    p = pr.passes(sd, cfg, x, t, y, layers)
    for tag in "FPU":
        err = rel_err(p[tag], g[f"{name}.{tag}"])
        print(f"[pag-measure] restatement {name}.{tag}: rel err {err:.2e}")
        assert err < FORWARD_BOUND, tag
    for a, b in ("FP", "FU", "PU"):                             # the perturbation is no rounding error
        assert rel_err(p[a], p[b]) > 1e-3, (a, b)
    with torch.no_grad():                                       # the swap is undone
        from oracle import mdm_forward as omf
        assert torch.equal(omf.forward(sd, cfg, x, t, y), p["F"])


@pytest.mark.parametrize("kind", ["only", "cfg"])
def test_restatement_loop_equals_the_reference(g, kind):
    name = pr.LOOP_CASE
    cfg, sd, x, t, y, layers = pr.case(g, name)
    tab, tmap = osch.make_tables("cosine", 1000, pr.RESPACING)
    k = pr.ONLY if kind == "only" else pr.CFG
    fn = lambda xx, tt, yy: pr.guided_forward(sd, cfg, xx, tt, yy, layers, k)          # noqa: E731
    tape = torch.from_numpy(g[f"{name}.{kind}_p20.tape"])
    yy = dict(y, pag_scale=torch.from_numpy(g[f"{name}.{kind}_w"]))
    if kind == "cfg":
        yy["scale"] = torch.from_numpy(g[f"{name}.cfg_s"])
    with torch.no_grad():
        r = osamp.sample_loop(fn, tab, tmap, tuple(tape[0].shape), tape, yy, kind="p")
    err = rel_err(r, g[f"{name}.{kind}_p20.out"])
    print(f"[pag-measure] restatement p20 loop {kind}: rel err {err:.2e}")
    assert err < LOOP_BOUND


# ------------------------------------------------------------------------------------------------------- the rules' op order
def test_both_rules_round_in_the_order_written():
    """float64 inputs at which another association of the same algebra gives other bits."""
    gen = torch.Generator().manual_seed(9)
    p = {k: torch.randn(3, 4, 1, 5, generator=gen, dtype=torch.float64) for k in "FPU"}
    s0 = torch.tensor([1.5, 2.5, 0.75], dtype=torch.float64)
    s1 = torch.tensor([3.0, -1.0, 2.25], dtype=torch.float64)
    v0, v1 = s0.view(3, 1, 1, 1), s1.view(3, 1, 1, 1)
    f, q, u = p["F"], p["P"], p["U"]
    only = pr.compose_only(p, s0)
    assert torch.equal(only, q + v0 * (f - q))
    assert not torch.equal(only, (1 - v0) * q + v0 * f) and not torch.equal(only, f + (v0 - 1) * (f - q))
    assert float((only - ((1 - v0) * q + v0 * f)).abs().max()) < 1e-14
    cfg = pr.compose_cfg(p, s0, s1)
    assert torch.equal(cfg, (u + v0 * (f - u)) + v1 * (f - q))
    assert not torch.equal(cfg, u + (v0 * (f - u) + v1 * (f - q)))
    assert not torch.equal(cfg, (1 - v0) * u + (v0 + v1) * f - v1 * q)
    assert float((cfg - ((1 - v0) * u + (v0 + v1) * f - v1 * q)).abs().max()) < 1e-13
    # w = 0: kind 2 is the joint blend, kind 1 at operand 1 is F up to rounding, at operand 0 it is P
    zero, one = torch.zeros(3, dtype=torch.float64), torch.ones(3, dtype=torch.float64)
    assert torch.equal(pr.compose_cfg(p, s0, zero), u + v0 * (f - u))
    assert torch.equal(pr.compose_only(p, zero), q) and float((pr.compose_only(p, one) - f).abs().max()) < 1e-14
    # the triangle factors of numerics.py are the rules' coefficient sums
    assert numerics.pag_factor(3.0) == 7.0 and numerics.pag_factor(-1.0) == 1.0 and numerics.pag_factor(0.0) == 1.0
    assert numerics.pag_factor(3.0, 1.5) == 0.5 + 4.5 + 3.0 and numerics.pag_factor(0.0, 2.5) == numerics.guidance_factor(2.5)


def test_scale_operands():
    w, s = torch.tensor([3.0, 0.5, 1.25]), torch.tensor([1.5, 2.5, 0.75])
    off = {"compose": (_lib.GDX_GUIDE_JOINT, None)}
    only = sampling_options.Record(off, (_lib.GDX_PAG_ONLY, 2, w.double())).scale_operand(None)
    assert only.dtype == torch.float32 and torch.equal(only, torch.tensor([4.0, 1.5, 2.25]))
    both = sampling_options.Record(off, (_lib.GDX_PAG_CFG, 2, w)).scale_operand(s.view(3, 1))
    assert both.is_contiguous() and torch.equal(both, torch.stack([s, w]))
    assert torch.equal(sampling_options.Record(off).scale_operand(s.view(3, 1, 1, 1)), s)
    assert [_lib.GDX_PAG_OFF, _lib.GDX_PAG_ONLY, _lib.GDX_PAG_CFG] == [pr.OFF, pr.ONLY, pr.CFG] == [0, 1, 2]
    assert pr.layer_mask((0, 2)) == 5


# ------------------------------------------------------------------------------------------------------------- y validation
def test_attention_guidance_of_y():
    sc, w = torch.ones(3), torch.ones(3) * 2
    seed = torch.zeros(3, 16, 1, 10)

    def of(y, guided=True, layers=4, pag_only=False):
        base = {"seed": seed} if pag_only else {"seed": seed, "scale": sc}
        return E.attention_guidance_of(dict(base, **y), guided, layers, pag_only)
    assert of({}) == E.PAG_OFF == (0, 0, None) and of({}, guided=False) == E.PAG_OFF
    with pytest.raises(ValueError, match=r"PerturbedAttentionSampleModel needs y\['pag_scale'\]"):
        of({}, pag_only=True)
    for key, val in (("pag_scale", w), ("pag_layers", (1,))):
        with pytest.raises(ValueError, match="needs a PerturbedAttentionSampleModel or a ClassifierFreeSampleModel"):
            of({key: val}, guided=False)
    with pytest.raises(ValueError, match=r"pag_layers'\] needs y\['pag_scale'\]"):
        of({"pag_layers": (1,)})
    for key, val in (("scale", sc), ("guidance_drop", "both"), ("text_scale", w), ("guidance_order", "seed_text")):
        with pytest.raises(ValueError, match=rf"y\['{key}'\] belongs to classifier-free guidance"):
            of({"pag_scale": w, key: val}, pag_only=True)
    for drop in ("text", "seed"):
        with pytest.raises(ValueError, match=r"guidance_drop'\] other than 'both' exclude each other"):
            of({"pag_scale": w, "guidance_drop": drop})
    with pytest.raises(ValueError, match=r"pag_scale'\] and y\['text_scale'\] exclude each other"):
        of({"pag_scale": w, "text_scale": w})
    for bad in (2.0, [2.0, 2.0, 2.0], torch.ones(3, dtype=torch.int64), None):
        with pytest.raises(ValueError, match=r"pag_scale'\] must be a floating tensor"):
            of({"pag_scale": bad})
    for bad in (torch.ones(2), torch.ones(3, 1), torch.ones(()), torch.ones(4)):
        for pag_only in (False, True):
            with pytest.raises(ValueError, match=r"pag_scale'\] must be \[batch\]"):
                of({"pag_scale": bad}, pag_only=pag_only)
    with pytest.raises(ValueError, match="not a tensor: reading it would synchronise"):
        of({"pag_scale": w, "pag_layers": torch.tensor([1])})
    for bad in ((), [], True, 1, 1.0, (1.0,), (True,), "1", None):
        with pytest.raises(ValueError, match=r"pag_layers'\] must be a non-empty tuple or list of Python ints"):
            of({"pag_scale": w, "pag_layers": bad})
    for bad in ((1, 1), (4,), (-1,), (0, 7)):
        with pytest.raises(ValueError, match=r"distinct encoder layers in 0 \.\. num_layers - 1 = 3"):
            of({"pag_scale": w, "pag_layers": bad})
    with pytest.raises(E.GdxError, match=r"y\['pag_scale'\] is on cpu"):        # a host tensor has no fallback, like y['seed']
        of({"pag_scale": w})
    # everything in front of the device check holds: kind, default layer, mask
    seen = []
    real = E.require_device
    E.require_device = lambda t, what: seen.append(what) or t
    try:
        assert of({"pag_scale": w})[:2] == (_lib.GDX_PAG_CFG, 1 << 2)
        assert of({"pag_scale": w, "guidance_drop": "both"})[:2] == (_lib.GDX_PAG_CFG, 1 << 2)
        assert of({"pag_scale": w}, layers=5, pag_only=True)[:2] == (_lib.GDX_PAG_ONLY, 1 << 2)
        assert of({"pag_scale": w, "pag_layers": [3, 0]})[:2] == (_lib.GDX_PAG_CFG, 0b1001)
        assert of({"pag_scale": w, "pag_layers": (0,)}, layers=1, pag_only=True)[1:] == (1, w)
    finally:
        E.require_device = real
    assert seen == ["y['pag_scale']"] * 5


class Recorder:
    """Stands in for an Engine: every method call is recorded as (name, positional arguments, keywords)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *a, **kw: self.calls.append((name, a, kw))


def test_the_setting_travels_with_the_compose_setter_and_absent_keys_reset_it(monkeypatch):
    monkeypatch.setattr(E, "require_device", lambda t, what: t)
    w = torch.ones(2)
    rec = Recorder()
    sampling_options.read({"pag_scale": w, "scale": w}, guided=True, num_layers=4, use_text=False).apply_before_condition(rec)
    sampling_options.read({"pag_scale": w, "pag_layers": (0, 3)}, guided=True, num_layers=4, use_text=False,
                          pag_only=True).apply_before_condition(rec)
    sampling_options.read({"scale": w}, guided=True, num_layers=4, use_text=False).apply_before_condition(rec)
    sampling_options.read({"guidance_rescale": 0.5}, guided=True, num_layers=4, use_text=False).apply_before_condition(rec)
    assert rec.calls == [("set_guidance_compose", (_lib.GDX_GUIDE_JOINT,), {"attention": (_lib.GDX_PAG_CFG, 4)}),
                         ("set_guidance_compose", (_lib.GDX_GUIDE_JOINT,), {"attention": (_lib.GDX_PAG_ONLY, 9)}),
                         ("set_guidance_compose", (_lib.GDX_GUIDE_JOINT,), {"attention": (_lib.GDX_PAG_OFF, 0)}),
                         ("set_guidance_compose", (_lib.GDX_GUIDE_JOINT,), {"attention": (_lib.GDX_PAG_OFF, 0)})]
    # the paths that read a part of the table: the plain forwards refuse the keys, the memory check does not look at them
    with pytest.raises(ValueError, match="needs a PerturbedAttentionSampleModel"):
        sampling_options.read({"pag_scale": w}, guided=False, num_layers=4, use_text=False, options=sampling_options.PLAIN_FORWARD)
    assert sampling_options.read({"pag_layers": 3}, guided=False, num_layers=4, use_text=False,
                                 options=sampling_options.MEMORY).attention == E.PAG_OFF


def test_wrappers():
    from gesturediffusion_amd.model.cfg_sampler import ClassifierFreeSampleModel
    from gesturediffusion_amd.model.mdm import MDM
    from gesturediffusion_amd.model.pag_sampler import PerturbedAttentionSampleModel
    kw = dict(njoints=16, nfeats=1, pose_rep="rot6d", data_rep="genea_vec", latent_dim=64, ff_size=64, num_layers=3, seed_poses=10,
              mfcc_input=True)
    trained_without = MDM(cond_mask_prob=0.0, **kw).eval()
    with pytest.raises(AssertionError, match="has not been trained with no conditions"):
        ClassifierFreeSampleModel(trained_without)
    g = PerturbedAttentionSampleModel(trained_without)
    assert isinstance(g, ClassifierFreeSampleModel) and g.pag_only and not ClassifierFreeSampleModel.pag_only
    with pytest.raises(TypeError, match="wraps gesturediffusion_amd MDM"):
        PerturbedAttentionSampleModel(torch.nn.Linear(2, 2))

    class OnDevice:                      # passes _check_inputs without a device
        device = torch.device("cuda")
        shape = (2, 16, 1, 20)

        def dim(self):
            return 4
    y = {"seed": torch.zeros(2, 16, 1, 10), "mfcc": torch.zeros(2, 26, 1, 20)}
    with pytest.raises(ValueError, match=r"needs y\['pag_scale'\]"):
        g(OnDevice(), None, y)
    with pytest.raises(ValueError, match="belongs to classifier-free guidance"):
        g(OnDevice(), None, dict(y, pag_scale=torch.ones(2), scale=torch.ones(2)))
    for model in (trained_without, MDM(cond_mask_prob=0.1, **kw).eval()):
        with pytest.raises(ValueError, match="needs a PerturbedAttentionSampleModel or a ClassifierFreeSampleModel"):
            model.forward(OnDevice(), None, dict(y, pag_scale=torch.ones(2)))


def test_three_pass_conflicts():
    w = torch.ones(2)

    def conflicts(kind, y, parallel=False):
        sampling_options.Record({"compose": (_lib.GDX_GUIDE_JOINT, None), "refresh": E.guidance_refresh_of(y, True),
                                 "layer_cache": E.layer_cache_of(y, 8)}, (kind, 1, w)).refuse_conflicts(parallel=parallel)
    many = {"guidance_refresh": 2, "layer_cache": (2, 1)}
    conflicts(_lib.GDX_PAG_CFG, {})
    conflicts(_lib.GDX_PAG_CFG, {"guidance_refresh": 1, "layer_cache": (1, 0)})
    with pytest.raises(ValueError, match=r"guidance_refresh'\] > 1 exclude each other"):
        conflicts(_lib.GDX_PAG_CFG, {"guidance_refresh": 2})
    with pytest.raises(ValueError, match=r"layer_cache'\] with every > 1 exclude each other"):
        conflicts(_lib.GDX_PAG_CFG, {"layer_cache": (2, 1)})
    with pytest.raises(ValueError, match="not supported by parallel_sample_loop"):
        conflicts(_lib.GDX_PAG_CFG, {}, parallel=True)
    for kind in (_lib.GDX_PAG_ONLY, _lib.GDX_PAG_OFF):          # two row groups keep every feature
        conflicts(kind, many, parallel=True)


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def _cfg(**over):
    kw = dict(arch=_lib.GDX_ARCH_MDM, njoints=16, latent_dim=128, ff_size=192, num_layers=3, num_heads=4, seed_poses=10,
              mfcc_dim=26, cl_head=8, window=10, compute_dtype=0, text_dim=0, clip_dim=0)
    kw.update(over)
    return _lib.Config(**kw)


def test_prototypes_and_refusals_without_a_device():
    lib = _lib.load()
    protos = _lib.HEADER.prototypes
    assert protos["gdx_set_attention_guidance"] == ("int", [("gdx_handle_t", "h"), ("int32_t", "kind"), ("uint64_t", "layer_mask")])
    assert protos["gdx_attention_identity"] == ("int", [("int32_t", "elem_bytes"), ("int64_t", "rows"), ("int32_t", "d"),
                                                        ("const void*", "qkv"), ("void*", "ctx")])
    assert (_lib.GDX_PAG_OFF, _lib.GDX_PAG_ONLY, _lib.GDX_PAG_CFG) == (0, 1, 2)
    for kind in (0, 1, 2, 7):
        assert lib.gdx_set_attention_guidance(None, kind, 0) != 0 and b"gdx_set_attention_guidance: null handle" in lib.gdx_last_error()
    # the stand-alone pass: every refusal is in front of the first HIP call
    a, b = C.c_void_p(1 << 20), C.c_void_p(1 << 21)
    for args, says in (((3, 4, 128, a, b), b"elem_bytes must be 2"), ((8, 4, 128, a, b), b"elem_bytes must be 2"),
                       ((4, 4, 128, None, b), b"null argument"), ((4, 4, 128, a, None), b"null argument"),
                       ((4, 0, 128, a, b), b"must be positive"), ((4, -1, 128, a, b), b"must be positive"),
                       ((2, 4, 0, a, b), b"must be positive"), ((4, 4, 130, a, b), b"multiple of 16 bytes"),
                       ((2, 4, 132, a, b), b"multiple of 16 bytes"), ((4, 4, 128, C.c_void_p((1 << 20) + 4), b), b"16-byte aligned"),
                       ((2, 4, 128, a, C.c_void_p((1 << 21) + 8)), b"16-byte aligned")):
        assert lib.gdx_attention_identity(*args) != 0 and says in lib.gdx_last_error(), args
    h = C.c_void_p()
    if lib.gdx_create(C.byref(_cfg()), C.byref(h)) == 0:          # where a handle can be made without a device
        for bad in (-1, 3, 99):
            assert lib.gdx_set_attention_guidance(h, bad, 1) != 0 and b"unknown kind" in lib.gdx_last_error()
        for kind in (0, 1, 2):
            for mask in (1 << 3, 1 << 63, 0b1111):
                assert lib.gdx_set_attention_guidance(h, kind, mask) != 0 and b"beyond num_layers = 3" in lib.gdx_last_error()
        for kind, mask in ((1, 0b101), (2, 0b010), (1, 0), (0, 0b111), (0, 0)):   # an unprepared handle: nothing to re-prepare
            assert lib.gdx_set_attention_guidance(h, kind, mask) == 0
        for bad in (-1, 5, 99):
            assert lib.gdx_set_guidance_compose(h, bad) != 0 and b"unknown mode" in lib.gdx_last_error()
        assert lib.gdx_set_guidance_compose(h, 1) != 0 and b"nothing to compose" in lib.gdx_last_error()
        # kind 2 is refused by the parallel loop before it looks at the workspace
        assert lib.gdx_set_attention_guidance(h, 2, 1) == 0
        one, anchor, its = C.c_void_p(16), C.c_int32(0), C.c_int32(0)
        tmap, thr = (C.c_int64 * 4)(0, 1, 2, 3), (C.c_double * 4)()
        rc = lib.gdx_parallel_loop(h, _lib.GDX_SAMPLER_P, _lib.GDX_CFG, 4, 3, one, tmap, thr, 2, one, one, None, None, 0, None, 0, 0,
                                   C.byref(anchor), 0, None, 0, C.byref(its), None)
        assert rc != 0 and b"not supported by the parallel loop" in lib.gdx_last_error()
        lib.gdx_destroy(h)
    h = C.c_void_p()
    if lib.gdx_create(C.byref(_cfg(num_layers=65)), C.byref(h)) == 0:
        assert lib.gdx_set_attention_guidance(h, 0, 1 << 63) == 0
        for kind in (1, 2):
            assert lib.gdx_set_attention_guidance(h, kind, 1) != 0 and b"this handle has more" in lib.gdx_last_error()
        lib.gdx_destroy(h)
    h = C.c_void_p()
    if lib.gdx_create(C.byref(_cfg(text_dim=64, clip_dim=512, num_layers=1)), C.byref(h)) == 0:
        # a compose mode other than JOINT: the guided loop is refused in front of its look at the workspace
        assert lib.gdx_set_guidance_compose(h, 1) == 0 and lib.gdx_set_attention_guidance(h, 1, 1) == 0
        one, anchor, its = C.c_void_p(16), C.c_int32(0), C.c_int32(0)
        tmap, thr = (C.c_int64 * 4)(0, 1, 2, 3), (C.c_double * 4)()
        rc = lib.gdx_parallel_loop(h, _lib.GDX_SAMPLER_P, _lib.GDX_CFG, 4, 3, one, tmap, thr, 2, one, one, None, None, 0, None, 0, 0,
                                   C.byref(anchor), 0, None, 0, C.byref(its), None)
        assert rc != 0 and b"four are not supported" in lib.gdx_last_error()
        lib.gdx_destroy(h)


def test_the_layout_table():
    """groups / three_pass / u_group of every (compose mode, PAG kind), read from the header both sides include."""
    import os
    import re
    from conftest import REPO
    src = open(os.path.join(REPO, "gesturediffusion_amd", "csrc", "gdx_host.h")).read()
    body = re.search(r"GUIDE_LAYOUT\[5\]\[3\] = \{(.*?)\n\};", src, re.S).group(1)
    rows = [re.findall(r"\{(\d), (true|false), (\d)\}", line) for line in body.splitlines() if "{{" in line]
    assert len(rows) == 5 and all(len(r) == 3 for r in rows)
    joint = [(int(a), b == "true", int(c)) for a, b, c in rows[0]]
    assert joint == [(2, False, 1), (2, False, 2), (3, True, 2)]
    for mode in (1, 2):
        assert set(rows[mode]) == {("2", "false", "2")}
    for mode in (3, 4):
        assert set(rows[mode]) == {("3", "true", "2")}
    assert "guide_compose >=" not in src                         # no helper compares the compose mode by order any more


# --------------------------------------------------------------------------------------------------------------------- CLI
def test_cli_flags(capsys):
    from gesturediffusion_amd.utils.parser_util import generate_args
    base = ["--synthetic"]
    a = generate_args(base)
    assert (a.pag_scale, a.pag_layers) == (None, None)
    a = generate_args(base + ["--guidance_param", "1", "--pag_scale", "3"])
    assert (a.pag_scale, a.pag_layers, a.guidance_param) == (3.0, (a.layers // 2,), 1)
    a = generate_args(base + ["--pag_scale", "2", "--pag_layers", "3", "4", "--sampler", "dpmpp", "--timestep_respacing", "logsnr20"])
    assert (a.pag_scale, a.pag_layers) == (2.0, (3, 4)) and a.guidance_param == 2.5
    # under kind 1 the features of a two-group guided call stay
    a = generate_args(base + ["--guidance_param", "1", "--pag_scale", "3", "--guidance_refresh", "2", "--layer_cache", "2", "1",
                              "--guidance_interval", "300", "700", "--guidance_rescale", "0.5"])
    assert a.guidance_refresh == 2 and a.layer_cache == (2, 1)
    assert generate_args(base + ["--guidance_param", "1", "--pag_scale", "3", "--parallel_window", "4"]).parallel_window == 4
    assert generate_args(base + ["--use_text", "--pag_scale", "3", "--guidance_drop", "both"]).guidance_drop == "both"
    text = base + ["--use_text", "--pag_scale", "2"]
    for argv, says in (
            (base + ["--pag_layers", "1"], "--pag_layers needs --pag_scale"),
            (base + ["--pag_scale", "2", "--pag_layers", "1", "1"], "distinct encoder layers"),
            (base + ["--pag_scale", "2", "--pag_layers", "8"], "distinct encoder layers"),
            (base + ["--pag_scale", "2", "--pag_layers", "-1"], "distinct encoder layers"),
            (base + ["--pag_scale", "2", "--pag_layers"], "expected at least one argument"),
            (text + ["--text_guidance_param", "2"], "--pag_scale and --text_guidance_param exclude each other"),
            (text + ["--guidance_drop", "text"], "--pag_scale and --guidance_drop text|seed exclude each other"),
            (text + ["--guidance_drop", "seed"], "--pag_scale and --guidance_drop text|seed exclude each other"),
            (base + ["--pag_scale", "2", "--invert_gt"], "--pag_scale does not combine with --invert_gt"),
            (base + ["--pag_scale", "2", "--guidance_refresh", "2"], "runs no guidance refresh"),
            (base + ["--pag_scale", "2", "--layer_cache", "2", "1"], "runs no layer cache"),
            (base + ["--pag_scale", "2", "--parallel_window", "4"], "does not combine with --parallel_window"),
            (base + ["--guidance_param", "1", "--guidance_refresh", "2"], "--guidance_refresh needs guidance")):
        with pytest.raises(SystemExit):
            generate_args(argv)
        assert says in capsys.readouterr().err, argv
    from gesturediffusion_amd.sample.generate import sample_chunks
    with pytest.raises(ValueError, match="pag_layers needs pag_scale"):
        sample_chunks(None, None, torch.zeros(1, 1, 1, 1), None, 0, 20, 10, pag_layers=(1,))
    with pytest.raises(ValueError, match="guidance_interval needs guidance_param != 1"):
        sample_chunks(None, None, torch.zeros(1, 1, 1, 1), None, 0, 20, 10, guidance_interval=(3, 7))
    # with pag_scale a run at guidance_param 1 is guided: nothing is refused, and no chunk is no work
    assert sample_chunks(None, type("D", (), {k: None for k in ("p_sample_loop", "ddim_sample_loop", "plms_sample_loop", "dpm_solver_sample_loop",
                                                               "dpm_solver_sde_sample_loop", "unipc_sample_loop")}),
                         torch.zeros(1, 1, 1, 1), None, 0, 20, 10, guidance_interval=(3, 7), guidance_refresh=2, pag_scale=2.0) == []
