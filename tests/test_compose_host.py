"""Per-condition guidance for use_text models without a GPU: the CPU restatement (tests/compose_restatement.py) against what the
reference's own class computed under zeroed inputs (tests/golden/forward_text_compose.npz, tools/make_golden_compose.py), the
algebra of the 3-pass rule, the [2][B] packing, and every refusal that needs no device."""
import ctypes as C

import pytest
import torch

import compose_restatement as cr
from conftest import load_golden, rel_err
from gesturediffusion_amd import _lib
from gesturediffusion_amd import engine as E
from gesturediffusion_amd import sampling_options
from oracle import sampler as osamp
from oracle import schedule as osch

T64 = "mdm_128_t64"


@pytest.fixture(scope="module")
def g():
    return load_golden("forward_text_compose.npz")


# ------------------------------------------------------------------------------------------- the restatement vs the reference
@pytest.mark.parametrize("name", sorted(cr.CASES))
def test_restatement_passes_equal_the_reference(g, name):
    cfg, sd, x, t, y = cr.case(g, name)
    p = cr.passes(sd, cfg, x, t, y)
    for tag in "FSXU":
        assert rel_err(p[tag], g[f"{name}.{tag}"]) < 2e-6, tag
    # the four states differ at these weights, and U is the reference's own uncond
    for a, b in ("FS", "FX", "SU", "XU", "SX"):
        assert rel_err(p[a], p[b]) > 1e-3, (a, b)
    import text_restatement as tr
    with torch.no_grad():
        assert torch.equal(tr.forward(sd, cfg, x, t, dict(y, uncond=True)), p["U"])


@pytest.mark.parametrize("order", ["seed_text", "text_seed"])
def test_restatement_loop_equals_the_reference(g, order):
    cfg, sd, x, t, y = cr.case(g, T64)
    tab, tmap = osch.make_tables("cosine", 1000, cr.RESPACING)
    mode = cr.MODES[order]
    fn = lambda xx, tt, yy: cr.compose_forward(sd, cfg, xx, tt, yy, mode)          # noqa: E731
    tape = torch.from_numpy(g[f"{T64}.{order}_p20.tape"])
    yy = dict(y, scale=torch.from_numpy(g[T64 + ".seed_scale"]), text_scale=torch.from_numpy(g[T64 + ".text_scale"]))
    assert not torch.equal(yy["scale"], yy["text_scale"])
    with torch.no_grad():
        r = osamp.sample_loop(fn, tab, tmap, tuple(tape[0].shape), tape, yy, kind="p")
    assert rel_err(r, g[f"{T64}.{order}_p20.out"]) < 2e-5


def test_equal_scales_give_the_joint_blend_in_fp64(g):
    """At s0 == s1 == s the M terms cancel: both orders are U + s*(F - U) up to fp64 rounding."""
    p = {k: torch.from_numpy(g[f"{T64}.{k}"]).double() for k in "FSXU"}
    s = torch.tensor([2.5, 0.5, -1.25], dtype=torch.float64)
    joint = cr.compose(cr.JOINT, p, s)
    assert torch.equal(joint, p["U"] + s.view(-1, 1, 1, 1) * (p["F"] - p["U"]))
    for mode in (cr.SEED_TEXT, cr.TEXT_SEED):
        got = cr.compose(mode, p, s, s)
        assert float((got - joint).abs().max() / joint.abs().max()) < 1e-14
    # with different scales the orders differ from each other and from the joint blend
    s2 = s + 1.0
    a, b = cr.compose(cr.SEED_TEXT, p, s, s2), cr.compose(cr.TEXT_SEED, p, s, s2)
    assert rel_err(a, b) > 1e-3 and rel_err(a, joint) > 1e-3
    # the two-pass modes: scale 1 gives F, scale 0 the contrast pass
    one, zero = torch.ones(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64)
    assert float((cr.compose(cr.TEXT, p, one) - p["F"]).abs().max()) < 1e-14 and torch.equal(cr.compose(cr.TEXT, p, zero), p["S"])
    assert torch.equal(cr.compose(cr.SEED, p, zero), p["X"])


# ------------------------------------------------------------------------------------------------------------ the [2][B] packing
def test_scales_are_packed_in_stage_order():
    def operand(mode, scale, text_scale):
        return sampling_options.Record({"compose": (mode, text_scale)}).scale_operand(scale)
    seed, text = torch.tensor([1.0, 2.0, 3.0]), torch.tensor([10.0, 20.0, 30.0])
    a = operand(_lib.GDX_GUIDE_SEED_TEXT, seed.view(3, 1), text)
    b = operand(_lib.GDX_GUIDE_TEXT_SEED, seed, text.double())
    assert a.shape == b.shape == (2, 3) and a.is_contiguous() and b.is_contiguous() and b.dtype == torch.float32
    assert torch.equal(a, torch.stack([seed, text])) and torch.equal(b, torch.stack([text, seed]))
    assert torch.equal(a, cr.packed(cr.SEED_TEXT, seed, text)) and torch.equal(b, cr.packed(cr.TEXT_SEED, seed, text))
    for mode in (_lib.GDX_GUIDE_JOINT, _lib.GDX_GUIDE_TEXT, _lib.GDX_GUIDE_SEED):
        assert torch.equal(operand(mode, seed.view(3, 1, 1, 1), None), seed)
    assert [_lib.GDX_GUIDE_JOINT, _lib.GDX_GUIDE_TEXT, _lib.GDX_GUIDE_SEED, _lib.GDX_GUIDE_SEED_TEXT, _lib.GDX_GUIDE_TEXT_SEED] == [
        cr.JOINT, cr.TEXT, cr.SEED, cr.SEED_TEXT, cr.TEXT_SEED] == list(range(5))


# ------------------------------------------------------------------------------------------------------------- y validation
def test_guidance_compose_of_y():
    sc = torch.ones(3)
    ts = torch.ones(3) * 2

    def of(y, guided=True, use_text=True):
        return E.guidance_compose_of(dict({"scale": sc}, **y), guided, use_text)
    assert of({}) == (_lib.GDX_GUIDE_JOINT, None)
    assert of({}, guided=False, use_text=False) == (_lib.GDX_GUIDE_JOINT, None)
    for drop, mode in (("both", 0), ("text", 1), ("seed", 2)):
        assert of({"guidance_drop": drop}) == (mode, None)
    for key, val in (("guidance_drop", "text"), ("text_scale", ts), ("guidance_order", "seed_text")):
        with pytest.raises(ValueError, match="needs a ClassifierFreeSampleModel"):
            of({key: val}, guided=False)
        with pytest.raises(ValueError, match="needs a use_text model"):
            of({key: val}, use_text=False)
    with pytest.raises(ValueError, match="exclude each other"):
        of({"text_scale": ts, "guidance_drop": "text"})
    with pytest.raises(ValueError, match=r"guidance_order'\] needs y\['text_scale'\]"):
        of({"guidance_order": "text_seed"})
    with pytest.raises(ValueError, match=r"guidance_order'\] needs y\['text_scale'\]"):
        of({"guidance_order": "text_seed", "guidance_drop": "seed"})
    for bad in ("neither", 1, None, ("text",)):
        with pytest.raises(ValueError, match=r"guidance_drop'\] must be one of"):
            of({"guidance_drop": bad})
    for bad in ("text", 3, None):
        with pytest.raises(ValueError, match=r"guidance_order'\] must be one of"):
            of({"text_scale": ts, "guidance_order": bad})
    for bad in (2.0, [2.0, 2.0, 2.0], torch.ones(3, dtype=torch.int64), None):
        with pytest.raises(ValueError, match=r"text_scale'\] must be a floating tensor"):
            of({"text_scale": bad})
    for bad in (torch.ones(2), torch.ones(3, 1), torch.ones(()), torch.ones(4)):
        with pytest.raises(ValueError, match=r"text_scale'\] must be \[batch\]"):
            of({"text_scale": bad})
    with pytest.raises(E.GdxError, match=r"y\['text_scale'\] is on cpu"):          # a host tensor has no fallback, like y['seed']
        of({"text_scale": ts})


def test_plain_models_refuse_the_new_keys():
    """MDM.forward and MDM_Old.forward validate y before they look at a tensor."""
    import text_restatement as tr
    from gesturediffusion_amd.utils.init import init_state_dict
    cfg = tr.text_cfg(40, 32)
    m = tr.build_text_model(cfg, init_state_dict(cfg, seed=1))

    class OnDevice:                      # passes _check_inputs without a device
        device = torch.device("cuda")
        shape = (2, 16, 1, 20)

        def dim(self):
            return 4
    from gesturediffusion_amd.model.mdm_old import MDM_Old
    old = MDM_Old(njoints=16, nfeats=1, translation=True, pose_rep="rot6d", glob=True, glob_rot=True, latent_dim=64, num_layers=1,
                  data_rep="genea_vec", cond_mask_prob=0.1, seed_poses=10).eval()
    for key, val in (("guidance_drop", "text"), ("text_scale", torch.ones(2)), ("guidance_order", "seed_text")):
        for model in (m, old):
            with pytest.raises(ValueError, match="needs a ClassifierFreeSampleModel"):
                model.forward(OnDevice(), None, {key: val})


def test_three_pass_conflicts():
    y = {"text_scale": torch.ones(2)}
    three, two = _lib.GDX_GUIDE_SEED_TEXT, _lib.GDX_GUIDE_TEXT

    def conflicts(y, mode, num_layers, parallel=False):         # the mode as given: y['text_scale'] is on the host
        sampling_options.Record({"compose": (mode, y.get("text_scale")), "refresh": E.guidance_refresh_of(y, True),
                                 "layer_cache": E.layer_cache_of(y, num_layers)}).refuse_conflicts(parallel=parallel)
    conflicts(y, three, 8)
    conflicts(dict(y, guidance_refresh=1, layer_cache=(1, 0)), _lib.GDX_GUIDE_TEXT_SEED, 8)
    with pytest.raises(ValueError, match=r"guidance_refresh'\] > 1 exclude each other"):
        conflicts(dict(y, guidance_refresh=2), three, 8)
    with pytest.raises(ValueError, match=r"layer_cache'\] with every > 1 exclude each other"):
        conflicts(dict(y, layer_cache=(2, 1)), three, 8)
    with pytest.raises(ValueError, match="not supported by parallel_sample_loop"):
        conflicts(y, three, 8, parallel=True)
    # the two-pass modes keep every feature
    conflicts({"guidance_drop": "text", "guidance_refresh": 2, "layer_cache": (2, 1)}, two, 8, parallel=True)


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def _cfg(**over):
    kw = dict(arch=_lib.GDX_ARCH_MDM, njoints=16, latent_dim=128, ff_size=192, num_layers=1, num_heads=4, seed_poses=10,
              mfcc_dim=26, cl_head=8, window=10, compute_dtype=0, text_dim=64, clip_dim=512)
    kw.update(over)
    return _lib.Config(**kw)


def test_setter_refusals_and_no_new_stream_entry():
    lib = _lib.load()
    assert _lib.HEADER.prototypes["gdx_set_guidance_compose"] == ("int", [("gdx_handle_t", "h"), ("int32_t", "mode")])
    assert lib.gdx_set_guidance_compose(None, 0) != 0 and b"gdx_set_guidance_compose: null handle" in lib.gdx_last_error()
    assert lib.gdx_set_guidance_compose(None, 9) != 0 and b"null handle" in lib.gdx_last_error()
    h = C.c_void_p()
    if lib.gdx_create(C.byref(_cfg()), C.byref(h)) == 0:          # where a handle can be made without a device
        for bad in (-1, 5, 99):
            assert lib.gdx_set_guidance_compose(h, bad) != 0 and b"unknown mode" in lib.gdx_last_error()
        for mode in (3, 1, 4, 2, 0):                             # an unprepared handle: nothing to re-prepare, no HIP call
            assert lib.gdx_set_guidance_compose(h, mode) == 0
        # the parallel loop's refusal precedes its look at the workspace
        assert lib.gdx_set_guidance_compose(h, 3) == 0
        one, anchor, its = C.c_void_p(16), C.c_int32(0), C.c_int32(0)
        tmap, thr = (C.c_int64 * 4)(0, 1, 2, 3), (C.c_double * 4)()
        rc = lib.gdx_parallel_loop(h, _lib.GDX_SAMPLER_P, _lib.GDX_CFG, 4, 3, one, tmap, thr, 2, one, one, None, None, 0, None, 0, 0,
                                   C.byref(anchor), 0, None, 0, C.byref(its), None)
        assert rc != 0 and b"3-pass guidance compose mode" in lib.gdx_last_error()
        lib.gdx_destroy(h)
    h = C.c_void_p()
    if lib.gdx_create(C.byref(_cfg(text_dim=0, clip_dim=0)), C.byref(h)) == 0:
        assert lib.gdx_set_guidance_compose(h, 0) == 0
        for mode in (1, 2, 3, 4):
            assert lib.gdx_set_guidance_compose(h, mode) != 0 and b"nothing to compose" in lib.gdx_last_error()
        assert lib.gdx_set_guidance_compose(h, 7) != 0 and b"unknown mode" in lib.gdx_last_error()
        lib.gdx_destroy(h)


# --------------------------------------------------------------------------------------------------------------------- CLI
def test_cli_flags(capsys):
    from gesturediffusion_amd.utils.parser_util import generate_args
    base = ["--synthetic", "--use_text"]
    a = generate_args(base)
    assert (a.text_guidance_param, a.guidance_order, a.guidance_drop) == (None, None, None)
    a = generate_args(base + ["--text_guidance_param", "3.5", "--guidance_order", "text_seed"])
    assert (a.text_guidance_param, a.guidance_order, a.guidance_drop) == (3.5, "text_seed", None)
    assert generate_args(base + ["--guidance_drop", "text", "--guidance_refresh", "2", "--layer_cache", "2", "1"]).guidance_drop == "text"
    for argv, says in (
            (["--synthetic", "--text_guidance_param", "2"], "--text_guidance_param needs --use_text"),
            (["--synthetic", "--guidance_drop", "seed"], "--guidance_drop needs --use_text"),
            (["--synthetic", "--guidance_order", "seed_text"], "--guidance_order needs --use_text"),
            (base + ["--text_guidance_param", "2", "--guidance_param", "1"], "--text_guidance_param needs guidance"),
            (base + ["--guidance_drop", "text", "--guidance_param", "1"], "--guidance_drop needs guidance"),
            (base + ["--text_guidance_param", "2", "--guidance_drop", "text"], "exclude each other"),
            (base + ["--guidance_order", "text_seed"], "--guidance_order needs --text_guidance_param"),
            (base + ["--guidance_order", "text_seed", "--guidance_drop", "seed"], "--guidance_order needs --text_guidance_param"),
            (base + ["--text_guidance_param", "2", "--guidance_refresh", "2"], "runs no guidance refresh"),
            (base + ["--text_guidance_param", "2", "--layer_cache", "2", "1"], "runs no layer cache"),
            (base + ["--text_guidance_param", "2", "--parallel_window", "4"], "does not combine with --parallel_window"),
            (base + ["--guidance_drop", "none"], "invalid choice"),
            (base + ["--guidance_order", "text"], "invalid choice")):
        with pytest.raises(SystemExit):
            generate_args(argv)
        assert says in capsys.readouterr().err, argv
    from gesturediffusion_amd.sample.generate import sample_chunks
    for kw in (dict(text_guidance_param=2.0), dict(guidance_order="seed_text"), dict(guidance_drop="text")):
        with pytest.raises(ValueError, match="need guidance_param != 1"):
            sample_chunks(None, None, torch.zeros(1, 1, 1, 1), None, 0, 20, 10, guidance_param=1.0, **kw)
