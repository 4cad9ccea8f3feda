"""use_text models without a GPU: the CPU restatement (tests/text_restatement.py) against what the reference's own
MDM(use_text=True) computed (tests/golden/forward_text_tiny.npz, tools/make_golden_text.py), the drop-in surface of such a
model, and every refusal of the feature that needs no device -- gdx_create's, the two conditioning entries', the model's for
y, and the CLI's.  Tolerances are those tests/test_oracle_golden.py uses for the same quantities of the no-text model."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import text_restatement as tr
from conftest import GOLDEN, load_golden, rel_err
from genea_tree import GOLDEN_SEED_POSES, GOLDEN_TREE, GOLDEN_WINDOW, build_tree
from gesturediffusion_amd import _lib
from oracle import sampler as osamp
from oracle import schedule as osch


@pytest.fixture(scope="module")
def g():
    return load_golden("forward_text_tiny.npz")


# ------------------------------------------------------------------------------------------- the restatement vs the reference
@pytest.mark.parametrize("name", sorted(tr.CASES))
def test_restatement_forwards_equal_the_reference(g, name):
    cfg, sd, x, t, y = tr.case(g, name)
    with torch.no_grad():
        out = tr.forward(sd, cfg, x, t, y)
        un = tr.forward(sd, cfg, x, t, dict(y, uncond=True))
    assert rel_err(out, g[name + ".cond.out"]) < 2e-6
    assert rel_err(un, g[name + ".uncond.out"]) < 2e-6
    # against the reference run in fp64, in units of the reference's own fp32 round-off (test_oracle_golden.py::test_fp32_noise_floor)
    floor = rel_err(g[name + ".cond.out"], g[name + ".cond.out_fp64"])
    assert rel_err(out, g[name + ".cond.out_fp64"]) < 10 * max(floor, 1e-7)
    assert rel_err(out, un) > 1e-2                                    # the condition matters at these weights
    # uncond is the bias row whatever the inputs are
    other = dict(y, seed=y["seed"] + 1.0, text_embed=y["text_embed"] * 2.0, uncond=True)
    with torch.no_grad():
        assert torch.equal(tr.forward(sd, cfg, x, t, other), un)


def test_token0_rows_are_text_then_seed(g):
    """The fp64 rows the GPU test compares with: columns [0, text_dim) move with the text only, the rest with the seed only."""
    cfg, sd, x, t, y = tr.case(g, "mdm_128_t40")
    td = cfg["text_dim"]
    rows, cond = tr.token0_rows(sd, cfg, t, y["seed"], y["text_embed"])
    moved_text = tr.token0_rows(sd, cfg, t, y["seed"], y["text_embed"] + 1.0)[0]
    moved_seed = tr.token0_rows(sd, cfg, t, y["seed"] + 1.0, y["text_embed"])[0]
    assert torch.equal(moved_text[:, td:], rows[:, td:]) and not torch.equal(moved_text[:, :td], rows[:, :td])
    assert torch.equal(moved_seed[:, :td], rows[:, :td]) and not torch.equal(moved_seed[:, td:], rows[:, td:])
    bias = torch.cat((sd["embed_text.bias"], sd["seed_pose_encoder.seed_embed.bias"])).double()
    assert torch.equal(tr.token0_rows(sd, cfg, t, y["seed"], y["text_embed"], uncond=True)[1], bias.expand(3, -1))


def test_restatement_guided_loop_and_chunks_equal_the_reference(g):
    name = "mdm_128_t64"
    cfg, sd, x, t, y = tr.case(g, name)
    tab, tmap = osch.make_tables("cosine", 1000, tr.RESPACING)
    fn = lambda xx, tt, yy: tr.cfg_forward(sd, cfg, xx, tt, yy)          # noqa: E731
    tape = torch.from_numpy(g[name + ".cfg_p20.tape"])
    B = x.shape[0]
    with torch.no_grad():
        r = osamp.sample_loop(fn, tab, tmap, tuple(tape[0].shape), tape, dict(y, scale=torch.ones(B) * tr.SCALE), kind="p")
    assert rel_err(r, g[name + ".cfg_p20.out"]) < 2e-5
    # the chunk driver's three statements (oracle.sampler.sample_chunks) with a text per chunk
    sample_out = None
    for c in range(g[name + ".chunks.out"].shape[0]):
        yc = {"mfcc": torch.from_numpy(g[name + ".chunks.mfcc"][c]), "text_embed": torch.from_numpy(g[name + ".chunks.text"][c]),
              "seed": y["seed"] if c == 0 else sample_out[..., -cfg["seed_poses"]:], "scale": torch.ones(B) * tr.SCALE}
        tape = torch.from_numpy(g[name + ".chunks.tape"][c])
        with torch.no_grad():
            sample_out = osamp.sample_loop(fn, tab, tmap, tuple(tape[0].shape), tape, yc, kind="p")
        assert rel_err(sample_out, g[name + ".chunks.out"][c]) < 5e-5, c


# --------------------------------------------------------------------------------------------------------- drop-in surface
@pytest.mark.parametrize("J,d,td,cd", [(16, 128, 64, 512), (16, 128, 40, 32), (498, 256, 64, 512)])
def test_state_dict_keys_and_shapes_match_the_reference(J, d, td, cd):
    want = {}
    for line in open(os.path.join(GOLDEN, "state_dict_keys_text.txt")):
        _, j, dd, t, c, key, shape = line.split()
        if (int(j), int(dd), int(t), int(c)) == (J, d, td, cd):
            want[key] = tuple(int(s) for s in shape.split("x"))
    from gesturediffusion_amd.utils.init import init_state_dict, param_shapes
    layers, ff = (2, 1024) if J == 498 else (1, 192)
    cfg = tr.text_cfg(td, cd, J=J, d=d, layers=layers, ff=ff)
    m = tr.build_text_model(cfg, init_state_dict(cfg, seed=0))
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert want and got == want
    assert not hasattr(m, "clip_model") and len(m.parameters_wo_clip()) == len(list(m.parameters()))
    # init_state_dict covers exactly the parameters (the three buffers are the model's own)
    assert set(param_shapes(cfg)) == {k for k in want if not k.endswith(".pe") and not k.endswith("inv_freq")}
    named = m._engine_tensors()
    assert named["embed_text.weight"].shape == (td, cd) and named["seed_pose_encoder.seed_embed.bias"].shape == (d - td,)
    assert m._text_dims() == (td, cd)


def test_no_text_model_is_unchanged():
    from gesturediffusion_amd.utils.init import init_state_dict, param_shapes, synthetic_inputs
    cfg = {k: v for k, v in tr.text_cfg(0, 0).items() if k not in ("text_dim", "clip_dim")}
    assert "embed_text.weight" not in param_shapes(cfg) and param_shapes(cfg)["seed_pose_encoder.seed_embed.bias"] == (128,)
    assert len(synthetic_inputs(cfg, 2, 20)) == 3
    with_text = synthetic_inputs(tr.text_cfg(40, 32), 2, 20)
    assert with_text[3].shape == (2, 32) and all(torch.equal(a, b) for a, b in zip(with_text, synthetic_inputs(cfg, 2, 20)))
    sd, sdt = init_state_dict(cfg, seed=3), init_state_dict(tr.text_cfg(40, 32), seed=3)
    assert all(torch.equal(sd[k], sdt[k]) for k in sd if "seed_embed" not in k) and set(sdt) - set(sd) == {"embed_text.weight",
                                                                                                         "embed_text.bias"}


def test_load_model_wo_clip_and_model_args_for_a_text_checkpoint():
    """A checkpoint of a --use_text training run holds embed_text.* and the narrow seed encoder and no clip_model.* key."""
    from gesturediffusion_amd.utils.init import init_state_dict
    from gesturediffusion_amd.utils.model_util import create_model_and_diffusion, load_model_wo_clip
    from gesturediffusion_amd.utils.parser_util import generate_args
    args = generate_args(["--synthetic", "--use_text", "--mfcc_input", "--dataset", "genea2023", "--layers", "1", "--latent_dim", "128"])
    model, _ = create_model_and_diffusion(args, None)
    assert model.use_text and model._text_dims() == (64, 512) and model.seed_pose_encoder.seed_embed.out_features == 64
    cfg = tr.text_cfg(64, 512, J=498, ff=1024)
    sd = {k: v.clone() for k, v in create_model_and_diffusion(args, None)[0].state_dict().items()}     # buffers included
    sd.update({k: v + 0.5 for k, v in init_state_dict(cfg, seed=4).items()})
    assert not any(k.startswith("clip_model.") for k in sd)
    load_model_wo_clip(model, sd)
    got = model.state_dict()
    assert all(torch.equal(got[k], v) for k, v in sd.items())
    with pytest.raises(AssertionError, match="unexpected"):
        load_model_wo_clip(model, dict(sd, **{"clip_model.positional_embedding": torch.zeros(1)}))
    with pytest.raises(AssertionError, match="lacks"):
        load_model_wo_clip(model, {k: v for k, v in sd.items() if not k.startswith("embed_text.")})
    plain = create_model_and_diffusion(generate_args(["--synthetic", "--mfcc_input", "--dataset", "genea2023", "--layers", "1", "--latent_dim", "128"]),
                                       None)[0]
    with pytest.raises((AssertionError, RuntimeError)):                # a text checkpoint does not load into a no-text model
        load_model_wo_clip(plain, sd)


def test_text_dim_must_stay_below_latent_dim():
    from gesturediffusion_amd.model.mdm_old import MDM_Old
    for td in (128, 200, 0, -1):
        with pytest.raises(NotImplementedError):
            tr.build_text_model(tr.text_cfg(td, 512), {})
    old = MDM_Old(njoints=16, nfeats=1, translation=True, pose_rep="rot6d", glob=True, glob_rot=True, latent_dim=64, num_layers=1,
                  data_rep="genea_vec", cond_mask_prob=0.1, use_text=True, seed_poses=10)
    assert old._text_dims() == (0, 0) and "embed_text.weight" not in old.state_dict()


# --------------------------------------------------------------------------------------------------------------- the C ABI
def _cfg(**over):
    kw = dict(arch=_lib.GDX_ARCH_MDM, njoints=16, latent_dim=128, ff_size=192, num_layers=1, num_heads=4, seed_poses=10,
              mfcc_dim=26, cl_head=8, window=10, compute_dtype=0, text_dim=64, clip_dim=512)
    kw.update(over)
    return _lib.Config(**kw)


@pytest.mark.parametrize("over,says", [
    (dict(text_dim=-1), b"text_dim must not be negative"),
    (dict(arch=_lib.GDX_ARCH_MDM_OLD), b"MDM_Old has no text path"),
    (dict(text_dim=128), b"text_dim must be smaller than latent_dim"),
    (dict(text_dim=129), b"text_dim must be smaller than latent_dim"),
    (dict(clip_dim=0), b"needs clip_dim > 0"),
    (dict(clip_dim=-3), b"needs clip_dim > 0"),
    (dict(text_dim=0), b"clip_dim without text_dim"),
    (dict(text_dim=0, clip_dim=-1), b"clip_dim without text_dim"),
])
def test_gdx_create_refusals(over, says):
    """Each refusal comes before gdx_create touches a device, so it fires on a machine without one."""
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.gdx_create(C.byref(_cfg(**over)), C.byref(h)) != 0 and not h.value
    assert says in lib.gdx_last_error(), lib.gdx_last_error()


def test_config_ends_in_the_two_text_fields_and_zero_means_no_text():
    names = [f for f, _ in _lib.Config._fields_]
    assert names[-2:] == ["text_dim", "clip_dim"] and names.index("compute_dtype") == len(names) - 3
    old = _lib.Config(arch=1, njoints=16, latent_dim=128, ff_size=256, num_layers=2, num_heads=4, seed_poses=10, mfcc_dim=26)
    assert (old.text_dim, old.clip_dim) == (0, 0)
    assert [t for t, _ in _lib.HEADER.prototypes["gdx_set_condition_text"][1]] == [
        "gdx_handle_t", "const float*", "const float*", "const float*", "void*"]


def test_condition_entries_refuse_the_other_kind_of_handle():
    from gesturediffusion_amd.engine import Engine, GdxError, check_condition_entry
    lib = _lib.load()
    null = C.c_void_p()
    for fn, args in ((lib.gdx_set_condition_text, (null, null, null, null, null)), (lib.gdx_set_condition, (null, null, null, null))):
        assert fn(*args) != 0 and b"null argument" in lib.gdx_last_error()
    check_condition_entry(0, False)
    check_condition_entry(64, True)
    with pytest.raises(GdxError, match="gdx_set_condition_text"):
        check_condition_entry(64, False)
    with pytest.raises(GdxError, match=r"no text \(text_dim = 0\): call gdx_set_condition "):
        check_condition_entry(0, True)
    # through Engine.set_condition, before it looks at a tensor: a handle-less Engine is enough
    eng = Engine.__new__(Engine)
    eng.cfg, eng._cond_key = _cfg(), None
    cpu = torch.zeros(1)
    with pytest.raises(GdxError, match="gdx_set_condition_text"):
        eng.set_condition(cpu, cpu)
    eng.cfg = _cfg(text_dim=0, clip_dim=0)
    with pytest.raises(GdxError, match="call gdx_set_condition "):
        eng.set_condition(cpu, cpu, text=cpu)
    h = C.c_void_p()
    if lib.gdx_create(C.byref(_cfg()), C.byref(h)) == 0:          # where a handle can be made without a device
        one = C.c_void_p(16)
        assert lib.gdx_set_condition(h, one, one, None) != 0 and b"call gdx_set_condition_text" in lib.gdx_last_error()
        assert lib.gdx_set_condition_text(h, one, one, one, None) != 0 and b"missing weights" in lib.gdx_last_error()
        assert b"embed_text.weight, embed_text.bias" in lib.gdx_last_error()
        lib.gdx_destroy(h)


# ---------------------------------------------------------------------------------------------------------------- y errors
def test_text_features_of_y():
    from gesturediffusion_amd._lib import GdxError
    cfg = tr.text_cfg(40, 32)
    from gesturediffusion_amd.utils.init import init_state_dict
    m = tr.build_text_model(cfg, init_state_dict(cfg, seed=1))
    with pytest.raises(KeyError, match="text"):
        m._text_features({"seed": 0}, 2)
    with pytest.raises(NotImplementedError, match=r"text_embed.*set_text_encoder"):
        m._text_features({"text": ["a", "b"]}, 2)
    with pytest.raises(GdxError, match=r"y\['text_embed'\] is on cpu"):
        m._text_features({"text_embed": torch.zeros(2, 32)}, 2)
    with pytest.raises(TypeError):
        m._text_features({"text_embed": [[0.0] * 32] * 2}, 2)
    seen = []
    m.set_text_encoder(lambda texts: seen.append(texts) or torch.zeros(len(texts), 32))
    with pytest.raises(GdxError, match="is on cpu"):                     # the encoder ran; its host tensor is refused like any
        m._text_features({"text": ("a", "b")}, 2)
    assert seen == [["a", "b"]] and "text_encoder" not in dict(m.named_modules()) and "text_encoder" not in m.state_dict()
    with pytest.raises(TypeError):
        m.set_text_encoder("ViT-B/32")
    m.set_text_encoder(None)
    with pytest.raises(NotImplementedError):
        m._text_features({"text": ["a", "b"]}, 2)
    for bad, err in ((torch.zeros(2, 31), r"\[2, 32\], got \[2, 31\]"), (torch.zeros(3, 32), "got"), (torch.zeros(2, 32, 1), "got"),
                     (torch.zeros(2, 32, dtype=torch.int64), "floating")):
        with pytest.raises(ValueError, match=err):
            m._text_features({"text_embed": bad}, 2)
    # a model without text ignores both keys
    from gesturediffusion_amd.model.mdm import MDM
    plain = MDM(njoints=16, nfeats=1, pose_rep="rot6d", data_rep="genea_vec", latent_dim=64, num_layers=1, mfcc_input=True, seed_poses=10)
    assert plain._text_features({"text": ["a"], "text_embed": None}, 1) is None


# --------------------------------------------------------------------------------------------------------------------- CLI
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return build_tree(str(tmp_path_factory.mktemp("genea_text")), **GOLDEN_TREE)


DATA = ["--dataset", "genea2023", "--num_frames", str(GOLDEN_WINDOW), "--seed_poses", str(GOLDEN_SEED_POSES), "--num_samples", "3",
        "--chunks", "1"]


def test_cli_needs_text_features_on_a_data_directory(tree, capsys):
    from gesturediffusion_amd.utils.parser_util import generate_args
    with pytest.raises(SystemExit):
        generate_args(DATA + ["--data_dir", tree, "--use_text"])
    assert "--text_features FILE.npz" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        generate_args(["--synthetic", "--use_text", "--list_texts", "x.txt"])
    a = generate_args(DATA + ["--data_dir", tree, "--use_text", "--text_features", "f.npz"])
    assert a.use_text and a.text_features == "f.npz" and a.list_texts == ""
    assert generate_args(["--synthetic", "--use_text"]).use_text                      # synthetic features need no file
    assert generate_args(DATA + ["--data_dir", tree, "--use_text", "--arch_version", "mdm_old"]).use_text   # MDM_Old has no text path
    assert generate_args(DATA + ["--data_dir", tree]).text_features == ""


def test_list_texts_and_lookup(tree, tmp_path, capsys):
    """--list_texts writes the run's distinct strings without a GPU; a features file made from that list resolves every
    (take, chunk) string, the empty one included, and a file that lacks some is refused with their number and the first few."""
    from gesturediffusion_amd.data_loaders.gesture.data.dataset import Genea2023
    from gesturediffusion_amd.sample import generate
    out = tmp_path / "texts.txt"
    assert generate.main(DATA + ["--data_dir", tree, "--use_text", "--list_texts", str(out)]) == 0
    ds = Genea2023(split="val", datapath=tree, window=GOLDEN_WINDOW, n_seed_poses=GOLDEN_SEED_POSES)
    index = generate.chunk_items(ds.samples_cumulative, 3, 1)
    texts = generate.run_texts(ds, index)
    assert texts == [[ds.text_window(*ds.locate(i)) for i in index[0]]] and len(texts[0]) == 3
    lines = out.read_text().split("\n")
    assert lines[-1] == "" and lines[:-1] == generate.distinct(texts) and len(set(lines[:-1])) == len(lines[:-1])
    assert "distinct texts" in capsys.readouterr().out
    # every window of the split, so that the empty string (a window without words) is among the keys if the tree has one
    every = [[ds.text_window(*ds.locate(i)) for i in range(len(ds))] + [""]]
    keys = generate.distinct(every)
    assert "" in keys
    rng = np.random.default_rng(0)
    feats = rng.normal(size=(len(keys), 8)).astype(np.float32)
    path = str(tmp_path / "features.npz")
    np.savez(path, text=np.array(keys), features=feats)
    got = generate.lookup_text_features(path, every, 8)
    assert got.dtype == torch.float32 and got.shape == (1, len(every[0]), 8)
    for k, t in enumerate(every[0]):
        assert np.array_equal(got[0, k].numpy(), feats[keys.index(t)]), t
    # refusals
    short = str(tmp_path / "short.npz")
    np.savez(short, text=np.array(keys[2:]), features=feats[2:])
    with pytest.raises(ValueError, match=rf"^2 of the run's {len(keys)} texts are not in .*short.npz; the first: \[") as e:
        generate.lookup_text_features(short, every, 8)
    assert repr(keys[0]) in str(e.value) and repr(keys[1]) in str(e.value)
    with pytest.raises(ValueError, match=r"`features` must be \[\d+, 16\]"):
        generate.lookup_text_features(path, every, 16)
    np.savez(short, text=np.array(keys))
    with pytest.raises(ValueError, match="must hold the arrays `text` and `features`"):
        generate.lookup_text_features(short, every, 8)


def test_synthetic_text_features_come_from_the_seed():
    from gesturediffusion_amd.sample.generate import synthetic_text_features
    a, b = synthetic_text_features(7, 3, 512, 2), synthetic_text_features(7, 3, 512, 2)
    assert len(a) == 2 and a[0].shape == (3, 512) and all(torch.equal(p, q) for p, q in zip(a, b))
    assert not torch.equal(a[0], a[1]) and not torch.equal(a[0], synthetic_text_features(8, 3, 512, 2)[0])
