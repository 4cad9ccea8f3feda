"""The GENEA 2023 data path on the GPU: items of `Genea2023` with their device MFCCs, and `sample.generate --dataset genea2023
--data_dir ...` end to end against a direct `sample_chunks` call on inputs assembled by hand from the dataset's host methods
(which tests/test_genea_data_host.py pins to the reference's items), against the CPU oracle's chunk loop, and in fp16.
Trees come from tests/genea_tree.py.  Need an MI355X.

Tolerances are existing ones: 2e-4 for the MFCC front end (test_mfcc_front_end_vs_restated_package), LOOP_TOL for fp32 loops
against the oracle (tests/test_gpu_parity.py), numerics.stated_tolerance for fp16 under guidance."""
import os

import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err
from genea_tree import GOLDEN_SEED_POSES, GOLDEN_TREE, GOLDEN_WINDOW, MFCC_DIM, build_tree
from gesturediffusion_amd.numerics import stated_tolerance
from test_gpu_parity import LOOP_TOL, dev

pytestmark = pytest.mark.gpu

J, T, P, TAKES, CHUNKS, SEED, SCALE = 498, 20, 4, 3, 2, 10, 2.5          # SEED: the CLI's default --seed
FRAMES_VAL = [95, 70, 130]                                               # 3, 2 and 5 windows of 20 frames
ITEMS = [[0, 3, 5], [1, 4, 6]]                                           # item of (chunk, take): first item of a take + chunk


@pytest.fixture(scope="module")
def small_tree(tmp_path_factory):
    return build_tree(str(tmp_path_factory.mktemp("genea12")), **GOLDEN_TREE)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return build_tree(str(tmp_path_factory.mktemp("genea498")), J=J, frames_trn=[64], frames_val=FRAMES_VAL, seed=498, zero_std_at=7)


def open_val(tree, window=T, seed_poses=P):
    from gesturediffusion_amd.data_loaders.gesture.data.dataset import Genea2023
    return Genea2023(split="val", datapath=tree, window=window, n_seed_poses=seed_poses, device=dev())


def test_items_carry_device_mfccs(small_tree):
    """The first and the last 'val' item: five fields as the reference returned them, `mfcc` an fp32 device tensor [20, 26]
    within 2e-4 of oracle/mfcc.py on the same window and statistics."""
    from oracle import mfcc as om
    g = load_golden("genea2023_items.npz")
    ds = open_val(small_tree, GOLDEN_WINDOW, GOLDEN_SEED_POSES)
    for idx in (0, len(ds) - 1):
        motion, text, window, audio, mfcc, seed = ds[idx]
        assert motion.dtype == np.float64 and np.array_equal(motion, g["val.motion"][idx])
        assert seed.dtype == np.float64 and np.array_equal(seed, g["val.seed_poses"][idx])
        assert text == str(g["val.text"][idx]) and window == GOLDEN_WINDOW
        take, sample = ds.locate(idx)
        assert audio.dtype == np.float32 and np.array_equal(audio, ds.audio_window(take, sample))
        assert audio.shape == (int(g["val.audio"][idx][1]),)
        assert mfcc.device == dev() and mfcc.dtype == torch.float32 and tuple(mfcc.shape) == (GOLDEN_WINDOW, MFCC_DIM)
        want = om.genea_mfcc(audio.astype(np.float64), ds.sr, ds.fps, ds.mfcc_mean, ds.mfcc_std)
        err = rel_err(mfcc.cpu(), want)
        print(f"[genea-measure] item {idx}: mfcc rel err {err:.2e}")
        assert err < 2e-4


# ------------------------------------------------------------------------------------------------------------------ CLI
def argv_for(tree, out, arch, dtype):
    return ["--dataset", "genea2023", "--data_dir", tree, "--num_frames", str(T), "--seed_poses", str(P), "--latent_dim", "128",
            "--layers", "2", "--num_samples", str(TAKES), "--chunks", str(CHUNKS), "--sampler", "ddim", "--timestep_respacing",
            "ddim10", "--rng", "philox", "--guidance_param", str(SCALE), "--output_dir", out, "--arch_version", arch,
            "--compute_dtype", dtype]


@pytest.fixture(scope="module")
def cli(tree, tmp_path_factory):
    """results.npy of one CLI run per (arch, dtype), shared by the tests (read only)."""
    from gesturediffusion_amd.sample import generate
    done = {}

    def run(arch, dtype="fp32"):
        if (arch, dtype) not in done:
            out = str(tmp_path_factory.mktemp(f"out_{arch}_{dtype}"))
            assert generate.main(argv_for(tree, out, arch, dtype)) == 0
            res = np.load(os.path.join(out, "results.npy"), allow_pickle=True).item()      # written a moment ago
            done[(arch, dtype)] = (out, res)
        return done[(arch, dtype)]
    return run


@pytest.fixture(scope="module")
def by_hand(tree):
    """The inputs of the same run assembled from the dataset's host methods and MfccExtractor, and a direct sample_chunks
    call on them: (dataset, first seed, MFCCs per chunk, collated ground truth per chunk, model, diffusion, chunk outputs)
    per arch."""
    from gesturediffusion_amd.data_loaders.mfcc import MfccExtractor
    from gesturediffusion_amd.data_loaders.tensors import gg_collate
    from gesturediffusion_amd.model.cfg_sampler import ClassifierFreeSampleModel
    from gesturediffusion_amd.sample.generate import sample_chunks
    from gesturediffusion_amd.utils.init import init_state_dict
    from gesturediffusion_amd.utils.model_util import create_model_and_diffusion
    from gesturediffusion_amd.utils.parser_util import generate_args
    d = dev()
    ds = open_val(tree)
    assert ds.samples_per_file == [3, 2, 5]
    ex = MfccExtractor(d, sr=ds.sr, fps=ds.fps, mfcc_mean=ds.mfcc_mean, mfcc_std=ds.mfcc_std)
    seeds, mfccs, truth = [], [], []
    for row in ITEMS:
        where = [ds.locate(i) for i in row]
        windows = [ds.motion_window(*w) for w in where]
        audio = [ds.audio_window(*w) for w in where]
        seeds.append(torch.stack([torch.from_numpy(s).t().float().unsqueeze(1) for _, s in windows]))          # [3, J, 1, P]
        mfccs.append(torch.stack([ex(torch.from_numpy(a).to(d)).t().unsqueeze(1) for a in audio]).contiguous())  # [3, 26, 1, T]
        truth.append(gg_collate([(m, ds.text_window(*w), T, a, torch.zeros(T, MFCC_DIM), s)
                                 for w, (m, s), a in zip(where, windows, audio)]))
    done = {}

    def run(arch):
        if arch not in done:
            args = generate_args(argv_for(tree, "unused", arch, "fp32"))
            args.mfcc_input = True
            model, df = create_model_and_diffusion(args, None)
            assert df.num_timesteps == 10 and model.njoints == J
            cfg = dict(arch=arch, njoints=J, nfeats=1, latent_dim=128, ff_size=1024, num_layers=2, num_heads=4, seed_poses=P)
            sd = init_state_dict(cfg, seed=SEED)
            model.load_state_dict(sd, strict=False)
            model = ClassifierFreeSampleModel(model).to(d).eval()
            outs = sample_chunks(model, df, seeds[0].to(d), lambda c: mfccs[c], CHUNKS, T, P, guidance_param=SCALE,
                                 sampler="ddim", rng="philox", philox_seed=SEED)
            done[arch] = (cfg, sd, model, df, [o.clone() for o in outs])
        return done[arch]
    return ds, seeds, mfccs, truth, run


@pytest.mark.parametrize("arch", ["mdm", "mdm_old"])
def test_generate_cli_on_a_data_directory(tree, cli, by_hand, arch):
    """`sample.generate --dataset genea2023 --data_dir <tree>`: the saved motion is bit-equal to a direct sample_chunks +
    postprocess call on hand-assembled inputs, the ground truth to the postprocessed collation, text / lengths / takes /
    audio are the tree's, chunk 1 continues chunk 0's last frames."""
    from gesturediffusion_amd import engine as E
    out, res = cli(arch)
    ds, seeds, mfccs, truth, run = by_hand
    cfg, sd, model, df, outs = run(arch)
    d = dev()
    tails = [E.postprocess(o, ds.mean, ds.std) for o in outs]
    assert res["motion"].shape == res["motion_rot"].shape == (TAKES, J // 6, 3, CHUNKS * T)
    assert np.array_equal(res["motion"], np.concatenate([p.cpu().numpy() for p, _ in tails], axis=3))
    assert np.array_equal(res["motion_rot"], np.concatenate([r.cpu().numpy() for _, r in tails], axis=3))
    assert np.isfinite(res["motion"]).all() and np.abs(res["motion"]).max() > 0
    gts = [E.postprocess(m.to(d), ds.mean, ds.std) for m, _ in truth]
    assert np.array_equal(res["gt_motion"], np.concatenate([p.cpu().numpy() for p, _ in gts], axis=3))
    assert np.array_equal(res["gt_motion_rot"], np.concatenate([r.cpu().numpy() for _, r in gts], axis=3))
    # the ground truth is the takes' own first 40 frames, de-normalised: the z-score undone to fp32 round-off
    raw = np.stack([np.load(os.path.join(ds.motionpath, ds.takes[k][0] + ".npy"))[: CHUNKS * T] for k in range(TAKES)])
    pos_cols = np.asarray([[6 * j + 3, 6 * j + 4, 6 * j + 5] for j in range(J // 6)])
    assert np.allclose(res["gt_motion"], raw[:, :, pos_cols].transpose(0, 2, 3, 1), rtol=1e-5, atol=1e-5)
    assert res["num_samples"] == TAKES and res["num_chunks"] == CHUNKS
    assert res["text"] == [t for _, c in truth for t in c["y"]["text"]] and len(res["text"]) == TAKES * CHUNKS
    assert np.array_equal(res["lengths"], np.full(TAKES * CHUNKS, T))
    assert res["takes"] == [f"val_2023_v0_{k:03d}_main-agent" for k in range(TAKES)]
    whole = np.stack([np.load(os.path.join(ds.audiopath, name + ".npy"))[: CHUNKS * T * 735] for name in res["takes"]])
    assert res["audio"].dtype == np.float32 and np.array_equal(res["audio"], whole)
    with open(os.path.join(out, "results.txt")) as f:                     # both written by the run above
        assert f.read() == "\n".join(res["text"])
    with open(os.path.join(out, "results_len.txt")) as f:
        assert f.read() == "\n".join([str(T)] * (TAKES * CHUNKS))
    # seed hand-off: chunk 1 is one loop on chunk 0's last P frames, chunk 1's MFCCs and chunk 1's noise key
    y = {"seed": outs[0][..., -P:].clone(), "mfcc": mfccs[1], "scale": torch.ones(TAKES, device=d) * SCALE}
    alone = df.ddim_sample_loop(model, (TAKES, J, 1, T), clip_denoised=False, model_kwargs={"y": y}, rng="philox",
                                philox_seed=SEED + 1000)
    pos, rot = E.postprocess(alone, ds.mean, ds.std)
    assert np.array_equal(res["motion"][..., T:], pos.cpu().numpy()) and np.array_equal(res["motion_rot"][..., T:], rot.cpu().numpy())
    assert not torch.equal(outs[0][..., -P:].cpu(), seeds[1])              # and not the data's own seed poses of chunk 1


def normalised(res, ds):
    """results.npy's positions and rotations back as the sampler's [B, J, 1, T] (the tail undone in fp64)."""
    x = np.empty((TAKES, J, 1, CHUNKS * T))
    for j in range(J // 6):
        x[:, 6 * j: 6 * j + 3, 0] = res["motion_rot"][:, j]
        x[:, 6 * j + 3: 6 * j + 6, 0] = res["motion"][:, j]
    return (x - ds.mean[None, :, None, None]) / ds.std[None, :, None, None]


def test_data_chunks_vs_oracle(by_hand):
    """The same two chunks through the oracle's chunk loop on the CPU (x_T from the library's counter-based generator, the
    device MFCCs copied to the host; DDIM at eta 0 uses no further noise), fp32, at LOOP_TOL."""
    from gesturediffusion_amd import engine as E
    from oracle import mdm_forward as omf
    from oracle import sampler as osamp
    from oracle import schedule as osch
    ds, seeds, mfccs, truth, run = by_hand
    cfg, sd, model, df, outs = run("mdm")
    tab, tmap = osch.make_tables("cosine", 1000, "ddim10")
    shape = (TAKES, J, 1, T)
    tapes = [[E.randn(shape, dev(), SEED + 1000 * c, 0, 0).cpu()] + [torch.zeros(shape)] * 10 for c in range(CHUNKS)]
    with torch.no_grad():
        want = osamp.sample_chunks(lambda x, t, y: omf.cfg_forward(sd, cfg, x, t, y), tab, tmap, seeds[0],
                                   [m.cpu() for m in mfccs], tapes, P, scale=SCALE, kind="ddim")
    for c, (got, ref) in enumerate(zip(outs, want)):
        err = rel_err(got.cpu(), ref)
        print(f"[genea-measure] chunk {c} vs oracle: rel err {err:.2e}")
        assert err < LOOP_TOL, c


def test_generate_cli_on_a_data_directory_fp16(cli, by_hand):
    """The same command with --compute_dtype fp16 against its fp32 result, in the sampler's normalised units, at the
    mode's stated loop tolerance under guidance 2.5."""
    ds = by_hand[0]
    r32, r16 = cli("mdm")[1], cli("mdm", "fp16")[1]
    assert r16["text"] == r32["text"] and np.array_equal(r16["gt_motion"], r32["gt_motion"])
    assert not np.array_equal(r16["motion"], r32["motion"])
    err = rel_err(normalised(r16, ds), normalised(r32, ds))
    print(f"[genea-measure] fp16 CLI vs fp32 CLI: rel err {err:.2e}")
    assert err < stated_tolerance("fp16", SCALE, loop=True)
