#!/usr/bin/env python3
"""Generate tests/golden/forward_text_tiny.npz and state_dict_keys_text.txt by running the REFERENCE's MDM(use_text=True).

Development-machine tool: imports the reference at run time through the shims of oracle/tools/make_golden.py (never
copied) and writes DATA only -- inputs, recorded text features and the reference's outputs.  The weights come from
init_state_dict(cfg, seed, perturb=True) on both sides, so the file holds none.

The reference computes its text features with CLIP (model/mdm.py:229-240,252-267), whose weights are not to be had here.  The
stub `clip` module of the shims therefore gets a stand-in that leaves every line of the reference's text path running:
  clip.load(...)                 -> a tiny module whose encode_text(tokens) returns table[tokens[:, 0]]
  clip.model.convert_weights(m)  -> nothing
  clip.tokenize(texts, ...)      -> int64 [B, 77], a string's index in the recorded list in column 0
so that encode_text(y['text']) yields the recorded feature vectors, and mask_cond, embed_text, the narrower seed encoder, the
concatenation and everything behind it are the reference's own.

Cases (16 joints, one layer, ff_size 192, seed_poses 10, latent_dim 128, T = 20, t = [7, 993]):
  mdm_128_t64   text_dim 64, clip_dim 512, B = 2: <case>.cond.out, .uncond.out, .cond.out_fp64
  mdm_128_t40   text_dim 40, clip_dim 32,  B = 3 (t = [7, 993, 500]): the same three
  mdm_128_t64.cfg_p20   p_sample_loop on [20] steps under ClassifierFreeSampleModel at scale 2.5, noise tape .cfg_p20.tape
  mdm_128_t64.chunks    two chunks through the three chunk statements of sample/generate.py:91-130 (as chunks_tiny.npz), each
                        chunk with its own text features / MFCCs / tape: .chunks.text, .chunks.mfcc, .chunks.tape, .chunks.out
Inputs per case: <case>.x / .seed / .mfcc / .t / .text (the features [B, clip_dim]).

state_dict_keys_text.txt lists `mdm_text J latent_dim text_dim clip_dim key shape` of the reference's module without its
clip_model.* entries, which its trainer strips from every checkpoint (train/training_loop.py:269-272).

The archive is written with fixed zip timestamps: the same machine regenerates it byte for byte.

Usage:  python tools/make_golden_text.py --ref <checkout of the reference> [--out tests/golden]
"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle", "tools"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import make_golden as mg  # noqa: E402
from make_golden_bpd import save_npz  # noqa: E402
from gesturediffusion_amd.utils.init import init_state_dict, synthetic_inputs  # noqa: E402

CASES = {"mdm_128_t64": (64, 512, 2), "mdm_128_t40": (40, 32, 3)}          # text_dim, clip_dim, B
WEIGHT_SEED, INPUT_SEED, T = 21, 23, 20
LOOP = dict(respacing=[20], scale=2.5, tape_seed=2468, n_chunks=2)


def text_cfg(text_dim, clip_dim, J=16, d=128, layers=1, ff=192):
    return dict(arch="mdm", njoints=J, nfeats=1, latent_dim=d, ff_size=ff, num_layers=layers, num_heads=4, seed_poses=10,
                text_dim=text_dim, clip_dim=clip_dim)


class Recorded:
    """The stand-in the stub `clip` module serves: strings "0", "1", ... name the rows of `table`."""

    def __init__(self):
        self.table = torch.zeros(1, 1)

    def install(self, clip):
        recorded = self

        class Tower(torch.nn.Module):
            def encode_text(self, tokens):
                return recorded.table[tokens[:, 0]]

        def tokenize(texts, context_length=77, truncate=False):
            tokens = torch.zeros(len(texts), context_length, dtype=torch.long)
            tokens[:, 0] = torch.tensor([int(t) for t in texts])
            return tokens
        clip.load = lambda version, device="cpu", jit=False: (Tower(), None)
        clip.model = type(sys)("clip.model")
        clip.model.convert_weights = lambda m: None
        clip.tokenize = tokenize

    def names(self, feats):
        self.table = feats
        return [str(i) for i in range(feats.shape[0])]


def build_ref_text_model(mods, cfg, sd, double=False):
    kw = dict(njoints=cfg["njoints"], nfeats=cfg["nfeats"], translation=True, pose_rep="rot6d", glob=True, glob_rot=True,
              latent_dim=cfg["latent_dim"], text_dim=cfg["text_dim"], clip_dim=cfg["clip_dim"], ff_size=cfg["ff_size"],
              num_layers=cfg["num_layers"], num_heads=cfg["num_heads"], dropout=0.1, activation="gelu", data_rep="genea_vec",
              cond_mask_prob=0.1, dataset="genea2023", use_text=True, mfcc_input=True, use_wav_enc=False,
              seed_poses=cfg["seed_poses"], use_audio=False, modeltype="", clip_version="ViT-B/32")
    m = mg.quiet(mods[0].MDM, **kw)
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    assert all(k.endswith(".pe") or k.endswith("inv_freq") or k.startswith("clip_model.") for k in missing), missing
    m.eval()
    if double:
        m.double()                     # in place: the reference's _apply override returns None
    return m


def gen(mods, out):
    ref_cfg, gd, rs = mods[2], mods[3], mods[4]
    rec = Recorded()
    rec.install(sys.modules["clip"])
    d, keys = {}, []
    for name, (td, cd, B) in CASES.items():
        cfg = text_cfg(td, cd)
        sd = init_state_dict(cfg, seed=WEIGHT_SEED, perturb=True)
        x, seedp, mfcc, text = synthetic_inputs(cfg, B, T, seed=INPUT_SEED)
        t = torch.tensor([7, 993, 500][:B])
        m = build_ref_text_model(mods, cfg, sd)
        keys += [f"mdm_text {cfg['njoints']} {cfg['latent_dim']} {td} {cd} {k} {'x'.join(str(i) for i in v.shape)}"
                 for k, v in m.state_dict().items() if not k.startswith("clip_model.")]
        y = {"seed": seedp, "mfcc": mfcc, "text": rec.names(text)}
        d.update({f"{name}.x": x.numpy(), f"{name}.seed": seedp.numpy(), f"{name}.mfcc": mfcc.numpy(), f"{name}.t": t.numpy(),
                  f"{name}.text": text.numpy()})
        with torch.no_grad():
            d[f"{name}.cond.out"] = m(x, t, y).contiguous().numpy()
            d[f"{name}.uncond.out"] = m(x, t, dict(y, uncond=True)).contiguous().numpy()
            # fp64: the reference's encode_text ends in .float(), which a double embed_text cannot take; the harness hands the
            # same recorded rows over in fp64 instead
            m64 = build_ref_text_model(mods, cfg, sd, double=True)
            m64.encode_text = lambda raw: text.double()[[int(s) for s in raw]]
            d[f"{name}.cond.out_fp64"] = m64(x.double(), t, {"seed": seedp.double(), "mfcc": mfcc.double(),
                                                             "text": y["text"]}).contiguous().numpy()
        if name != "mdm_128_t64":
            continue
        guided = ref_cfg.ClassifierFreeSampleModel(m)
        df = mg.make_diffusion(gd, rs, LOOP["respacing"])
        shape = (B, cfg["njoints"], 1, T)
        g = torch.Generator().manual_seed(LOOP["tape_seed"])
        scale = torch.ones(B) * LOOP["scale"]
        tape = torch.randn(LOOP["respacing"][0] + 1, *shape, generator=g)
        with mg.TapeNoise(tape[1:]):
            r = df.p_sample_loop(guided, shape, noise=tape[0].clone(), clip_denoised=False, progress=False,
                                 model_kwargs={"y": dict(y, scale=scale)})
        d.update({f"{name}.cfg_p20.tape": tape.numpy(), f"{name}.cfg_p20.out": r.numpy()})
        # the chunk loop: the three statements of sample/generate.py:91-130 around the reference's own p_sample_loop
        n = LOOP["n_chunks"]
        texts = torch.randn(n, B, cd, generator=g)
        mfccs = torch.randn(n, B, 26, 1, T, generator=g)
        tapes = torch.randn(n, LOOP["respacing"][0] + 1, *shape, generator=g)
        outs, sample_out = [], None
        for chunk in range(n):
            yc = {"mfcc": mfccs[chunk], "seed": seedp, "text": rec.names(texts[chunk])}
            if chunk > 0:
                yc["seed"] = sample_out[..., -cfg["seed_poses"]:]
            yc["scale"] = torch.ones(B) * LOOP["scale"]
            with mg.TapeNoise(tapes[chunk][1:]):
                sample_out = df.p_sample_loop(guided, shape, clip_denoised=False, model_kwargs={"y": yc}, skip_timesteps=0,
                                              init_image=None, progress=False, dump_steps=None,
                                              noise=tapes[chunk][0].clone(), const_noise=False)
            outs.append(sample_out)
        d.update({f"{name}.chunks.text": texts.numpy(), f"{name}.chunks.mfcc": mfccs.numpy(),
                  f"{name}.chunks.tape": tapes.numpy(), f"{name}.chunks.out": torch.stack(outs).numpy()})
    # the GENEA width too: what a --use_text training run's checkpoint holds
    cfg = text_cfg(64, 512, J=498, d=256, layers=2, ff=1024)
    m = build_ref_text_model(mods, cfg, init_state_dict(cfg, seed=0))
    keys += [f"mdm_text 498 256 64 512 {k} {'x'.join(str(i) for i in v.shape)}" for k, v in m.state_dict().items()
             if not k.startswith("clip_model.")]
    for k, v in d.items():
        assert np.isfinite(v).all(), k
    path = os.path.join(out, "forward_text_tiny.npz")
    save_npz(path, d)
    with open(os.path.join(out, "state_dict_keys_text.txt"), "w") as f:
        f.write("\n".join(keys) + "\n")
    return path


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    torch.set_num_threads(8)
    path = gen(mg.import_reference(args.ref), args.out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
