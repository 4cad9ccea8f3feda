"""CPU restatement of MDM(use_text=True) (reference model/mdm.py:36-50, 118-127, 154-160) on top of the unchanged oracle
(oracle/mdm_forward.py), which knows no text.  Test infrastructure; pinned by tests/golden/forward_text_tiny.npz, which the
reference's own class wrote (tools/make_golden_text.py).

A text model is a no-text model whose seed encoder is block-diagonal over [text features | flat seed]:

    coa - emb_t = [embed_text(text) | seed_embed(flat_seed)] = W_fold [text | flat_seed] + [b_text | b_seed]
    W_fold = [[W_text, 0], [0, W_seed]]          ([latent_dim][clip_dim + njoints * seed_poses])

and `uncond` zeroes both inputs, which leaves the bias row in either form.  The oracle flattens y['seed'] [B, J, 1, P] joint by
joint, so for clip_dim = J * E the features ride along as E extra "poses" per joint -- y['seed'] becomes [B, J, 1, P + E] with
text[b, j * E + e] at pose P + e of joint j -- and W_fold's columns are permuted to that flatten order.  The only arithmetic
this adds to the oracle's is products with exact zeros."""
import torch

from oracle import mdm_forward as omf


def fold_weights(sd, cfg):
    """State dict and cfg of the equivalent no-text model (same tensors, one wider seed encoder in embed_text's place)."""
    td, cd, J, P, d = cfg["text_dim"], cfg["clip_dim"], cfg["njoints"], cfg["seed_poses"], cfg["latent_dim"]
    assert 0 < td < d and cd % J == 0, "the fold needs clip_dim to be a multiple of njoints"
    E = cd // J
    wt, ws = sd["embed_text.weight"], sd["seed_pose_encoder.seed_embed.weight"]
    assert wt.shape == (td, cd) and ws.shape == (d - td, J * P)
    w = torch.zeros(d, J, P + E, dtype=ws.dtype)
    w[td:, :, :P] = ws.reshape(d - td, J, P)
    w[:td, :, P:] = wt.reshape(td, J, E)
    out = {k: v for k, v in sd.items() if not k.startswith("embed_text.")}
    out["seed_pose_encoder.seed_embed.weight"] = w.reshape(d, J * (P + E))
    out["seed_pose_encoder.seed_embed.bias"] = torch.cat((sd["embed_text.bias"], sd["seed_pose_encoder.seed_embed.bias"]))
    plain = {k: v for k, v in cfg.items() if k not in ("text_dim", "clip_dim")}
    return out, dict(plain, seed_poses=P + E)


def fold_inputs(y, cfg):
    """y with the text features appended to y['seed'] as extra poses (and without 'text_embed')."""
    seed, text = y["seed"], y["text_embed"]
    B, J = seed.shape[0], cfg["njoints"]
    assert text.shape == (B, cfg["clip_dim"])
    out = {k: v for k, v in y.items() if k != "text_embed"}
    out["seed"] = torch.cat((seed, text.to(seed.dtype).reshape(B, J, 1, -1)), dim=3)
    return out


def forward(sd, cfg, x, t, y):
    """MDM(use_text=True).forward: y holds 'seed', 'mfcc', 'text_embed' [B, clip_dim] and optionally 'uncond'."""
    fsd, fcfg = fold_weights(sd, cfg)
    return omf.forward(fsd, fcfg, x, t, fold_inputs(y, cfg))


def cfg_forward(sd, cfg, x, t, y):
    """ClassifierFreeSampleModel around it (reference model/cfg_sampler.py:23-28); y also holds 'scale'."""
    fsd, fcfg = fold_weights(sd, cfg)
    return omf.cfg_forward(fsd, fcfg, x, t, fold_inputs(y, cfg))


def token0_rows(sd, cfg, t, seed, text, uncond=False):
    """Token 0 of the encoder input, emb_t + [embed_text(text) | seed_embed(flat seed)], in fp64 straight from the two Linears
    (no fold: any clip_dim) -> (rows [B, latent_dim], the condition part alone [B, latent_dim])."""
    p = {k: v.double() for k, v in sd.items()}
    B = seed.shape[0]
    flat, feats = seed.double().squeeze(2).reshape(B, -1), text.double()
    if uncond:
        flat, feats = torch.zeros_like(flat), torch.zeros_like(feats)
    lin = torch.nn.functional.linear
    cond = torch.cat((lin(feats, p["embed_text.weight"], p["embed_text.bias"]),
                      lin(flat, p["seed_pose_encoder.seed_embed.weight"], p["seed_pose_encoder.seed_embed.bias"])), dim=1)
    return omf.timestep_embed(p, t, omf.sinusoidal_pe(cfg["latent_dim"]).double()) + cond, cond


# ------------------------------------------------------------------------------------------ the fixture's cases, for both test files
CASES = {"mdm_128_t64": (64, 512), "mdm_128_t40": (40, 32)}          # text_dim, clip_dim (tools/make_golden_text.py)
WEIGHT_SEED, SCALE, RESPACING = 21, 2.5, [20]


def text_cfg(text_dim, clip_dim, J=16, d=128, layers=1, ff=192):
    return dict(arch="mdm", njoints=J, nfeats=1, latent_dim=d, ff_size=ff, num_layers=layers, num_heads=4, seed_poses=10,
                text_dim=text_dim, clip_dim=clip_dim)


def case(g, name):
    """(cfg, weights, x, t, y) of a case of forward_text_tiny.npz (`g`: the loaded archive); the weights are regenerated."""
    from gesturediffusion_amd.utils.init import init_state_dict
    cfg = text_cfg(*CASES[name])
    sd = init_state_dict(cfg, seed=WEIGHT_SEED, perturb=True)
    y = {"seed": torch.from_numpy(g[name + ".seed"]), "mfcc": torch.from_numpy(g[name + ".mfcc"]),
         "text_embed": torch.from_numpy(g[name + ".text"])}
    return cfg, sd, torch.from_numpy(g[name + ".x"]), torch.from_numpy(g[name + ".t"]), y


def build_text_model(cfg, sd, cond_mask_prob=0.1):
    """gesturediffusion_amd's MDM(use_text=True) for a text_cfg, holding the weights sd."""
    from gesturediffusion_amd.model.mdm import MDM
    m = MDM(njoints=cfg["njoints"], nfeats=1, translation=True, pose_rep="rot6d", glob=True, glob_rot=True,
            latent_dim=cfg["latent_dim"], text_dim=cfg["text_dim"], clip_dim=cfg["clip_dim"], ff_size=cfg["ff_size"],
            num_layers=cfg["num_layers"], num_heads=cfg["num_heads"], dropout=0.1, activation="gelu", data_rep="genea_vec",
            cond_mask_prob=cond_mask_prob, dataset="genea2023", use_text=True, mfcc_input=True, use_wav_enc=False,
            seed_poses=cfg["seed_poses"], use_audio=False, modeltype="", clip_version="ViT-B/32")
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith(".pe") or k.endswith("inv_freq") for k in missing), (missing, unexpected)
    return m.eval()
