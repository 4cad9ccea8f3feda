"""Gesture sampling CLI: `python -m gesturediffusion_amd.sample.generate`.

Keeps the reference CLI's flags and flow (`sample/generate.py:23-183`): args.json override,
fixseed, model + diffusion factory, checkpoint load, optional classifier-free-guidance wrapper,
then `chunks` autoregressive chunks, each a full sampling loop whose seed poses are the last
`seed_poses` frames of the previous chunk (`:104-107`).  The chunk tail of the reference (`:132-146`: inv_transform with
the dataset statistics, position / rotation split; rot2xyz is the identity for pose_rep 'xyz') runs on the device
(`gdx_postprocess`) whenever the feature count is 6 per joint (GENEA: 83 x 6 = 498); `results.npy` then holds `motion`
[B, n_joints, 3, T*chunks] and `motion_rot` like the reference's, otherwise the normalised poses [B, J, 1, T*chunks].

Two sources of conditioning.  `--dataset genea2023 [--data_dir D]` is the reference's flow (`:45-216`): take k of the
validation split is sample k, chunk c of it is item `samples_cumulative[k-1] + c` of `Genea2023`; seed poses of chunk 0,
MFCCs (computed on the GPU), text, lengths, raw audio and ground-truth motion come from the data directory, the tail uses
its statistics, and `results.npy` / `results.txt` / `results_len.txt` are written.  The BVH, MP4 and WAV files of
`:218-301` are not: bvhsdk, ffmpeg and soundfile are not dependencies of this project, and what they would hold is in
`results.npy`.  `--synthetic` needs no data: seed poses and MFCCs are N(0,1) and the tail's statistics are synthetic.
`--use_text` models are conditioned on CLIP text features, which this build does not compute: `--synthetic` draws them from the
run's seed, a data directory needs `--text_features FILE.npz` (`--list_texts OUT.txt` writes the strings to encode and exits).
`--invert_gt` (data directory and `--sampler ddim` only) starts every chunk's DDIM loop from the DDIM inversion of that chunk's
ground truth instead of a drawn x_T (`sample_chunks`, `invert_of_chunk`).
`--edit_mode in_between [--prefix_end 0.25 --suffix_start 0.75]` keeps every chunk's ground-truth frames outside the gap and
generates the gap (the reference's `sample/edit.py:76-83`); `--resample JUMP REPEATS` (`--sampler p` / `ddim`) adds RePaint's
resampling (`repaint_sample_loop`), with or without `--edit_mode`, and prints the hop and denoiser-call counts per chunk.
`--parallel_window W --parallel_tolerance TAU` (`--sampler p` / `ddim`) runs every chunk's loop parallel in time
(`parallel_sample_loop`) and prints each chunk's iteration count.

Multi-GPU: launch with `python -m torch.distributed.run --nproc-per-node N ...`; the batch is
sharded across ranks and gathered once at the end of every chunk (RCCL over xGMI).  Sharded runs draw their noise from
the counter-based generator keyed by the global sample index (`resolve_rng`), so the result does not depend on N.
"""
import os

import numpy as np
import torch

from .. import engine as E
from ..model.cfg_sampler import ClassifierFreeSampleModel
from ..model.pag_sampler import PerturbedAttentionSampleModel
from ..sampling_options import y_of_kwargs
from ..utils import dist_util
from ..utils.fixseed import fixseed
from ..data_loaders.get_data import get_dataset_loader
from ..data_loaders.tensors import gg_collate
from ..utils.init import init_state_dict, MFCC_DIM
from ..utils.model_util import create_model_and_diffusion, load_checkpoint, load_model_cached, load_model_wo_clip
from ..utils.parser_util import generate_args


def resolve_rng(rng, world):
    """Noise source of a run.  torch's generator (the reference's) gives every rank the same stream, so sharded samples
    would be correlated and depend on the world size: multi-GPU runs use the counter-based generator keyed by the
    GLOBAL sample index (shard invariant); asking for `--rng torch` there is an error, not a silent change."""
    if world > 1:
        if rng == "torch":
            raise ValueError("--rng torch with WORLD_SIZE > 1: every rank would draw the same noise for its shard; "
                             "use --rng philox (the multi-GPU default)")
        return "philox"
    return rng or "torch"


def sample_chunks(model, diffusion, first_seed, mfcc_of_chunk, n_chunks, frames, seed_poses, guidance_param=1.0,
                  sampler="p", eta=0.0, rng="torch", philox_seed=0, sample_offset=0, noise_tapes=None, progress=False,
                  on_chunk=None, plms_order=2, dpm_order=2, guidance_interval=None, guidance_rescale=0.0,
                  guidance_refresh=1, unipc_order=2, invert_of_chunk=None, report=None, text_of_chunk=None,
                  layer_cache=None, parallel=None, text_guidance_param=None, guidance_order=None, guidance_drop=None,
                  inpaint_of_chunk=None, resample=None, pag_scale=None, pag_layers=None):
    """The chunked autoregressive driver of reference `sample/generate.py:91-130`: chunk c is one complete sampling loop
    conditioned on its MFCCs and on seed poses that are `first_seed` for c = 0 and afterwards the LAST `seed_poses` frames
    of chunk c-1 -- a view of the previous output that stays on the device (`:104-107`).  Yields nothing; returns the list
    of chunk outputs [b, J, 1, frames].  noise_tapes: optional list of recorded noise tapes, one per chunk (tests); the PLMS,
    DPM-Solver++ ("dpmpp") and UniPC ("unipc": order `unipc_order`) samplers draw nothing after x_T and take entry 0 of a tape
    as that, the stochastic DPM-Solver++ ("dpmpp_sde": order `dpm_order`, 1 or 2, noise scale `eta`) draws per step like "p" and
    is handed the whole tape.
    guidance_interval (lo, hi): guidance only on model timesteps lo <= t <= hi (y['guidance_interval']; needs
    guidance_param != 1).  guidance_rescale phi > 0: the guidance rescale (y['guidance_rescale']; needs guidance_param != 1).
    guidance_refresh k > 1: the unconditional pass on every k-th guided denoiser call, the stored cond-uncond difference in
    between (y['guidance_refresh']; needs guidance_param != 1); each chunk is its own loop and starts with a refresh.
    invert_of_chunk(c) -> recorded motion [b, J, 1, frames] in the sampler's normalised units ("ddim" only): chunk c's x_T is not
    drawn but is that motion's DDIM inversion (ddim_reverse_sample_loop) under the chunk's own seed poses and MFCCs, with the
    conditional pass alone -- no guidance, whatever guidance_param says; the (guided) DDIM loop then starts from it.  With
    guidance_param == 1 the loop retraces the inversion, and report(text) is told each chunk's round-trip error.
    text_of_chunk(c) -> text features [b, clip_dim] on the device (a use_text model): chunk c's y['text_embed'].
    layer_cache (every, keep): every every-th denoiser call in full, the first keep encoder layers plus the stored change of the
    deeper ones in between (y['layer_cache']); each chunk is its own loop and starts with a full call.
    parallel (window, tolerance): every chunk's loop runs parallel in time (parallel_sample_loop; samplers "p" and "ddim", Philox
    noise or a tape; neither guidance_refresh > 1, layer_cache nor invert_of_chunk) and report(text) is told each chunk's iterations.
    Per-condition guidance of a use_text model (needs guidance_param != 1; the loops validate the rest): guidance_drop "both" |
    "text" | "seed" names what the contrast pass drops (y['guidance_drop']); text_guidance_param S runs three passes with the text
    stage at S and the seed stage at guidance_param (y['text_scale']), guidance_order saying which comes first (y['guidance_order']).
    inpaint_of_chunk(c) -> (mask bool, motion) [b, J, 1, frames] on the device: chunk c's y['inpainting_mask'] / y['inpainted_motion'];
    the seed hand-off is unchanged.  resample (jump, repeats): every chunk's loop resamples (repaint_sample_loop; samplers "p" and
    "ddim"; neither guidance_refresh > 1, layer_cache, parallel nor invert_of_chunk); a recorded tape then holds one entry per hop.
    pag_scale W: perturbed-attention guidance (y['pag_scale'], with pag_layers as y['pag_layers']; the loops validate both): with
    guidance_param == 1 the model is a PerturbedAttentionSampleModel and this is the run's guidance -- interval, rescale and
    refresh then apply to it --, otherwise it is the third pass of a ClassifierFreeSampleModel."""
    guided = guidance_param != 1 or pag_scale is not None
    if pag_layers is not None and pag_scale is None:
        raise ValueError("pag_layers needs pag_scale")
    if resample is not None:
        if sampler not in ("p", "ddim"):
            raise ValueError("resample needs sampler='p' or 'ddim': a multistep sampler's history does not survive a jump")
        if guidance_refresh != 1 or layer_cache is not None or parallel is not None or invert_of_chunk is not None:
            raise ValueError("resample runs neither guidance_refresh > 1, layer_cache, parallel nor invert_of_chunk")
    if guidance_param == 1 and (text_guidance_param is not None or guidance_order is not None or guidance_drop is not None):
        raise ValueError("text_guidance_param / guidance_order / guidance_drop need guidance_param != 1: without guidance there is "
                         "nothing to compose")
    if parallel is not None:
        if sampler not in ("p", "ddim"):
            raise ValueError("parallel needs sampler='p' or 'ddim'")
        if guidance_refresh != 1 or layer_cache is not None or invert_of_chunk is not None:
            raise ValueError("parallel runs neither guidance_refresh > 1, layer_cache nor invert_of_chunk: its window evaluates steps "
                             "side by side")
        if rng != "philox" and noise_tapes is None:
            raise ValueError("parallel draws its noise from the counter-based generator: rng must be 'philox' (or pass noise_tapes)")
    if invert_of_chunk is not None and layer_cache is not None:
        raise ValueError("invert_of_chunk runs no layer cache")
    if invert_of_chunk is not None and sampler != "ddim":
        raise ValueError("invert_of_chunk needs sampler='ddim': the latent is the start state of the deterministic DDIM loop")
    if invert_of_chunk is not None and guidance_refresh > 1:
        raise ValueError("invert_of_chunk runs no guidance refresh")
    if guidance_interval is not None and not guided:
        raise ValueError("guidance_interval needs guidance_param != 1: without guidance there is nothing to limit")
    if guidance_rescale > 0 and not guided:
        raise ValueError("guidance_rescale needs guidance_param != 1: without guidance there is nothing to rescale")
    if isinstance(guidance_refresh, bool) or not isinstance(guidance_refresh, int) or guidance_refresh < 1:
        raise ValueError(f"guidance_refresh must be an int >= 1, got {guidance_refresh!r}")
    if guidance_refresh > 1 and not guided:
        raise ValueError("guidance_refresh needs guidance_param != 1: without guidance there is nothing to refresh")
    b, J = first_seed.shape[0], first_seed.shape[1]
    sample_fn = {"p": diffusion.p_sample_loop, "ddim": diffusion.ddim_sample_loop, "plms": diffusion.plms_sample_loop,
                 "dpmpp": diffusion.dpm_solver_sample_loop, "dpmpp_sde": diffusion.dpm_solver_sde_sample_loop,
                 "unipc": diffusion.unipc_sample_loop}[sampler]
    options = dict(guidance_interval=guidance_interval, guidance_rescale=guidance_rescale, guidance_refresh=guidance_refresh,
                   text_guidance_param=text_guidance_param, guidance_order=guidance_order, guidance_drop=guidance_drop,
                   layer_cache=layer_cache)
    outs, sample_out = [], None
    for chunk in range(n_chunks):
        y = {"mfcc": mfcc_of_chunk(chunk), "seed": first_seed if chunk == 0 else sample_out[..., -seed_poses:]}
        if text_of_chunk is not None:
            y["text_embed"] = text_of_chunk(chunk)
        if guidance_param != 1:
            y["scale"] = torch.ones(b, device=first_seed.device) * guidance_param
        y.update(y_of_kwargs(options, b, first_seed.device))
        if pag_scale is not None:
            y["pag_scale"] = torch.ones(b, device=first_seed.device) * pag_scale
            if pag_layers is not None:
                y["pag_layers"] = tuple(int(l) for l in pag_layers)
        if inpaint_of_chunk is not None:
            y["inpainting_mask"], y["inpainted_motion"] = inpaint_of_chunk(chunk)
        kw = dict(clip_denoised=False, model_kwargs={"y": y}, skip_timesteps=0, init_image=None, progress=progress,
                  noise=None, rng=rng, philox_seed=philox_seed + 1000 * chunk, sample_offset=sample_offset,
                  noise_tape=noise_tapes[chunk] if noise_tapes is not None else None)
        if sampler == "p":
            kw.update(dump_steps=None, const_noise=False)
        elif sampler == "ddim":
            kw.update(eta=eta)
        elif sampler == "dpmpp_sde":
            kw.update(order=dpm_order, eta=eta)
        else:
            tape = kw.pop("noise_tape")
            kw.update(order={"dpmpp": dpm_order, "unipc": unipc_order, "plms": plms_order}[sampler],
                      noise=tape[0] if tape is not None else None)
        if on_chunk is not None:
            on_chunk(chunk)
        gt = None
        if invert_of_chunk is not None:
            gt = invert_of_chunk(chunk)
            inner = model.model if isinstance(model, ClassifierFreeSampleModel) else model
            kw["noise"] = diffusion.ddim_reverse_sample_loop(inner, gt, clip_denoised=False, progress=progress,
                                                             model_kwargs={"y": {k: y[k] for k in ("mfcc", "seed", "text_embed")
                                                                                 if k in y}})
        if parallel is not None:
            stats = {}
            sample_out = diffusion.parallel_sample_loop(
                model, (b, J, 1, frames), clip_denoised=False, model_kwargs={"y": y}, progress=progress, sampler=sampler, eta=eta,
                window=parallel[0], tolerance=parallel[1], philox_seed=kw["philox_seed"], sample_offset=sample_offset,
                noise_tape=kw["noise_tape"], report=stats)
            if report is not None:
                report(f"### chunk {chunk + 1}: parallel: {stats['iterations']} iterations for {sum(stats['strides'])} steps")
            outs.append(sample_out)
            continue
        if resample is not None:
            sample_out = diffusion.repaint_sample_loop(
                model, (b, J, 1, frames), clip_denoised=False, model_kwargs={"y": y}, progress=progress, sampler=sampler, eta=eta,
                jump=resample[0], repeats=resample[1], rng=rng, philox_seed=kw["philox_seed"], sample_offset=sample_offset,
                noise_tape=kw["noise_tape"])
            outs.append(sample_out)
            continue
        sample_out = sample_fn(model, (b, J, 1, frames), **kw)
        if gt is not None and guidance_param == 1 and report is not None:
            err = float((sample_out - gt).abs().max() / gt.abs().max())
            report(f"### chunk {chunk + 1}: round trip max|regenerated - gt| / max|gt| = {err:.3e}")
        outs.append(sample_out)
    return outs


def chunk_items(samples_cumulative, num_samples, n_chunks):
    """Dataset index of every (take, chunk) pair, [n_chunks][num_samples]: chunk c of take k is item
    `samples_cumulative[k-1] + c` (reference `:94-99`).  All pairs are checked here, in the reference's order and with its
    error, before anything is sampled."""
    if num_samples > len(samples_cumulative):
        raise ValueError(f"{num_samples} takes asked for, the split holds {len(samples_cumulative)}")
    index = []
    for chunk in range(n_chunks):
        row = []
        for take in range(num_samples):
            item = (0 if take == 0 else int(samples_cumulative[take - 1])) + chunk
            if item >= samples_cumulative[take]:
                raise ValueError(f'Chunk {chunk} is out of range for take {take}.')
            row.append(item)
        index.append(row)
    return index


def check_data_width(data_width, njoints):
    """The model is built for `njoints` pose features; a data directory of another width cannot condition or de-normalise it."""
    if data_width != njoints:
        raise ValueError(f"the data directory's poses have {data_width} features, the model is built for {njoints}")


def run_texts(ds, index):
    """The text of every (take, chunk) window of a run, [n_chunks][num_samples] (`index` from chunk_items); host only."""
    return [[ds.text_window(*ds.locate(i)) for i in row] for row in index]


def distinct(texts):
    """The distinct strings of run_texts' table in order of first appearance (what --list_texts writes, one per line)."""
    return list(dict.fromkeys(t for row in texts for t in row))


def lookup_text_features(path, texts, clip_dim):
    """--text_features: the npz's `features` rows for run_texts' table -> float32 [n_chunks, num_samples, clip_dim] (host), each
    string looked up by exact match in the npz's `text` array ('' is a key like any other).  ValueError, before anything is
    sampled, for a file without the two arrays, features that are not [len(text), clip_dim], and strings the file lacks: their
    number and the first few."""
    with np.load(path, allow_pickle=False) as f:
        if "text" not in f.files or "features" not in f.files:
            raise ValueError(f"{path} must hold the arrays `text` and `features`, it holds {sorted(f.files)}")
        keys, feats = [str(t) for t in f["text"].reshape(-1)], np.asarray(f["features"], dtype=np.float32)
    if feats.shape != (len(keys), clip_dim):
        raise ValueError(f"{path}: `features` must be [{len(keys)}, {clip_dim}] (one row of clip_dim per text), it is {list(feats.shape)}")
    row = {k: i for i, k in reversed(list(enumerate(keys)))}                 # a repeated string: its first row
    missing = [t for t in distinct(texts) if t not in row]
    if missing:
        raise ValueError(f"{len(missing)} of the run's {len(distinct(texts))} texts are not in {path}; the first: "
                         f"{missing[:3]!r} (--list_texts OUT.txt writes all of them)")
    return torch.from_numpy(np.stack([feats[[row[t] for t in chunk]] for chunk in texts]))


def synthetic_text_features(seed, num_samples, clip_dim, n_chunks):
    """--use_text --synthetic: N(0,1) stand-ins for the CLIP features, one [num_samples, clip_dim] per chunk, from a generator of
    their own keyed by the run's seed (the seed-pose and MFCC draws of a run do not depend on --use_text)."""
    g = torch.Generator().manual_seed(int(seed) * 1000003 + 512)
    return [torch.randn(num_samples, clip_dim, generator=g) for _ in range(n_chunks)]


def edit_mask(edit_mode, prefix_end, suffix_start, shape, device):
    """--edit_mode: the y['inpainting_mask'] of a chunk of `shape` [b, J, 1, T], True where the ground truth is kept (reference
    sample/edit.py:76-83 at full length): in_between keeps the frames outside [int(prefix_end * T), int(suffix_start * T))."""
    if edit_mode == "upper_body":
        raise NotImplementedError("--edit_mode upper_body: the reference's mask is HumanML's joint table (HML_LOWER_BODY_MASK), "
                                  "which says nothing about a GENEA skeleton")
    if edit_mode != "in_between":
        raise ValueError(f"edit_mode must be 'in_between' or 'upper_body', got {edit_mode!r}")
    T = shape[-1]
    mask = torch.ones(shape, dtype=torch.bool, device=device)
    mask[..., int(prefix_end * T):int(suffix_start * T)] = False
    return mask


def synthetic_ground_truth(seed, num_samples, njoints, frames, n_chunks):
    """--edit_mode --synthetic: N(0,1) stand-ins for the recorded chunks, one [num_samples, njoints, 1, frames] per chunk, from a
    generator of their own keyed by the run's seed (the seed-pose and MFCC draws of a run do not depend on --edit_mode)."""
    g = torch.Generator().manual_seed(int(seed) * 1000003 + 1024)
    return [torch.randn(num_samples, njoints, 1, frames, generator=g) for _ in range(n_chunks)]


def host_item(ds, idx):
    """Item `idx` of a Genea2023 without its MFCCs (zeros stand in): everything `gg_collate` needs that is host data."""
    take, sample = ds.locate(idx)
    motion, seed = ds.motion_window(take, sample)
    return (motion, ds.text_window(take, sample), ds.window, ds.audio_window(take, sample),
            np.zeros((ds.window, MFCC_DIM), dtype=np.float32), seed)


def main(argv=None):
    args = generate_args(argv)
    if args.list_texts:                # host only: the strings a user encodes with their own CLIP for --text_features
        n = min(args.num_samples if args.num_samples else 41, args.batch_size)
        ds = get_dataset_loader(args.dataset, n, args.num_frames, split='val', hml_mode='text_only', seed_poses=args.seed_poses,
                                datapath=args.data_dir or None).dataset
        lines = distinct(run_texts(ds, chunk_items(ds.samples_cumulative, n, args.chunks)))
        with open(args.list_texts, "w") as f:
            f.write("".join(t + "\n" for t in lines))
        print(f"wrote {len(lines)} distinct texts to [{args.list_texts}]")
        return 0
    fixseed(args.seed)
    rank, world, device = dist_util.init_from_env(arg_device=args.device)   # makes `device` current: nothing exists yet
    if device.type != "cuda":
        raise RuntimeError("sample.generate needs an MI355X GPU: the native path has no CPU fallback")
    rng = resolve_rng(args.rng, world)
    num_samples = min(args.num_samples if args.num_samples else 41, args.batch_size)
    dist_util.check_world(num_samples, world)       # the same refusal on every rank, before any of them builds a model
    if args.dataset not in ("genea2022", "genea2023") and not args.synthetic_njoints:
        args.synthetic_njoints = 263
    if args.synthetic or not args.model_path:       # random weights: the conditioning this CLI can feed is MFCCs
        args.mfcc_input = True
    T = args.num_frames
    ds = index = None
    if not args.synthetic:
        ds = get_dataset_loader(args.dataset, num_samples, T, split='val', hml_mode='text_only', seed_poses=args.seed_poses,
                                datapath=args.data_dir or None, device=device).dataset
        index = chunk_items(ds.samples_cumulative, num_samples, args.chunks)

    model, diffusion = create_model_and_diffusion(args, None)
    if ds is not None:
        check_data_width(ds.mean.shape[-1], model.njoints)
    text_dim, clip_dim = model._text_dims()
    text_feats = None                                   # per chunk [num_samples, clip_dim] on the host, every rank the whole table
    if text_dim and ds is not None:
        text_feats = lookup_text_features(args.text_features, run_texts(ds, index), clip_dim)
    elif text_dim:
        text_feats = synthetic_text_features(args.seed, num_samples, clip_dim, args.chunks)
    if args.model_path and args.packed_cache:
        model.to(device)
        how = load_model_cached(model, args.model_path, device, args.packed_cache)
        if rank == 0:
            print(f"### weights from the packed {how}" if how == "image" else "### weights from the checkpoint (packed image written)")
    elif args.model_path:
        state_dict = load_checkpoint(args.model_path)
        load_model_wo_clip(model, state_dict)
    else:
        cfg = dict(arch=args.arch_version, njoints=model.njoints, nfeats=1, latent_dim=args.latent_dim, ff_size=1024,
                   num_layers=args.layers, num_heads=4, seed_poses=args.seed_poses, text_dim=text_dim, clip_dim=clip_dim)
        model.load_state_dict(init_state_dict(cfg, seed=args.seed), strict=False)
    if args.guidance_param != 1:
        model = ClassifierFreeSampleModel(model)
    elif args.pag_scale is not None:
        model = PerturbedAttentionSampleModel(model)
    model.to(device)
    model.eval()

    lo, hi = dist_util.shard_range(num_samples, rank, world)
    J = model.njoints
    if ds is not None:
        shard = {}

        def shard_y(chunk):            # this rank's takes of one chunk, collated; their MFCCs are computed here, on the device
            if chunk not in shard:
                shard.clear()
                shard[chunk] = gg_collate([ds[i] for i in index[chunk][lo:hi]])[1]["y"]
            return shard[chunk]

        split6, mean, std = True, ds.mean, ds.std
        first_seed = shard_y(0)["seed"].to(device)

        def mfcc_of_chunk(chunk):
            return shard_y(chunk)["mfcc"]
    else:
        g = torch.Generator().manual_seed(args.seed)
        first_seed = torch.randn(num_samples, J, 1, args.seed_poses, generator=g)[lo:hi].to(device)
        split6 = J % 6 == 0                                   # GENEA layout: 3 rotation + 3 position features per joint
        if split6:
            stat_rng = np.random.default_rng(args.seed)       # stand-in for the dataset's Mean.npy / Std.npy (fp64)
            mean, std = stat_rng.normal(size=J), stat_rng.uniform(0.5, 2.0, size=J)
        extractor = None
        if args.synthetic_audio:
            # the reference's audio path (dataset.py:81-95) at its GENEA settings: 22 050 Hz, 30 fps, one MFCC vector per frame
            from ..data_loaders.mfcc import MfccExtractor
            stat = np.random.default_rng(args.seed + 1)
            extractor = MfccExtractor(device, sr=22050, fps=30, mfcc_mean=stat.normal(size=MFCC_DIM),
                                      mfcc_std=stat.uniform(0.5, 2.0, size=MFCC_DIM))

        def mfcc_of_chunk(chunk):          # called once per chunk, in order: the host generator's stream is part of the recipe
            if extractor is not None:
                audio = 0.1 * torch.randn(num_samples, T * 735, generator=g)[lo:hi].to(device)
                return torch.stack([extractor(a)[:T].t() for a in audio]).unsqueeze(2).contiguous()     # [nb, 26, 1, T]
            return torch.randn(num_samples, MFCC_DIM, 1, T, generator=g)[lo:hi].to(device)

    text_of_chunk = None
    if text_feats is not None:
        def text_of_chunk(chunk):          # this rank's shard of the chunk's features
            return text_feats[chunk][lo:hi].to(device)

    def on_chunk(chunk):
        if rank == 0:
            print(f"### Sampling chunk {chunk + 1} of {args.chunks}")

    invert_of_chunk = None
    if args.invert_gt:
        def invert_of_chunk(chunk):        # this rank's ground-truth chunks, normalised, as the sampler's [b, J, 1, T]
            return gg_collate([host_item(ds, i) for i in index[chunk][lo:hi]])[0].float().to(device)

    inpaint_of_chunk = None
    if args.edit_mode is not None:
        mask = edit_mask(args.edit_mode, args.prefix_end, args.suffix_start, (hi - lo, J, 1, T), device)
        synthetic_gt = synthetic_ground_truth(args.seed, num_samples, J, T, args.chunks) if ds is None else None

        def inpaint_of_chunk(chunk):       # this rank's ground-truth chunks, normalised, and the frames that are kept of them
            if ds is None:
                return mask, synthetic_gt[chunk][lo:hi].to(device)
            return mask, gg_collate([host_item(ds, i) for i in index[chunk][lo:hi]])[0].float().to(device)
        if rank == 0:
            print(f"### in-betweening: frames {int(args.prefix_end * T)}..{int(args.suffix_start * T) - 1} of {T} are generated, the "
                  f"rest is kept")
    if args.resample is not None and rank == 0:
        plan = diffusion.resample_plan(*args.resample)
        print(f"### resampling (jump {args.resample[0]}, repeats {args.resample[1]}): {len(plan)} hops, "
              f"{sum(h[0] == 'r' for h in plan)} denoiser calls per chunk")

    def report(text):
        print(text if world == 1 else f"{text} (rank {rank})")

    interval = tuple(args.guidance_interval) if args.guidance_interval is not None else None
    if interval is not None and rank == 0:
        flags = diffusion.guided_steps(interval)
        print(f"### guidance on {sum(flags)} of {len(flags)} steps (model timesteps {interval[0]}..{interval[1]})")
    if args.guidance_rescale > 0 and rank == 0:
        print(f"### guidance rescale {args.guidance_rescale:.2f}")
    if args.text_guidance_param is not None and rank == 0:
        print(f"### per-condition guidance ({args.guidance_order or 'seed_text'}): seed scale {args.guidance_param:g}, text scale "
              f"{args.text_guidance_param:g}, three passes per guided step")
    if args.pag_scale is not None and rank == 0:
        print(f"### perturbed-attention guidance: scale {args.pag_scale:g} on layers {list(args.pag_layers)}")
    if args.guidance_drop is not None and rank == 0:
        print(f"### guidance contrast pass drops: {args.guidance_drop}")
    if args.guidance_refresh > 1 and rank == 0:
        plan = diffusion.guidance_plan(interval, args.guidance_refresh, plms=args.sampler == "plms")
        print(f"### unconditional pass on {plan.count('refresh')} of {len(plan) - plan.count('off')} guided calls")
    if args.layer_cache is not None and rank == 0:
        plan = diffusion.layer_cache_plan(args.layer_cache, interval, args.guidance_refresh, guided=args.guidance_param != 1 or args.pag_scale is not None,
                                          plms=args.sampler == "plms")
        print(f"### layer cache: {plan.count('full')} full, {plan.count('partial')} partial calls; "
              f"{args.layer_cache[1]} of {args.layers} layers on a partial call")
    outs = sample_chunks(model, diffusion, first_seed, mfcc_of_chunk, args.chunks, T, args.seed_poses,
                         guidance_param=args.guidance_param, sampler=args.sampler,
                         eta=args.dpm_eta if args.sampler == "dpmpp_sde" else args.eta, rng=rng,
                         philox_seed=args.seed, sample_offset=lo, progress=args.progress and rank == 0, on_chunk=on_chunk,
                         plms_order=args.plms_order, dpm_order=args.dpm_order, unipc_order=args.unipc_order,
                         guidance_interval=interval, guidance_rescale=args.guidance_rescale,
                         guidance_refresh=args.guidance_refresh, invert_of_chunk=invert_of_chunk, report=report,
                         text_of_chunk=text_of_chunk, layer_cache=args.layer_cache, text_guidance_param=args.text_guidance_param,
                         guidance_order=args.guidance_order, guidance_drop=args.guidance_drop,
                         parallel=(args.parallel_window, args.parallel_tolerance) if args.parallel_window else None,
                         inpaint_of_chunk=inpaint_of_chunk, resample=args.resample, pag_scale=args.pag_scale,
                         pag_layers=args.pag_layers)
    out_chunks, rot_chunks = [], []
    for sample_out in outs:
        full = dist_util.gather_samples(sample_out, num_samples)
        if rank == 0:
            if split6:
                pos, rot = E.postprocess(full, mean, std)   # inv_transform + index split on the device
                out_chunks.append(pos.cpu().numpy())
                rot_chunks.append(rot.cpu().numpy())
            else:
                out_chunks.append(full.cpu().numpy())
    if rank == 0:
        out_path = args.output_dir or os.path.join(os.getcwd(), f"samples_{'synthetic' if args.synthetic else args.dataset}_seed{args.seed}")
        os.makedirs(out_path, exist_ok=True)
        motion = np.concatenate(out_chunks, axis=3)
        res = {"motion": motion, "num_samples": num_samples, "num_chunks": args.chunks}
        if split6:
            res["motion_rot"] = np.concatenate(rot_chunks, axis=3)
        if ds is not None:
            res.update(ground_truth(ds, index, device))
        npy_path = os.path.join(out_path, "results.npy")
        np.save(npy_path, res, allow_pickle=True)
        if ds is not None:
            with open(npy_path.replace('.npy', '.txt'), 'w') as f:
                f.write('\n'.join(res["text"]))
            with open(npy_path.replace('.npy', '_len.txt'), 'w') as f:
                f.write('\n'.join(str(n) for n in res["lengths"]))
            print("BVH, MP4 and WAV files are not written (they need bvhsdk, ffmpeg and soundfile): "
                  "results.npy holds the motion, the ground truth and the audio they would contain")
        print(f"saved results to [{npy_path}] motion {motion.shape}")
    return 0


def ground_truth(ds, index, device):
    """What the data directory itself says about the sampled takes (reference `:149-193`), read on the host by the rank
    that writes the results: per chunk the collated ground-truth motion through the same tail as the samples, the text, the
    lengths and the raw audio; chunks are joined along time, text and lengths listed chunk by chunk."""
    pos_chunks, rot_chunks, audio, text, lengths = [], [], [], [], []
    for row in index:
        gt_motion, cond = gg_collate([host_item(ds, i) for i in row])
        pos, rot = E.postprocess(gt_motion.to(device), ds.mean, ds.std)
        pos_chunks.append(pos.cpu().numpy())
        rot_chunks.append(rot.cpu().numpy())
        audio.append(cond["y"]["audio"].numpy())
        text += cond["y"]["text"]
        lengths.append(cond["y"]["lengths"].numpy())
    return {"gt_motion": np.concatenate(pos_chunks, axis=3), "gt_motion_rot": np.concatenate(rot_chunks, axis=3),
            "audio": np.concatenate(audio, axis=1), "text": text, "lengths": np.concatenate(lengths, axis=0),
            "takes": [ds.takes[k][0] for k in range(len(index[0]))]}


if __name__ == "__main__":
    raise SystemExit(main())
