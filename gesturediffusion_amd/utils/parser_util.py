"""Command-line options: drop-in for the sampling subset of reference `utils/parser_util.py`.

Same flag names, defaults and groups (`:53-58` base, `:61-67` diffusion, `:70-95` model,
`:99-106` dataset, `:141-154` sampling, `:157-171` generate) and the same rule that the
dataset / model / diffusion groups are overwritten from `args.json` next to the checkpoint
(`:7-33`).  The reference's quirks are kept on purpose: `type=bool` flags are truthy for any
non-empty string (`:55,67`), `--dataset`'s default is outside its own choices (`:101`).
Additive flags live in the 'native' group and never collide with reference names.
"""
import json
import os
from argparse import ArgumentParser


CHECKPOINT_GROUPS = ("dataset", "model", "diffusion")     # option groups a checkpoint's args.json decides (:13)


def parse_and_load_from_model(parser, argv=None):
    """Parse the command line, then let the `args.json` stored next to the checkpoint decide every option of the
    dataset / model / diffusion groups (reference `utils/parser_util.py:7-33`): a model is sampled with the settings it
    was trained with, whatever the command line says.  Options the file does not know keep their value, with the
    reference's warning.  A model trained without condition dropout cannot be guided, so its guidance scale becomes 1."""
    for add in (add_data_options, add_model_options, add_diffusion_options, add_native_options):
        add(parser)
    args = parser.parse_args(argv)
    if args.sampler == "dpmpp_sde" and args.dpm_order == 3:
        parser.error("--sampler dpmpp_sde has orders 1 and 2 only (a third-order stochastic step is unstable below about 20 "
                     "steps and no more accurate above): use --dpm_order 1 or 2, or --sampler dpmpp for order 3")
    if args.dpm_eta < 0:
        parser.error("--dpm_eta must be >= 0")
    asked_data_dir = args.data_dir
    # additive: without a checkpoint there is no args.json -- --synthetic, or a data directory sampled with random weights
    if not (not args.model_path and (args.synthetic or args.data_dir)):
        stored_path = os.path.join(os.path.dirname(args.model_path), "args.json")
        assert os.path.exists(stored_path), "Arguments json file was not found!"
        with open(stored_path) as f:
            stored = json.load(f)
        for name in (n for title in CHECKPOINT_GROUPS for n in get_args_per_group_name(parser, args, title)):
            if name in stored:
                setattr(args, name, stored[name])
            else:
                print("Warning: was not able to load [{}], using default value [{}] instead.".format(name, getattr(args, name)))
    if asked_data_dir:       # additive: where the data lies is this machine's business, not the training run's
        args.data_dir = asked_data_dir
    if args.cond_mask_prob == 0:
        args.guidance_param = 1
    if args.pag_layers is not None and args.pag_scale is None:
        parser.error("--pag_layers needs --pag_scale: the layers say where the pass is perturbed, the scale turns it on")
    if args.pag_scale is not None:
        layers = args.pag_layers if args.pag_layers is not None else [args.layers // 2]
        if len(set(layers)) != len(layers) or not all(0 <= l < args.layers for l in layers):
            parser.error(f"--pag_layers must name distinct encoder layers in 0 .. layers - 1 = {args.layers - 1}")
        args.pag_layers = tuple(layers)
        if args.text_guidance_param is not None:
            parser.error("--pag_scale and --text_guidance_param exclude each other: each adds a third pass, and four are not supported")
        if args.guidance_drop in ("text", "seed"):
            parser.error("--pag_scale and --guidance_drop text|seed exclude each other: the perturbed pass takes the place of the "
                         "pass with one condition dropped")
        if args.invert_gt:
            parser.error("--pag_scale does not combine with --invert_gt: the inversion is one conditional pass per step")
        if args.guidance_param != 1:                             # three passes: the conflicts of --text_guidance_param
            if args.guidance_refresh is not None and args.guidance_refresh > 1:
                parser.error("--pag_scale with --guidance_param != 1 runs no guidance refresh: the refresh stores one cond-uncond "
                             "difference (use --guidance_param 1)")
            if args.layer_cache is not None and args.layer_cache[0] > 1:
                parser.error("--pag_scale with --guidance_param != 1 runs no layer cache: the cache holds two row groups, this "
                             "guidance runs three (use --guidance_param 1)")
            if args.parallel_window:
                parser.error("--pag_scale with --guidance_param != 1 does not combine with --parallel_window, whose window repeats "
                             "one scale per slot (use --guidance_param 1)")
    # perturbed-attention guidance guides without the unconditional pass: the options of a guided loop apply to it
    unguided = args.guidance_param == 1 and args.pag_scale is None
    if args.guidance_interval is not None and unguided:
        parser.error("--guidance_interval needs guidance: --guidance_param is 1 (no classifier-free guidance runs at all)")
    if not 0 <= args.guidance_rescale <= 1:
        parser.error("--guidance_rescale must lie in [0, 1]")
    if args.guidance_rescale > 0 and unguided:
        parser.error("--guidance_rescale needs guidance: --guidance_param is 1 (no classifier-free guidance runs at all)")
    if args.guidance_refresh is not None and args.guidance_refresh < 1:
        parser.error("--guidance_refresh must be at least 1")
    if args.guidance_refresh is not None and unguided:
        parser.error("--guidance_refresh needs guidance: --guidance_param is 1 (no classifier-free guidance runs at all)")
    if args.guidance_refresh is None:
        args.guidance_refresh = 1
    composes = [f for f, on in (("--text_guidance_param", args.text_guidance_param is not None),
                                ("--guidance_order", args.guidance_order is not None),
                                ("--guidance_drop", args.guidance_drop is not None)) if on]
    if composes:
        if not args.use_text:
            parser.error(f"{composes[0]} needs --use_text: without text the seed poses are the one condition that can be dropped")
        if args.guidance_param == 1:
            parser.error(f"{composes[0]} needs guidance: --guidance_param is 1 (no classifier-free guidance runs at all)")
        if args.text_guidance_param is not None and args.guidance_drop is not None:
            parser.error("--text_guidance_param and --guidance_drop exclude each other: the first runs both contrast passes, "
                         "the second chooses the one that runs")
        if args.guidance_order is not None and args.text_guidance_param is None:
            parser.error("--guidance_order needs --text_guidance_param: with one scale there is one stage and no order")
    if args.text_guidance_param is not None:
        if args.guidance_refresh > 1:
            parser.error("--text_guidance_param runs no guidance refresh: the refresh stores one cond-uncond difference")
        if args.layer_cache is not None and args.layer_cache[0] > 1:
            parser.error("--text_guidance_param runs no layer cache: the cache holds two row groups, this guidance runs three")
        if args.parallel_window:
            parser.error("--text_guidance_param does not combine with --parallel_window, whose window repeats one scale per slot")
    if args.layer_cache is not None:
        every, keep = args.layer_cache
        if every < 1:
            parser.error("--layer_cache EVERY must be at least 1")
        if every > 1 and not 1 <= keep <= args.layers - 1:
            parser.error(f"--layer_cache KEEP must lie in 1 .. layers - 1 = {args.layers - 1}")
        args.layer_cache = (every, keep) if every > 1 else None         # EVERY = 1 is off: KEEP is not looked at
    if args.invert_gt:
        if args.layer_cache is not None:
            parser.error("--invert_gt runs no layer cache: the inversion makes every denoiser call in full")
        if args.synthetic or args.dataset != "genea2023" or not args.data_dir:
            parser.error("--invert_gt inverts recorded motion: it needs --dataset genea2023 --data_dir D (and no --synthetic)")
        if args.sampler != "ddim":
            parser.error("--invert_gt needs --sampler ddim: the latent is the start state of the deterministic DDIM loop")
        if args.guidance_refresh > 1:
            parser.error("--invert_gt runs no guidance refresh: the inversion is one conditional pass per step")
    if args.parallel_window < 0 or args.parallel_window > 64:
        parser.error("--parallel_window must lie in 0 .. 64 (0 = off)")
    if not args.parallel_tolerance >= 0:
        parser.error("--parallel_tolerance must be >= 0")
    if args.parallel_window:
        if args.sampler not in ("p", "ddim"):
            parser.error("--parallel_window runs --sampler p or ddim only: the window re-runs their one-step update chain")
        if args.guidance_refresh > 1:
            parser.error("--parallel_window runs no guidance refresh: the stored difference needs sequential denoiser calls")
        if args.layer_cache is not None:
            parser.error("--parallel_window runs no layer cache: the stored change needs sequential denoiser calls")
        if args.invert_gt:
            parser.error("--parallel_window does not combine with --invert_gt")
        if args.rng == "torch":
            parser.error("--parallel_window draws its noise from the counter-based generator: use --rng philox (its default)")
        args.rng = "philox"
    if not 0 <= args.prefix_end <= args.suffix_start <= 1:
        parser.error("--prefix_end and --suffix_start must satisfy 0 <= prefix_end <= suffix_start <= 1")
    if args.resample is not None:
        jump, repeats = args.resample
        if jump < 1 or repeats < 1:
            parser.error("--resample JUMP REPEATS must both be at least 1")
        if args.sampler not in ("p", "ddim"):
            parser.error("--resample runs --sampler p or ddim only: a multistep sampler's history does not survive a jump")
        if args.guidance_refresh > 1:
            parser.error("--resample runs no guidance refresh: a forward hop invalidates the stored difference")
        if args.layer_cache is not None:
            parser.error("--resample runs no layer cache: a forward hop invalidates the stored change")
        if args.parallel_window:
            parser.error("--resample does not combine with --parallel_window")
        if args.invert_gt:
            parser.error("--resample does not combine with --invert_gt: the resampled chain is stochastic")
        args.resample = (jump, repeats)
    if args.list_texts and args.synthetic:
        parser.error("--list_texts lists the texts of a data directory: --synthetic has none")
    if args.use_text and args.arch_version == "mdm" and not (args.synthetic or args.text_features or args.list_texts):
        parser.error("--use_text on a data directory needs --text_features FILE.npz (arrays `text`: the strings, `features`: "
                     "float32 [N, clip_dim], their CLIP text features); --list_texts OUT.txt writes the strings this run needs")
    return args


def get_args_per_group_name(parser, args, group_name):
    """Destination names of the options declared in the argparse group titled `group_name`.  (The reference *returns* a
    ValueError instance for an unknown title instead of raising it, `:36-41`; iterating that fails with TypeError -- kept.)"""
    for group in parser._action_groups:
        if group.title == group_name:
            return [action.dest for action in group._group_actions]
    return ValueError("group_name was not found.")


def add_base_options(parser):
    group = parser.add_argument_group('base')
    group.add_argument("--cuda", default=True, type=bool, help="Use cuda device, otherwise use CPU.")
    group.add_argument("--device", default=0, type=int, help="Device id to use.")
    group.add_argument("--seed", default=10, type=int, help="For fixing random seed.")
    group.add_argument("--batch_size", default=256, type=int, help="Batch size during training.")


def add_diffusion_options(parser):
    group = parser.add_argument_group('diffusion')
    group.add_argument("--noise_schedule", default='cosine', choices=['linear', 'cosine'], type=str)
    group.add_argument("--diffusion_steps", default=1000, type=int,
                       help="Parsed but ignored, exactly like the reference (utils/model_util.py:40).")
    group.add_argument("--sigma_small", default=True, type=bool, help="Use smaller sigma values.")


def add_model_options(parser):
    group = parser.add_argument_group('model')
    group.add_argument("--arch", default='trans_enc', choices=['trans_enc', 'trans_dec', 'gru'], type=str)
    group.add_argument("--emb_trans_dec", default=False, type=bool)
    group.add_argument("--layers", default=8, type=int, help="Number of layers.")
    group.add_argument("--latent_dim", default=256, type=int, help="Transformer width.")
    group.add_argument("--cond_mask_prob", default=.1, type=float)
    group.add_argument("--lambda_rcxyz", default=0.0, type=float)
    group.add_argument("--lambda_vel", default=0.0, type=float)
    group.add_argument("--lambda_fc", default=0.0, type=float)
    group.add_argument("--unconstrained", action='store_true')
    group.add_argument("--use_text", action='store_true')
    group.add_argument("--use_audio", action='store_true')
    group.add_argument("--mfcc_input", action='store_true')
    group.add_argument("--use_wav_enc", action='store_true')
    group.add_argument("--seed_poses", type=int, default=10)


def add_data_options(parser):
    group = parser.add_argument_group('dataset')
    group.add_argument("--dataset", default='humanml', choices=['genea2022', 'genea2023'], type=str)
    group.add_argument("--data_dir", default="", type=str,
                       help="GENEA 2023 data directory ('' = the reference's ./dataset/Genea2023/).")
    group.add_argument("--num_frames", default=120, type=int)


def add_sampling_options(parser):
    group = parser.add_argument_group('sampling')
    group.add_argument("--model_path", default='', type=str,
                       help="Path to model####.pt (without it --synthetic and --data_dir runs use random weights).")
    group.add_argument("--output_dir", default='', type=str)
    group.add_argument("--num_samples", default=10, type=int)
    group.add_argument("--num_repetitions", default=3, type=int)
    group.add_argument("--guidance_param", default=2.5, type=float)


def add_generate_options(parser):
    group = parser.add_argument_group('generate')
    group.add_argument("--motion_length", default=6.0, type=float)
    group.add_argument("--input_text", default='', type=str)
    group.add_argument("--action_file", default='', type=str)
    group.add_argument("--text_prompt", default='', type=str)
    group.add_argument("--action_name", default='', type=str)


def add_native_options(parser):
    """Additive flags of the MI355X build (none exist in the reference)."""
    group = parser.add_argument_group('native')
    group.add_argument("--synthetic", action='store_true',
                       help="Random weights + N(0,1) seed poses / MFCCs (no dataset, no checkpoint needed).")
    group.add_argument("--synthetic_njoints", default=0, type=int,
                       help="Pose channels for --synthetic when --dataset is not a GENEA set (e.g. 263).")
    group.add_argument("--arch_version", default='mdm', choices=['mdm', 'mdm_old'],
                       help="mdm = V2 (model/mdm.py), mdm_old = V1 encoder-only topology (model/mdm_old.py).")
    group.add_argument("--sampler", default='p', choices=['p', 'ddim', 'plms', 'dpmpp', 'dpmpp_sde', 'unipc'],
                       help="p_sample_loop (reference default), ddim_sample_loop, plms_sample_loop, dpm_solver_sample_loop "
                            "(DPM-Solver++ multistep), dpm_solver_sde_sample_loop (its stochastic twin, orders 1 and 2) or "
                            "unipc_sample_loop (UniPC: a corrector on top of the multistep predictor, same forwards per step); use "
                            "the last three with --timestep_respacing logsnrN.")
    group.add_argument("--plms_order", default=2, type=int, choices=[2, 3, 4],
                       help="--sampler plms: order of the Adams-Bashforth multistep update.")
    group.add_argument("--dpm_order", default=2, type=int, choices=[1, 2, 3],
                       help="--sampler dpmpp: order of the multistep update (1 = DDIM at eta 0, 2 = 2M, 3 = 3M); "
                            "--sampler dpmpp_sde: 1 or 2.")
    group.add_argument("--unipc_order", default=2, type=int, choices=[1, 2, 3],
                       help="--sampler unipc: order of the predictor and the corrector (the corrected state is one order higher).")
    group.add_argument("--dpm_eta", default=1.0, type=float,
                       help="--sampler dpmpp_sde: scale of the injected noise (1 = the ancestral sampler's, 0 = --sampler dpmpp).")
    group.add_argument("--timestep_respacing", default='', type=str,
                       help="e.g. ddim100, or logsnr20 (at most 20 steps, even in log-SNR); '' = all 1000 steps.")
    group.add_argument("--eta", default=0.0, type=float)
    group.add_argument("--guidance_interval", default=None, type=int, nargs=2, metavar=("LO", "HI"),
                       help="Classifier-free guidance only while LO <= model timestep <= HI (0..999, after respacing; "
                            "inclusive); other steps take the conditional prediction and skip the unconditional pass. "
                            "Every sampler; an error with --guidance_param 1.")
    group.add_argument("--guidance_rescale", default=0.0, type=float, metavar="PHI",
                       help="Guidance rescale (Lin et al. 2023): scale each guided x0 prediction to the conditional one's "
                            "per-sample standard deviation and mix it with the unscaled one by PHI in [0, 1]; 0 = off. "
                            "Every sampler; an error with --guidance_param 1.")
    group.add_argument("--text_guidance_param", default=None, type=float, metavar="S",
                       help="--use_text: steer the text on its own in three passes per guided step (text+seed, one condition "
                            "dropped, neither): S scales the text stage, --guidance_param the seed-pose stage. An error without "
                            "--use_text, with --guidance_param 1, --guidance_drop, --guidance_refresh > 1, --layer_cache or "
                            "--parallel_window.")
    group.add_argument("--guidance_order", default=None, choices=["seed_text", "text_seed"],
                       help="--text_guidance_param: the condition stepped to first from the unconditional prediction "
                            "(default seed_text).")
    group.add_argument("--guidance_drop", default=None, choices=["both", "text", "seed"],
                       help="--use_text: what the contrast pass of classifier-free guidance drops (default both, the "
                            "unconditional pass); text keeps the seed poses out of the extrapolation, seed the text. Two passes "
                            "per guided step under the one scale --guidance_param.")
    group.add_argument("--pag_scale", default=None, type=float, metavar="W",
                       help="Perturbed-attention guidance (Ahn et al. 2024): contrast the conditional pass with one whose "
                            "self-attention map is the identity in the encoder layers --pag_layers, x0 = F + W (F - P). Needs no "
                            "condition dropout: with --guidance_param 1 it is the only guidance (two passes per guided step), "
                            "otherwise it is added to classifier-free guidance as a third pass. An error with "
                            "--text_guidance_param, --guidance_drop text|seed and --invert_gt; in the 3-pass case also with "
                            "--guidance_refresh > 1, --layer_cache and --parallel_window.")
    group.add_argument("--pag_layers", default=None, type=int, nargs="+", metavar="L",
                       help="--pag_scale: the perturbed encoder layers, distinct, 0 .. layers - 1 (default: the middle layer).")
    group.add_argument("--guidance_refresh", default=None, type=int, metavar="K",
                       help="Guidance refresh: run the unconditional pass only on every K-th guided denoiser call of a chunk's "
                            "loop and reuse the stored cond-uncond difference in between (1 = every call, the default). "
                            "Every sampler; an error with --guidance_param 1 or K < 1.")
    group.add_argument("--layer_cache", default=None, type=int, nargs=2, metavar=("EVERY", "KEEP"),
                       help="Layer cache: run every EVERY-th denoiser call of a chunk's loop in full and store the change its "
                            "encoder layers KEEP .. L-1 made; the calls in between recompute only the first KEEP layers and add "
                            "the stored change (EVERY = 1: every call in full, the default). Every sampler; an error with "
                            "EVERY < 1, KEEP outside 1 .. layers - 1, or --invert_gt.")
    group.add_argument("--invert_gt", action='store_true',
                       help="DDIM inversion of the data: each ground-truth chunk is carried up the deterministic DDIM ODE under "
                            "that chunk's conditioning with the conditional pass only (no guidance: the standard practice "
                            "for inversion), and the latent replaces the drawn x_T of the (guided) DDIM loop. "
                            "Needs --dataset genea2023 --data_dir D and --sampler ddim; with --guidance_param 1 the per-chunk "
                            "round-trip error max|regenerated - gt| / max|gt| is printed.")
    group.add_argument("--parallel_window", default=0, type=int, metavar="W",
                       help="Parallel-in-time sampling (ParaDiGMS): evaluate W consecutive states of a chunk's loop in one batched "
                            "denoiser call and advance past every state that has stopped changing (0 = off, at most 64). "
                            "--sampler p and ddim only; an error with --guidance_refresh > 1, --layer_cache and --invert_gt. "
                            "Implies --rng philox.")
    group.add_argument("--edit_mode", default=None, choices=['in_between', 'upper_body'], type=str,
                       help="Inpainting, with the reference's sample/edit.py flag names: in_between keeps each chunk's ground-truth "
                            "frames outside [prefix_end * T, suffix_start * T) and generates the gap (y['inpainting_mask'] / "
                            "y['inpainted_motion']); the ground truth is the data directory's, or under --synthetic drawn from the "
                            "run's seed. upper_body is not implemented (the reference's mask is HumanML's joint table).")
    group.add_argument("--prefix_end", default=0.25, type=float, help="--edit_mode in_between: end of the known prefix, a fraction of the chunk.")
    group.add_argument("--suffix_start", default=0.75, type=float, help="--edit_mode in_between: start of the known suffix, a fraction of the chunk.")
    group.add_argument("--resample", default=None, type=int, nargs=2, metavar=("JUMP", "REPEATS"),
                       help="RePaint resampling (Lugmayr et al. 2022): after every JUMP steps down, diffuse JUMP steps forward again "
                            "and come down again, REPEATS times in all, so that the generated frames catch up with the known ones "
                            "(REPEATS = 1: off). --sampler p and ddim only; allowed without --edit_mode; an error with "
                            "--guidance_refresh > 1, --layer_cache, --parallel_window and --invert_gt.")
    group.add_argument("--parallel_tolerance", default=0.1, type=float, metavar="TAU",
                       help="--parallel_window: a state counts as converged when its mean squared change is at most TAU^2 times "
                            "the step's posterior variance; 0 reproduces the sequential loop bit for bit in fp32.")
    group.add_argument("--text_features", default='', type=str, metavar="FILE.npz",
                       help="--use_text on a data directory: the CLIP text features of the run's texts, arrays `text` (strings) "
                            "and `features` (float32 [N, clip_dim]); every (take, chunk) text is looked up by exact match before "
                            "sampling starts.  This build has no CLIP tower: encode the strings of --list_texts with "
                            "clip.tokenize(texts, truncate=True) and clip_model.encode_text(tokens).float().")
    group.add_argument("--list_texts", default='', type=str, metavar="OUT.txt",
                       help="Write the distinct texts of the run's (take, chunk) windows, one per line, and exit (no GPU needed).")
    group.add_argument("--rng", default=None, choices=['torch', 'philox'],
                       help="torch = the reference's generator and draw order (single-GPU default); philox = in-kernel "
                            "counter-based noise keyed by the global sample index (shard invariant; multi-GPU default).")
    group.add_argument("--progress", action='store_true', help="tqdm bar over the denoising steps (reference: always on).")
    group.add_argument("--chunks", default=14, type=int, help="Autoregressive chunks per take (reference: 14).")
    group.add_argument("--synthetic_audio", action='store_true',
                       help="With --synthetic: derive y['mfcc'] from synthetic audio through the GPU MFCC front end "
                            "(dataset.py:81-95) instead of drawing N(0,1) features.")
    group.add_argument("--packed_cache", default='', type=str,
                       help="Directory of packed-weight images: the first run of a checkpoint writes the kernels' operand "
                            "layout there, later runs upload it instead of unpickling and repacking the checkpoint.")
    group.add_argument("--compute_dtype", default='fp32', choices=['fp32', 'fp16', 'bf16'],
                       help="fp32 = exact fp32 MFMA (reference precision); fp16 / bf16 = 16-bit MFMA operands and activation "
                            "stream, fp32 accumulate (bf16 trades 3 significant bits for fp32's exponent range).")


def generate_args(argv=None):
    parser = ArgumentParser()
    add_base_options(parser)
    add_sampling_options(parser)
    add_generate_options(parser)
    return parse_and_load_from_model(parser, argv)
