/*
 * gdx.h -- C ABI of libgdx.so: the MI355X-native (gfx950) diffusion-sampling hot path.
 *
 * Plain pointers and sizes only; every tensor argument is a DEVICE pointer owned by the
 * caller (PyTorch-ROCm in this repo), fp32 unless stated, laid out exactly like the
 * reference's tensors:
 *     pose tensors  [B, J, 1, T]   (J = njoints * nfeats, nfeats must be 1; T fastest)
 *     seed poses    [B, J, 1, P]   mfcc [B, 26, 1, T]   timesteps int64 [B]
 *     text features [B, clip_dim]  (use_text models only: the output of the caller's CLIP text tower, gdx_set_condition_text)
 * The library owns only its packed copy of the weights and its workspace.  One handle per
 * (device, stream); not thread-safe per handle; no hidden device synchronisation;
 * int status return (0 = ok, <0 = error, text via gdx_last_error()); no exceptions cross
 * the ABI.  `stream` is a hipStream_t passed as void*.
 *
 * The stream contract.  Every launch, copy and fill of a call goes to the `stream` it was given: any stream is accepted, the
 * null stream, a blocking or a non-blocking one (PyTorch's side streams are non-blocking), and the result has the same bits on
 * each.  The calls on ONE handle must be ordered by the caller -- one stream, or the caller's own events between streams: the
 * handle's workspace is shared by all of them.  Two handles may run on two streams at once.  gdx_prepare (which takes no
 * stream) zeroes what it allocates on the null stream and waits for that stream.  Workspace that a later call needs (its first
 * use of a feature, a loop with more steps than before) is allocated by that call and zeroed on that call's `stream`.
 * The entries that say "synchronises" wait for `stream`.  Nothing else waits.
 * tests/test_gpu_streams.py runs every entry with a `stream` on a non-default stream against its default-stream bits.
 *
 * The reference has no plugin ABI for this path: it is pure Python.  Each
 * entry point below names the reference Python interface it replaces; INTEGRATION.md shows
 * the ctypes stub a reference maintainer would add.
 */
#ifndef GDX_H
#define GDX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gdx_model* gdx_handle_t;

/* Rows of padding the library keeps behind every token-major buffer (its kernels read / store whole tiles); part of
 * the ABI only through gdx_mfcc's caller-provided workspace layout. */
#define GDX_ROW_PAD 256

enum { GDX_ARCH_MDM_OLD = 1,  /* model/mdm_old.py:11  MDM_Old ("V1") */
       GDX_ARCH_MDM = 2 };    /* model/mdm.py:10      MDM     ("V2") */

enum { GDX_COND = 0,          /* y without 'uncond'                     (model/mdm.py:111) */
       GDX_UNCOND = 1,        /* y['uncond'] = True: seed poses zeroed  (model/mdm.py:127,242-250) */
       GDX_CFG = 2 };         /* both passes + blend                    (model/cfg_sampler.py:23-28) */

enum { GDX_DTYPE_F32 = 0,     /* every GEMM on the exact fp32 MFMA (default; parity tolerance of the fp32 path) */
       GDX_DTYPE_F16 = 1,     /* fp16 MFMA operands (weights + activations), fp32 accumulate / LayerNorm statistics / softmax:
                                 BASELINE config 5's reduced-precision mode */
       GDX_DTYPE_BF16 = 2 };  /* the same mode with bf16 elements: fp32's exponent range (fp16 overflows at 65 504) for 8 instead of
                                 11 significant bits; the same kernels compiled for __bf16.  The residual stream (x + sublayer(x),
                                 LayerNorm in / out) stays fp32 in this mode, only the GEMM / attention operands are bf16.
                                 Stated tolerance against the reference's fp32 outputs, both 16-bit modes: 2e-2 of max|ref| for
                                 forwards and whole loops; under classifier-free guidance with scale s the blend (1-s) u + s c of two
                                 forwards is held to 2e-2 * (|s| + |1-s|)  (gesturediffusion_amd/numerics.py).  Measured: fp16
                                 <= 2.6e-3 with or without guidance; bf16 forwards <= 1.2e-2, guided + clipped loops at s <= 2.5
                                 <= 1.6e-2 (profiles/r03a_bf16_stream32_ab.txt; with a bf16 stream they reached 2.9e-2) */

enum { GDX_SAMPLER_P = 0,     /* p_sample      diffusion/gaussian_diffusion.py:496-548 */
       GDX_SAMPLER_DDIM = 1 };/* ddim_sample   diffusion/gaussian_diffusion.py:732-782 */

/* Constructor arguments of MDM / MDM_Old that shape the computation
 * (model/mdm.py:11-13, utils/model_util.py:18-34). */
typedef struct {
    int32_t arch;        /* GDX_ARCH_* */
    int32_t njoints;     /* njoints * nfeats */
    int32_t latent_dim;  /* d, multiple of 32 */
    int32_t ff_size;     /* multiple of 32 */
    int32_t num_layers;
    int32_t num_heads;   /* head_dim = latent_dim / num_heads in {32, 64, 96, 128, 192, 256} */
    int32_t seed_poses;
    int32_t mfcc_dim;    /* 26 (model/mdm.py:57) */
    int32_t cl_head;     /* 8  (model/mdm.py:71), V2 only */
    int32_t window;      /* 10 (model/mdm.py:75), V2 only */
    int32_t compute_dtype;   /* GDX_DTYPE_*.  The reference samples in fp32 only (its `use_fp16` is a deprecated
                                trainer switch, train/training_loop.py:43); fp16 is this library's additive mode */
    int32_t text_dim;    /* use_text (model/mdm.py:36-50), V2 only: width of embed_text's output, 0 < text_dim < latent_dim; the
                            seed-pose encoder then has latent_dim - text_dim rows.  0 = no text (with clip_dim 0) */
    int32_t clip_dim;    /* use_text: width of the text features the caller supplies (512 for CLIP ViT-B/32); 0 without text */
} gdx_config_t;

/* ---- lifetime ------------------------------------------------------------------------- */
/* replaces MDM.__init__ / MDM_Old.__init__ (model/mdm.py:11-103, model/mdm_old.py:11-75). */
int gdx_create(const gdx_config_t* cfg, gdx_handle_t* out);
int gdx_destroy(gdx_handle_t h);
/* last error text of the calling thread ("" if none). */
const char* gdx_last_error(void);

/* replaces nn.Module.load_state_dict for one entry (utils/model_util.py:6-9): `name` is the
 * reference state-dict key, `dev_ptr` fp32 device data of `shape`; the library keeps its own
 * packed (K-padded) copy.  Buffers `sequence_pos_encoder.pe` [max_len,1,d] (model/mdm.py:277-289)
 * and, for V2, the rotary cos/sin tables are passed the same way under the names
 * "sequence_pos_encoder.pe", "rope.cos", "rope.sin" ([max_pos, d/cl_head/2]). */
int gdx_set_weight(gdx_handle_t h, const char* name, const float* dev_ptr,
                   const int64_t* shape, int32_t ndim, void* stream);
/* 0 when every parameter the architecture needs has been set, else <0 and the missing
 * names in gdx_last_error(). */
int gdx_weights_ready(gdx_handle_t h);

/* ---- packed-weight image: the weight pre-packing cache -------------------- */
/* The reference re-reads a checkpoint written by train/training_loop.py:265-285 through utils/model_util.py:6-9 on every
 * start.  gdx_set_weight turns each tensor into the kernels' operand layout (zero-padded K-contiguous panels, their fp16
 * twins in the fp16 mode, padded bias / LayerNorm vectors, positional and rotary tables); these three calls move that
 * whole layout out of and into a handle as ONE host blob, so a caller can keep it next to the checkpoint and skip the
 * per-tensor path.  The blob starts with a magic, the gdx_config_t it was built for and a 64-bit checksum of its payload;
 * gdx_import_packed refuses (and leaves the handle untouched) unless the configuration, the compute dtype, every record's
 * dimensions and the checksum match what this handle computes for itself.  Once validation has passed the upload starts and
 * the handle counts as "weights not set" until it has completed: a failed allocation or copy leaves gdx_weights_ready()
 * failing, never a half-uploaded model.  After a successful import gdx_weights_ready() holds.  An image written before
 * gdx_config_t had text_dim / clip_dim carries a shorter header: its record count lies where text_dim is read, so every handle
 * refuses it as "built for another configuration" (utils/model_util.py load_model_cached then re-packs from the checkpoint).
 *   gdx_packed_bytes : size of the blob for this handle (all weights must be set)
 *   gdx_export_packed: fill `host` (exactly that many bytes); synchronises `stream`
 *   gdx_import_packed: upload a blob; synchronises `stream` (the caller may free `host` on return) */
int gdx_packed_bytes(gdx_handle_t h, int64_t* bytes);
int gdx_export_packed(gdx_handle_t h, void* host, int64_t bytes, void* stream);
int gdx_import_packed(gdx_handle_t h, const void* host, int64_t bytes, void* stream);

/* ---- per-problem set-up ---------------------------------------------------------------- */
/* Size the workspace for `batch` samples of `frames` frames (allocates; not capturable).
 * V2 requires frames % window == 0 (the reference's einops rearrange raises,
 * model/local_attention.py:104,110).  The GEMMs address their operands through 32-bit buffer offsets: a forward whose
 * largest operand (rows x 3 * latent_dim, or rows x ff_size, in the compute dtype) reaches 2 GiB fails with "an operand
 * exceeds the 2 GiB buffer-descriptor range; run the batch in smaller pieces" -- fp32 at the BASELINE width: a little
 * under 3 000 samples of 197 tokens in ONE call (bench.py --config 4 runs its 2 048 samples as sub-batches of 256). */
int gdx_prepare(gdx_handle_t h, int32_t batch, int32_t frames);

/* Step-invariant conditioning (hoisted out of the 1000-step loop): seed-pose embedding for the
 * cond and uncond passes (model/mdm.py:125-127), the MFCC slice of the input / project_to_lat
 * linear (model/mdm.py:133-169, model/mdm_old.py:104-108).  seed [B,J,1,P], mfcc [B,26,1,T]. */
int gdx_set_condition(gdx_handle_t h, const float* seed, const float* mfcc, void* stream);

/* The same for a handle with text_dim > 0 (MDM(use_text=True), model/mdm.py:118-127,154-160).  text [B, clip_dim] holds what the
 * reference's clip_model.encode_text(tokenize(y['text'])).float() returns: the CLIP tower and its tokenizer are the caller's (the
 * reference's trainer strips clip_model.* from every checkpoint, train/training_loop.py:269-272, so a checkpoint holds only
 * embed_text and the narrower seed-pose encoder).  Row b of the coarse condition becomes
 *     cond   [ embed_text(text_b) | seed_embed(seed_b) ]      text in columns 0 .. text_dim-1, the seed in the rest
 *     uncond [ embed_text.bias    | seed_embed.bias    ]      both inputs zeroed before their Linear (mask_cond, :242-250)
 * and everything behind it is gdx_set_condition's.  Each of the two entries refuses a handle of the other kind, naming the entry
 * to call; like every refusal of either (null pointer, no gdx_prepare, weights missing) that happens before any device work. */
int gdx_set_condition_text(gdx_handle_t h, const float* seed, const float* mfcc, const float* text, void* stream);

/* Per-condition guidance for a handle with text_dim > 0 (compositional classifier-free guidance, Liu et al. 2022,
 * arXiv:2206.01714; the two-scale form of Brooks et al. 2023, arXiv:2211.09800, section 3.2).  The reference's trainer drops the
 * text features and the seed poses independently (mask_cond is called once on each, model/mdm.py:121,127,242-250), so a use_text
 * checkpoint has seen four conditioning states.  Per sample, with the MFCC term unchanged in all four (audio is never dropped):
 *     F  text + seed   [ embed_text(text) | seed_embed(seed) ]     the conditional pass
 *     S  seed only     [ embed_text.bias  | seed_embed(seed) ]     the text features zeroed in front of embed_text
 *     X  text only     [ embed_text(text) | seed_embed.bias  ]     the flat seed poses zeroed in front of seed_embed
 *     U  neither       [ embed_text.bias  | seed_embed.bias  ]     the unconditional pass
 * The mode says which of them a guided call (GDX_CFG inside the guidance interval) runs, as row groups of ONE batch in the order
 * given, and how it combines them; every difference, product and sum is a separate fp32 operation in the order written:
 *     GDX_GUIDE_JOINT      (F, U)     g = U + s*(F - U)                       the state after gdx_create
 *     GDX_GUIDE_TEXT       (F, S)     g = S + s*(F - S)                       the text steered, the seed kept out of the contrast
 *     GDX_GUIDE_SEED       (F, X)     g = X + s*(F - X)
 *     GDX_GUIDE_SEED_TEXT  (F, S, U)  g = (U + s0*(S - U)) + s1*(F - S)       3 passes: first to the seed, then to the text
 *     GDX_GUIDE_TEXT_SEED  (F, X, U)  g = (U + s0*(X - U)) + s1*(F - X)       3 passes
 * Modes 1 and 2 are the two-group guided call of JOINT with other rows in the second group: every path of a guided call applies
 * unchanged (token-major, graph replay, refresh, layer cache, rescale) and `scale` stays [B].  GDX_UNCOND gives U in every mode.
 * In the 3-pass modes every entry that takes `scale` -- gdx_forward and the scale field of every loop argument struct -- reads
 * it as [2][B] contiguous under GDX_CFG: row 0 is s0 (it multiplies M - U, M the middle pass), row 1 is s1 (F - M).  No struct
 * layout changes.  A guided 3-pass call runs 3 * batch samples (gdx_forward_samples, the 2 GiB operand check); a call outside the
 * guidance interval runs GDX_COND on batch samples and computes neither contrast pass; gdx_forward, whose timesteps are on the
 * device, keeps the triple batch and selects per sample like the blend does.  The loops compose in place on the conditional third
 * of the prediction and call the unchanged step kernel with x0_uncond = scale = NULL, as the guidance rescale does; gdx_sample_loop
 * takes the pose-layout path and graph replay runs such a call eagerly.  The guidance rescale applies in every mode under its rule
 * with c = F and g = the composed prediction.
 * Refused in a 3-pass mode under GDX_CFG, before the first launch: the guidance refresh (every > 1) and the layer cache
 * (every > 1) in every loop that takes part in them -- their buffers and the covers() rule are written for two row groups -- and
 * gdx_parallel_loop.
 * gdx_set_guidance_compose: a null handle, an unknown mode, or a mode other than GDX_GUIDE_JOINT on a handle with text_dim == 0
 * (one droppable condition, nothing to compose) is refused before any HIP call.  The conditioning rows depend on the mode: the
 * call clears the conditioning (condition again before the next forward) and the stored guidance difference and layer change.
 * When the number of row groups changes (2 <-> 3) the workspace is prepared again at the current shape (allocates). */
enum { GDX_GUIDE_JOINT = 0, GDX_GUIDE_TEXT = 1, GDX_GUIDE_SEED = 2, GDX_GUIDE_SEED_TEXT = 3, GDX_GUIDE_TEXT_SEED = 4 };
int gdx_set_guidance_compose(gdx_handle_t h, int32_t mode);

/* Perturbed-attention guidance (PAG; Ahn et al. 2024, arXiv:2403.17377; no counterpart in the reference).  The contrast pass P is
 * the conditional forward F -- the same conditioning rows -- in which the self-attention map of chosen encoder layers is replaced
 * by the identity: every token attends to itself alone, so ctx = V.  It needs no condition dropout at training time.  `kind`
 * says what a guided call (GDX_CFG inside the guidance interval) runs, as row groups of ONE batch in the order given; every
 * difference, product and sum is a separate fp32 operation in the order written:
 *     GDX_PAG_OFF   the state after gdx_create: nothing new is launched, every result keeps its bits
 *     GDX_PAG_ONLY  (F, P)     g = P + s*(F - P)                       scale [B]; s = 1 + w gives the paper's F + w*(F - P)
 *     GDX_PAG_CFG   (F, P, U)  g = (U + s0*(F - U)) + s1*(F - P)       scale [2][B]: row 0 = s0 (CFG), row 1 = s1 (PAG)
 * GDX_PAG_ONLY is the two-group guided call with P where U stood: the step kernels, the token-major path, graph replay, the
 * refresh, the rescale and the layer cache apply unchanged with u := P.  GDX_PAG_CFG composes in place on the conditional third
 * like the 3-pass modes of gdx_set_guidance_compose, runs 3 * batch samples, applies the guidance rescale with c = F, and has
 * their conflicts: the refresh (every > 1), the layer cache (every > 1) and gdx_parallel_loop are refused before the first launch.
 * Bit l of layer_mask: in encoder layer l the rows of group P get the identity (gdx_attention_identity) instead of
 * self-attention; the attention kernels run on the other groups' rows only, and all other layers and rows run as without PAG.
 * GDX_COND and GDX_UNCOND calls are never perturbed, nor is V2's local-attention front end; GDX_UNCOND reads U in every kind
 * (the all-dropped rows are kept in group 2).  gdx_forward_flops leaves out the attention core of the perturbed (layer, group)
 * pairs.  A guided call with kind != GDX_PAG_OFF on a handle whose compose mode is not GDX_GUIDE_JOINT is refused before its
 * first launch (four row groups are not supported).
 * gdx_set_attention_guidance: a null handle, an unknown kind, a mask bit >= num_layers, or num_layers > 64 with kind !=
 * GDX_PAG_OFF is refused before any HIP call, and the handle stays as it was.  The call clears the stored guidance difference and
 * layer change; when the place of the U rows changes (kind 0 <-> not 0) it clears the conditioning (condition again before the
 * next forward), and when the number of row groups changes the workspace is prepared again at the current shape (allocates). */
enum { GDX_PAG_OFF = 0, GDX_PAG_ONLY = 1, GDX_PAG_CFG = 2 };
int gdx_set_attention_guidance(gdx_handle_t h, int32_t kind, uint64_t layer_mask);

/* ctx[r][c] = qkv[r][2*d + c] for r < rows, c < d: what self-attention gives when its map is the identity, as a bit copy of
 * elem_bytes-wide elements (4 = fp32, 2 = fp16 or bf16) in 128-bit accesses.  qkv is [rows][3*d], ctx [rows][d]; nothing outside
 * rows * d elements of ctx is written.  A test entry of the kernel the forwards launch on their own stream: it takes none, waits
 * for the device's pending work (the operands, on whatever stream they were written), runs on the null stream and returns when
 * the copy is done.  Refused before the first HIP call: elem_bytes not 2 or 4, a null pointer, a non-positive size, d * elem_bytes
 * not a multiple of 16, a pointer that is not 16-byte aligned. */
int gdx_attention_identity(int32_t elem_bytes, int64_t rows, int32_t d, const void* qkv, void* ctx);

/* Guidance interval (limited-interval guidance, Kynkaanniemi et al. 2024, arXiv:2404.07724; no counterpart in the reference):
 * the MODEL timesteps -- the values the denoiser sees after the respacing map, 0..999 for the reference's schedule -- at which
 * GDX_CFG means guidance, bounds inclusive.  Per-handle state like the conditioning; after gdx_create it is every timestep
 * (INT64_MIN, INT64_MAX).  One rule everywhere:
 *   lo <= tau <= hi : guided, exactly u + scale*(c - u)
 *   otherwise       : unguided, the x0 prediction is the conditional output c itself (not a blend at scale 1: other bits)
 *   lo > hi         : a legal empty interval, never guided
 * In the loops (gdx_sample_loop, gdx_plms_loop, gdx_dpm_loop, gdx_dpm_sde_loop, gdx_unipc_loop, gdx_bpd_loop) the host decides per step from
 * timestep_map[index]: an unguided step of a GDX_CFG loop runs the denoiser as GDX_COND on B samples -- the unconditional
 * pass is never computed -- and its update gets x0_uncond = scale = NULL; both forwards of gdx_plms_loop's first step take
 * the mode of their own timestep.  Inpainting, clip_denoised, the noise and the multistep history apply after the choice of
 * x0, unchanged.  gdx_forward under GDX_CFG has its timesteps on the device, so it keeps the double batch and selects per
 * sample in the blend kernel (no saving there).  Modes other than GDX_CFG ignore the interval.  A null handle fails before
 * any HIP call. */
int gdx_set_guidance_interval(gdx_handle_t h, int64_t lo, int64_t hi);

/* Guidance rescale (Lin et al. 2023, "Common Diffusion Noise Schedules and Sample Steps are Flawed", arXiv:2305.08891,
 * section 3.4; no counterpart in the reference): the guided x0 prediction of a sample is scaled so that its standard deviation
 * over the sample's N = J*T elements matches the conditional output's, mixed with the unscaled one by phi.  One rule everywhere,
 * for sample b with conditional output c, unconditional u and s = scale[b]:
 *   g_i  = u_i + s*(c_i - u_i)                        fp32, exactly the blend of today
 *   S_c = sum c_i, Q_c = sum c_i^2, S_g = sum g_i, Q_g = sum g_i^2         accumulated in fp64
 *   SS_c = max(Q_c - S_c^2/N, 0),  SS_g = max(Q_g - S_g^2/N, 0)
 *   r    = SS_g > 0 ? sqrt(SS_c / SS_g) : 1           (= std(c)/std(g))
 *   f    = (float)(phi*r + (1 - phi))                 fp64 expression on phi widened from float, rounded once
 *   out_i = fl32(g_i * f)
 * The statistics are over the raw model outputs of the whole sample; inpainting and clip_denoised apply afterwards, in the step
 * kernel, unchanged.  An unguided sample (guidance interval) keeps c, f = 1.  A constant guided output gives f = 1.  A NaN or
 * infinity in a sample makes that sample's f and output NaN and touches no other sample.  fp64 sums: an fp32 value widens
 * exactly and its square is exact in fp64, so f is within one fp32 ulp of any other fp64 evaluation whatever the summation
 * order; an fp32 one-pass sum loses the variance at |mean| >> std.
 *
 * gdx_set_guidance_rescale: per-handle state like the guidance interval, 0 (off) after gdx_create; phi outside [0, 1] (NaN
 * included) or a null handle is refused before any HIP call.  With phi > 0, gdx_forward under GDX_CFG and every guided step of
 * the in-library loops (gdx_sample_loop, gdx_plms_loop, gdx_dpm_loop, gdx_dpm_sde_loop, gdx_unipc_loop, gdx_bpd_loop) run gdx_cfg_rescale between
 * the denoiser and the step kernel, which then gets x0_uncond = scale = NULL like an unguided step; a guided step still runs
 * 2 * batch samples.  With phi == 0 nothing is launched and every result keeps its bits.  There is no token-major variant of
 * the rescale: a gdx_sample_loop call with phi > 0 and at least one guided step takes the pose-layout path (two transposes per
 * step more than the token-major path).  Graph replay captures the three launches with the step. */
int gdx_set_guidance_rescale(gdx_handle_t h, float phi);

/* The stand-alone operation, three launches on `stream`: per-chunk fp64 sums (grid (ceil(J*T / GDX_BPD_CHUNK), batch), no
 * atomics: a sample's numbers do not depend on the batch around it), the factor of every sample, the streaming pass.
 * Refusals (a null struct or pointer other than t, non-positive sizes, batch > 65535, phi outside [0, 1]) come before the first
 * HIP call.  At phi = 0 it still computes: f = 1 exactly and out = g. */
typedef struct {
    int32_t batch, njoints, frames;
    const float* x0_cond;      /* [B,J,1,T] */
    const float* x0_uncond;    /* [B,J,1,T] */
    const float* scale;        /* [B] */
    float phi;
    const int64_t* t;          /* device [B] model timesteps, or NULL: every sample guided */
    int64_t lo, hi;            /* with t: sample b is guided when lo <= t[b] <= hi (the rule of gdx_set_guidance_interval) */
    double* workspace;         /* device, 4 * batch * ceil(J*T / GDX_BPD_CHUNK) doubles, the caller's */
    float* factor;             /* out [B]: f, 1 for an unguided sample */
    float* out;                /* [B,J,1,T]; may alias x0_cond */
} gdx_cfg_rescale_args_t;
int gdx_cfg_rescale(const gdx_cfg_rescale_args_t* a, void* stream);

/* Guidance refresh (the cond-uncond difference reused between guided calls, after "compress guidance" / CFG-cache samplers;
 * no counterpart in the reference): the unconditional pass runs only on every `every`-th guided denoiser call of a loop, the
 * calls in between reuse the stored difference d = c - u.  every = 1 (the state after gdx_create) is the behaviour without
 * the feature: nothing new is launched and every result keeps its bits.  One rule everywhere:
 *   Number the loop's guided denoiser calls n = 0, 1, 2, ... in execution order.  A call is guided when the loop's mode is
 *   GDX_CFG and the call's model timestep passes the handle's guidance interval.  gdx_plms_loop's first step makes two calls,
 *   at index i and then at (i - 1) mod num_steps; each is numbered on its own timestep, like any other call.
 *   refresh call (n % every == 0): exactly the guided call of every = 1 -- the 2 * batch forward, raw outputs c and u -- and in
 *     addition d_i = fl32(c_i - u_i) is stored for every element of the batch; then the step continues unchanged (the step
 *     kernel blends, or gdx_cfg_rescale runs when phi > 0).  A refresh step's output has the bits of every = 1.
 *   reuse call (otherwise): the denoiser runs as GDX_COND on batch samples -- the unconditional pass is never computed,
 *     gdx_forward_samples advances by batch -- and u'_i = fl32(c_i - d_i) is written where the unconditional half of the
 *     output would be; the step continues exactly like a guided step with operands (c, u', scale): the blend u' + s*(c - u')
 *     in the unchanged step kernel, or the unchanged rescale when phi > 0.  Inpainting, clip_denoised, the noise and the
 *     multistep history follow, untouched.
 *   unguided calls (outside the interval) are neither counted nor changed.
 * State: the stored difference belongs to the handle (first use allocates it, gdx_prepare resets it) and carries a validity
 * flag that a refresh sets and gdx_prepare, gdx_set_condition and gdx_set_guidance_refresh clear.  A reuse call without a
 * valid difference is refused before anything is launched: a block-wise call must continue the loop that stored the
 * difference.  Block-wise issue (run_steps / k_base): the host derives the n of a call from timestep_map, the whole loop's
 * first index first_index + k_base and, for gdx_plms_loop, the second call of step 0 -- no counter lives in the handle -- so
 * issue in blocks gives the bits of one call.
 * It applies in gdx_sample_loop, gdx_plms_loop, gdx_dpm_loop, gdx_dpm_sde_loop and gdx_unipc_loop.  There is no token-major variant: a
 * gdx_sample_loop call with every > 1 and at least one guided step takes the pose-layout path (two transposes per step more
 * than the token-major path), and graph replay runs such a call eagerly.  gdx_forward and gdx_bpd_loop keep every guided call a
 * full one and never touch the stored difference: the step-wise forward has no memory, and the bound's steps draw independent
 * x_t.  How far the result moves from the fully guided loop depends on the model; nothing is claimed about a trained
 * checkpoint.
 * gdx_set_guidance_refresh: every < 1 or a null handle is refused before any HIP call. */
int gdx_set_guidance_refresh(gdx_handle_t h, int32_t every);

/* The stand-alone pass behind both uses, one launch on `stream`: out_i = fl32(a_i - b_i) for i < count, a plain fp32
 * subtraction (store: a = c, b = u; apply: a = c, b = d).  128-bit accesses when count % 4 == 0 and every pointer is 16-byte
 * aligned, a scalar path with a tail otherwise; nothing is written past count.  out may alias b.  Refusals (a null struct or
 * pointer, a non-positive count) come before the first HIP call. */
typedef struct {
    int64_t count;
    const float* a;
    const float* b;
    float* out;
} gdx_cfg_delta_args_t;
int gdx_cfg_delta(const gdx_cfg_delta_args_t* a, void* stream);

/* Host-side count of the samples pushed through the denoiser since gdx_create: every forward adds the batch it ran (2 * batch
 * under guidance, batch otherwise; a replayed graph step counts like an eager one).  Issues no GPU work: a test reads off it
 * that an unguided step skipped the unconditional pass instead of computing and discarding it. */
int gdx_forward_samples(gdx_handle_t h, int64_t* samples);

/* Layer cache (the deep encoder layers' change reused between denoiser calls, after DeepCache, Ma et al. 2023, arXiv:2312.00858,
 * and the transformer block-caching samplers, arXiv:2406.01125, arXiv:2312.03209; no counterpart in the reference): every
 * `every`-th denoiser call of a loop runs in full and stores the change its layers keep .. L-1 made to the residual stream;
 * the calls in between recompute only layers 0 .. keep-1 and add the stored change.  every = 1 (the state after gdx_create)
 * is the behaviour without the feature: nothing new is launched and every result keeps its bits; keep is then not looked at.
 * One rule everywhere (L = num_layers, d = latent_dim, B = batch, Beff = the samples the call runs):
 *   Number ALL denoiser calls of a loop m = 0, 1, 2, ... in execution order: the second call of gdx_plms_loop's first step is
 *   counted, and so are the unguided calls of a guidance interval and the reuse calls of the guidance refresh.  The call's
 *   forward mode c_m is what the denoiser is actually run with: GDX_COND, GDX_UNCOND or GDX_CFG (a refresh call is GDX_CFG; a
 *   refresh-reuse call and a call outside the guidance interval are GDX_COND).  K is the mode stored by the loop's most recent
 *   full call (none at the loop's start), and covers(K, c) = (K == c) or (K == GDX_CFG and c == GDX_COND): the conditional
 *   rows are the first B.
 *   full call (m % every == 0, or not covers(K, c_m)): exactly the forward of every = 1, with the same bits of x0.  In
 *     addition delta[b,t,j] = fl32(out[b,t,j] - in[b,t+1,j]) is stored for every row (b, t), 0 <= t < T, of the Beff samples
 *     and every column j < d, where `in` is the residual stream after encoder layer keep-1 (rows [Beff, T+1, d], token 0
 *     skipped) and `out` the operand the output GEMM reads ([Beff, T, d]).  Both are read as fp32: the fp32 buffer where the
 *     residual stream is fp32 (the fp32 mode, and bf16 with its fp32 stream), the widened 16-bit value otherwise (fp16 `in`;
 *     `out` in both 16-bit modes).  It sets K = c_m.
 *   partial call (otherwise): everything up to and including layer keep-1 runs as in a full call, with this call's own
 *     input, timestep embedding and conditioning.  Layers keep .. L-1 are not launched: no QKV GEMM, no attention, no FFN.
 *     The output GEMM's operand is formed as xc[b,t,j] = fl32(in'[b,t+1,j] + delta[b,t,j]), rounded once more to the 16-bit
 *     type in the 16-bit modes; a GDX_COND call under K = GDX_CFG uses rows 0 .. B-1 of delta.  The output GEMM, the
 *     transpose, the guidance refresh, the rescale and the step kernel follow, untouched.
 * State: delta and the buffer that holds `in` until the end of a full call belong to the handle (first use allocates them,
 * with guard zones under gdx_set_guards; gdx_prepare resets them).  A validity flag plus the stored mode are set by a full
 * call and cleared by gdx_prepare, gdx_set_condition, gdx_set_condition_text and gdx_set_layer_cache.  No counter lives in the
 * handle: for block-wise issue (run_steps / k_base) the host derives every call's m, c_m and K from the whole loop's first
 * index first_index + k_base, as it does for the guidance refresh, so issue in blocks gives the bits of one call.  A block that
 * would begin with a partial call without a valid delta of the planned mode is refused before its first launch.
 * It applies in gdx_sample_loop (pose-layout AND token-major paths), gdx_plms_loop, gdx_dpm_loop, gdx_dpm_sde_loop and
 * gdx_unipc_loop; graph replay runs a call with every > 1 eagerly.  gdx_forward, gdx_bpd_loop and gdx_ddim_reverse_loop keep
 * every call full and never touch delta.  The encoder part of a step falls to (1 + (every-1)*keep/L) / every of itself; how far
 * the result moves from the uncached loop depends on the model, and nothing is claimed about motion quality on a trained
 * checkpoint.
 * gdx_set_layer_cache: every < 1, a null handle, or every > 1 with keep outside 1 .. num_layers - 1 is refused before any HIP
 * call. */
int gdx_set_layer_cache(gdx_handle_t h, int32_t every, int32_t keep);

/* The stand-alone pass behind both uses, one launch on `stream`.  op 0 (store) reads in and outc and writes delta; op 1 (apply)
 * reads in and delta and writes outc.  in [batch, frames + 1, width] of in_dtype, outc [batch, frames, width] of out_dtype,
 * delta [batch, frames, width] fp32; row (b, t) of outc and delta pairs with row (b, t + 1) of in.  (in_dtype, out_dtype) is one
 * of (GDX_DTYPE_F32, GDX_DTYPE_F32), (GDX_DTYPE_F16, GDX_DTYPE_F16), (GDX_DTYPE_F32, GDX_DTYPE_BF16): the three the compute
 * modes use.  There is only a 128-bit path: width % 32 != 0 or a pointer that is not 16-byte aligned is refused, like another
 * op or pairing, a non-positive size and a null pointer, all before the first HIP call.  Nothing outside [batch, frames, width]
 * of the written operand is touched. */
int gdx_layer_delta(int32_t op, int32_t in_dtype, int32_t out_dtype, int32_t batch, int32_t frames, int32_t width,
                    const void* in, void* outc, float* delta, void* stream);

/* Host-side count of samples x encoder layers launched since gdx_create: every forward adds Beff * (the encoder layers it
 * launched), num_layers on a full call and keep on a partial one.  Issues no GPU work: a test reads off it that a partial call
 * skipped the deep layers. */
int gdx_forward_layer_samples(gdx_handle_t h, int64_t* n);

/* ---- denoiser -------------------------------------------------------------------------- */
/* replaces MDM.forward / MDM_Old.forward / ClassifierFreeSampleModel.forward
 * (model/mdm.py:105-224, model/mdm_old.py:84-122, model/cfg_sampler.py:23-28).
 * x [B,J,1,T]; timesteps int64 [B] (already mapped through timestep_map); mode GDX_COND /
 * GDX_UNCOND / GDX_CFG; scale [B] (GDX_CFG only, y['scale']); out [B,J,1,T] contiguous.  Under GDX_CFG sample b is blended
 * when timesteps[b] lies in the handle's guidance interval and is the conditional output otherwise.  In a 3-pass mode of
 * gdx_set_guidance_compose scale is [2][B] and the blend is that mode's composition. */
int gdx_forward(gdx_handle_t h, const float* x, const int64_t* timesteps, int32_t mode,
                const float* scale, float* out, void* stream);

/* Debug/parity taps: copy an internal activation to `out` (device).  which: 0 = encoder
 * input [B,T+1,d], 1..L = output of encoder layer l [B,T+1,d] (only the most recent
 * forward's last layer buffer is live unless keep_taps was set), see gdx_set_keep_taps.
 * which = L + 1 (under keep_taps): the output GEMM's operand of the most recent forward, [Beff, T, d], as fp32 (widened in
 * the 16-bit modes), for full and partial calls of the layer cache alike.  A partial call writes taps 0 .. keep only: taps
 * keep+1 .. L stay stale, holding an earlier forward's values. */
int gdx_set_keep_taps(gdx_handle_t h, int32_t keep);
int gdx_get_tap(gdx_handle_t h, int32_t which, float* out, int64_t count, void* stream);

/* Test aid: with guards on, every workspace buffer, whenever it is allocated, is followed by a 64 KiB canary
 * zone; gdx_check_guards synchronises `stream` and counts canary bytes that were overwritten (0 = no kernel stored past
 * a buffer); it fails when a workspace allocation has no zone.  first_bad_zone (optional) = allocation order index of the first damaged zone, -1 if none. */
int gdx_set_guards(gdx_handle_t h, int32_t on);
int gdx_check_guards(gdx_handle_t h, int64_t* bad_bytes, int32_t* first_bad_zone, void* stream);

/* ---- sampler update -------------------------------------------------------------------- */
/* One fused reverse-process update over [B,J,1,T] (replaces p_mean_variance's tail + p_sample /
 * ddim_sample: gaussian_diffusion.py:307-311,374-376,524-548,748-782 and the CFG blend
 * cfg_sampler.py:28).  Per element, with per-sample fp32 coefficient row c = coef[idx]:
 *   x0  = x0_cond                       or  u + scale*(c - u)   when x0_uncond != NULL
 *   x0  = x0*(1-m) + motion*m           when inpaint_mask != NULL
 *   x0  = clamp(x0, -1, 1)              when clip_denoised
 *   P   : out = (c[0]*x0 + c[1]*x) + c[2]*z
 *   DDIM: eps = (c[0]*x - x0)/c[1];  out = (x0*c[2] + c[3]*eps) + c[4]*z
 * with separately rounded products/sums (no FMA contraction), matching torch's op order.
 * idx = t[b] if t != NULL else step_index.  z = noise[...] if noise != NULL, else Philox4x32-10
 * N(0,1) keyed by (philox_seed; sample_offset+b [or sample 0 when const_noise]; rng_step; element).
 * coef: device [num_steps][8] fp32 rows built by the host with the reference's own rounding
 * (fp64 table -> .float(), gaussian_diffusion.py:1595-1608). */
typedef struct {
    int32_t kind;              /* GDX_SAMPLER_* */
    int32_t batch, njoints, frames;
    const float* coef;         /* [num_steps][8] */
    const int64_t* t;          /* [B] or NULL */
    int32_t step_index;        /* used when t == NULL */
    const float* x;            /* x_t */
    const float* x0_cond;      /* model output (cond pass) */
    const float* x0_uncond;    /* NULL or uncond pass */
    const float* scale;        /* [B] when x0_uncond != NULL */
    const uint8_t* inpaint_mask;   /* NULL or bool bytes [B,J,1,T] */
    const float* inpaint_motion;   /* [B,J,1,T] when mask != NULL */
    const float* noise;        /* NULL -> Philox */
    int32_t const_noise;       /* noise[[0]].repeat(B) (gaussian_diffusion.py:534-535) */
    uint64_t philox_seed;
    uint64_t sample_offset;    /* global index of sample 0 of this shard */
    uint32_t rng_step;
    float* out;                /* x_{t-1}; may alias x */
    float* pred_xstart;        /* NULL or [B,J,1,T]: x0 after CFG/inpainting */
    /* cond_fn guidance (gaussian_diffusion.py:418-494); both NULL when unused:
     *   P   : mean += c[3] * cond_grad            (condition_mean; c[3] = model variance of the step)
     *   DDIM: eps -= cond_coef[idx] * cond_grad, pred_xstart recomputed from it (condition_score;
     *         cond_coef[idx] = sqrt(1 - alpha_bar) in fp32, device [num_steps]) */
    const float* cond_grad;    /* [B,J,1,T] gradient returned by cond_fn */
    const float* cond_coef;
    int32_t clip_denoised;     /* x0 = clamp(x0, -1, 1) after the CFG / inpainting blends (process_xstart, :349-355) */
} gdx_update_args_t;
int gdx_sampler_update(const gdx_update_args_t* a, void* stream);

/* PLMS building blocks (plms_sample, gaussian_diffusion.py:995-1079), element-wise over [B, per_sample] with
 * separately rounded products / sums in the reference's op order.  coef rows as for gdx_sampler_update with the
 * DDIM layout (c[0] sqrt_recip_alphas_cumprod, c[1] sqrt_recipm1_alphas_cumprod, c[2] sqrt(alpha_bar_prev),
 * c[3] sqrt(1 - alpha_bar_prev)) plus c[7] = (t != 0).  idx = t[b] if t != NULL else step_index.
 *   kind 0: out = eps = (c0*x - pred_xstart) / c1                      (_predict_eps_from_xstart :407-411)
 *   kind 6: out = pred_xstart*c2 + c3*eps[0]                           (pseudo improved Euler predictor :1048)
 *   kind 7: out = pred_xstart under condition_score (:452-472): eps[0] = cond_fn gradient [B,J,1,T],
 *           eps[1] = device table sqrt(1 - alpha_bar)[num_steps]
 *   kind 8: out = c0*x - c1*pred_xstart-slot: the x0 prediction of a denoiser whose output is read as EPSILON (x = x_t,
 *           slot = the output, DDIM rows: _predict_xstart_from_eps :390-396) or as PREVIOUS_X (x = the output, slot = x_t,
 *           rows c0 = 1/posterior_mean_coef1, c1 = posterior_mean_coef2/posterior_mean_coef1: _predict_xstart_from_xprev :398-405)
 *   kind 1..4: Adams-Bashforth of that order over eps[0] (newest) .. eps[3]   (:1060-1069)
 *   kind 5: eps' = (eps[0] + eps[1]) / 2                               (improved Euler corrector :1050)
 *   kinds 1..5 then: pred' = c0*x - c1*eps';  out = (pred'*c2 + c3*eps')*nz + pred_xstart*(1 - nz)   (:1051-1077) */
typedef struct {
    int32_t kind;
    int32_t batch;
    int64_t per_sample;
    const float* coef;         /* [num_steps][8] */
    const int64_t* t;          /* [B] or NULL */
    int32_t step_index;
    const float* x;            /* x_t (unused by kind 6) */
    const float* pred_xstart;  /* model x0 after CFG / inpainting */
    const float* eps[4];       /* eps history, newest first (unused by kind 0) */
    float* out;
} gdx_plms_args_t;
int gdx_plms_update(const gdx_plms_args_t* a, void* stream);

/* One whole PLMS step over [B,J,1,T] in ONE pass, with the bits of the three launches it replaces (gdx_sampler_update's
 * pred_xstart output, gdx_plms_update kind 0, gdx_plms_update kind 1..6): per element, every product / sum / quotient rounded
 * separately, coefficient row c = coef[idx] (DDIM layout at eta = 0 as above), idx = t[b] if t != NULL else step_index:
 *   pred = x0_cond -> CFG blend u + scale*(c - u) -> inpainting blend -> clamp, exactly as in gdx_sampler_update
 *   eps  = (c0*x - pred) / c1, written to eps_out (the caller's history slot)
 *   kind 1..4: eps' = Adams-Bashforth of that order over eps (newest), eps_hist[0], eps_hist[1], eps_hist[2]
 *   kind 5   : the corrector of a loop's first step.  x0_cond / x0_uncond hold the SECOND forward's output, run on the
 *              predictor x_eps at row idx_e = t_eps[b] if t_eps != NULL else step_index_eps:  eps = (ce0*x_eps - pred) / ce1,
 *              eps' = (eps_hist[0] + eps) / 2 with eps_hist[0] the first forward's eps; eps_out may be NULL (the reference keeps
 *              the first eps in its history, :1043-1052)
 *   kind 1..5: pred' = c0*x - c1*eps';  out = (pred'*c2 + c3*eps')*nz + keep*(1 - nz),  nz = c7,  keep = pred (kind 5: pred_prev,
 *              the first forward's pred)
 *   kind 6   : out = pred*c2 + c3*eps, the improved-Euler predictor of a loop's first step (out must not alias x there:
 *              kind 5 reads x again)
 * History slots a kind does not use are never read.  128-bit accesses when J*T % 4 == 0 and every pointer is 16-byte aligned
 * (the mask 4-byte), a scalar path otherwise.  batch <= 65535 (the grid's second dimension is the sample). */
typedef struct {
    int32_t kind;              /* 1..6 */
    int32_t batch, njoints, frames;
    const float* coef;         /* [num_steps][8] */
    const int64_t* t;          /* [B] or NULL */
    const int64_t* t_eps;      /* kind 5: [B] or NULL */
    int32_t step_index;        /* used when t == NULL */
    int32_t step_index_eps;    /* kind 5, used when t_eps == NULL */
    const float* x;            /* x_t */
    const float* x_eps;        /* kind 5: the predictor the second forward ran on */
    const float* x0_cond;      /* model output (cond pass) */
    const float* x0_uncond;    /* NULL or uncond pass */
    const float* scale;        /* [B] when x0_uncond != NULL */
    const uint8_t* inpaint_mask;   /* NULL or bool bytes [B,J,1,T] */
    const float* inpaint_motion;   /* [B,J,1,T] when mask != NULL */
    int32_t clip_denoised;
    const float* eps_hist[3];  /* older eps, newest first: kind k <= 4 reads k - 1 of them, kind 5 one, kind 6 none */
    const float* pred_prev;    /* kind 5: pred of the first forward */
    float* eps_out;            /* this launch's eps; required except for kind 5 */
    float* out;                /* may alias x */
    float* pred_xstart;        /* NULL or [B,J,1,T]: pred */
} gdx_plms_step_args_t;
int gdx_plms_step(const gdx_plms_step_args_t* a, void* stream);

/* One DPM-Solver++ multistep step over [B,J,1,T] in ONE pass (Lu et al. 2022, arXiv:2211.01095: the data-prediction solver of
 * Algorithm 2 and its third-order extension; no counterpart in the reference).  With the diffusion's own (possibly respaced)
 * tables at index i: abar_i = alphas_cumprod[i], alpha_i = sqrt(abar_i), sigma_i = sqrt(1 - abar_i), lambda_i =
 * 0.5*log(abar_i / (1 - abar_i)); subscript p = the step's target, from alphas_cumprod_prev[i];  h = lambda_p - lambda_i,
 * a = sigma_p / sigma_i, phi = -alpha_p*expm1(-h);  m0 = this step's x0 prediction, m1 / m2 those of the two previous executed
 * steps (indices i+1, i+2);  r0 = (lambda_i - lambda_{i+1}) / h, r1 = (lambda_{i+1} - lambda_{i+2}) / h:
 *   order 1: x' = a*x + phi*m0                                     (DDIM at eta = 0)
 *   order 2: x' = a*x + phi*m0 + 0.5*phi*(m0 - m1)/r0                                                    (2M)
 *   order 3: D1_0 = (m0 - m1)/r0, D1_1 = (m1 - m2)/r1, D1 = D1_0 + r0/(r0 + r1)*(D1_0 - D1_1), D2 = (D1_0 - D1_1)/(r0 + r1),
 *            x' = a*x + phi*m0 + alpha_p*(expm1(-h)/h + 1)*D1 - alpha_p*((expm1(-h) + h)/h^2 - 0.5)*D2    (3M)
 * Every order is linear in (m0, m1, m2): the host collects the weights in fp64 and rounds them once to fp32.  coef: device
 * [num_steps][8] fp32 rows (a, w1_0, w2_0, w2_1, w3_0, w3_1, w3_2, 0), w{order}_{j} the weight of m_j; for every row and
 * order the weights sum to phi.  Row 0 (abar_p = 1, sigma_p = 0, h = inf) is (0, 1, 0, ...): x' = m0.  Entries that would
 * need an index >= num_steps are 0.  Neither kind of zero is selected by the order rule of gdx_dpm_loop.
 * Per element, row c = coef[idx], idx = t[b] if t != NULL else step_index, every product / sum rounded separately:
 *   m0 = x0_cond -> CFG blend u + scale*(c - u) -> inpainting blend -> clamp, exactly as in gdx_sampler_update
 *   D = w0*m0;  order >= 2: D = D + w1*hist[0];  order 3: D = D + w2*hist[1];  out = a*x + D
 * m0 is written to pred_out (optional; it must not be a history slot this order reads).  History slots the order does not use
 * are never read.  128-bit accesses when J*T % 4 == 0 and every pointer is 16-byte aligned (the mask 4-byte), a scalar path
 * otherwise.  batch <= 65535 (the grid's second dimension is the sample).  Refusals come before the first HIP call. */
typedef struct {
    int32_t order;             /* 1..3 */
    int32_t batch, njoints, frames;
    const float* coef;         /* [num_steps][8], rows as above */
    const int64_t* t;          /* [B] or NULL */
    int32_t step_index;        /* used when t == NULL */
    const float* x;            /* x_t */
    const float* x0_cond;      /* model output (cond pass) */
    const float* x0_uncond;    /* NULL or uncond pass */
    const float* scale;        /* [B] when x0_uncond != NULL */
    const uint8_t* inpaint_mask;   /* NULL or bool bytes [B,J,1,T] */
    const float* inpaint_motion;   /* [B,J,1,T] when mask != NULL */
    int32_t clip_denoised;
    const float* hist[2];      /* older x0 predictions, newest first: order k reads k - 1 of them */
    float* out;                /* may alias x */
    float* pred_out;           /* NULL or [B,J,1,T]: m0 */
} gdx_dpm_step_args_t;
int gdx_dpm_step(const gdx_dpm_step_args_t* a, void* stream);

/* One SDE-DPM-Solver++ multistep step over [B,J,1,T] in ONE pass: the stochastic twin of gdx_dpm_step, orders 1 and 2 (Lu et
 * al. 2022, arXiv:2211.01095, the SDE solver at eta = 1; eta >= 0 scales the injected noise in the midpoint form known from
 * k-diffusion's dpmpp_2m_sde, written here with alpha != 1; no counterpart in the reference).  Notation of gdx_dpm_step, and
 * z ~ N(0, I):
 *   a = (sigma_p / sigma_i)*exp(-eta*h),  phi = -alpha_p*expm1(-(1 + eta)*h),  s = sigma_p*sqrt(-expm1(-2*eta*h))
 *   order 1: x' = a*x + phi*m0 + s*z                (eta = 1: the ancestral step with the posterior variance; eta = 0: DDIM)
 *   order 2: x' = a*x + phi*m0 + 0.5*phi*(m0 - m1)/r0 + s*z
 * coef: device [num_steps][8] fp32 rows (a, w1_0, w2_0, w2_1, 0, 0, 0, s) for ONE eta, w1_0 = phi, w2_0 = phi + 0.5*phi/r0,
 * w2_1 = -0.5*phi/r0: the layout of gdx_dpm_step's rows with the noise scale in the spare column 7.  At eta = 0 columns 0..3
 * are those rows bit for bit and s = 0.  Row 0 is (0, 1, 0, 0, 0, 0, 0, 0): x' = m0 and no noise is applied (for finite x and
 * z).  Entries that would need an index >= num_steps are 0.
 * Per element, row c = coef[idx], idx = t[b] if t != NULL else step_index, every product / sum rounded separately:
 *   m0 as in gdx_dpm_step;  D = w0*m0;  order 2: D = D + w1*hist[0];  out = (a*x + D) + s*z
 * z = noise[b][..] when noise != NULL, else Philox N(0,1) keyed by (philox_seed; sample_offset + b; rng_step; element), the
 * keying of gdx_sampler_update and gdx_randn: a sample's noise does not depend on the batch it is drawn in.  m0 is written to
 * pred_out (optional; it must not be the history slot this order reads).  128-bit accesses when J*T % 4 == 0 and every
 * pointer is 16-byte aligned (the mask 4-byte), a scalar path otherwise.  batch <= 65535.  Refusals come before the first
 * HIP call. */
typedef struct {
    int32_t order;             /* 1..2 */
    int32_t batch, njoints, frames;
    const float* coef;         /* [num_steps][8], rows as above */
    const int64_t* t;          /* [B] or NULL */
    int32_t step_index;        /* used when t == NULL */
    const float* x;            /* x_t */
    const float* x0_cond;      /* model output (cond pass) */
    const float* x0_uncond;    /* NULL or uncond pass */
    const float* scale;        /* [B] when x0_uncond != NULL */
    const uint8_t* inpaint_mask;   /* NULL or bool bytes [B,J,1,T] */
    const float* inpaint_motion;   /* [B,J,1,T] when mask != NULL */
    int32_t clip_denoised;
    const float* hist[1];      /* the previous executed step's x0 prediction: read at order 2 */
    float* out;                /* may alias x */
    float* pred_out;           /* NULL or [B,J,1,T]: m0 */
    const float* noise;        /* NULL -> in-kernel Philox; else [B,J,1,T] */
    uint64_t philox_seed;
    uint64_t sample_offset;    /* global index of sample 0 of this shard */
    uint32_t rng_step;
} gdx_dpm_sde_step_args_t;
int gdx_dpm_sde_step(const gdx_dpm_sde_step_args_t* a, void* stream);

/* One UniPC step over [B,J,1,T] in ONE pass (Zhao et al. 2023, arXiv:2302.04867, the data-prediction form with B(h) = expm1(-h),
 * the paper's bh2; no counterpart in the reference): the x0 prediction m0 the denoiser just made is used twice -- to CORRECT the
 * step that led to the denoiser's input (one order of accuracy more, no further forward) and to PREDICT the next input.
 * Notation of gdx_dpm_step.  A step with base index b, target p = the target of b, h = lambda_p - lambda_b, E = expm1(-h) and the
 * predictions m_b, m_{b+1}, ... (older = larger index):  r_j = (lambda_{b+j} - lambda_b)/h (j = 1..q-1), r_q = 1,
 * D_j = (m_{b+j} - m_b)/r_j,  first = (sigma_p/sigma_b)*x - alpha_p*E*m_b;  with hh = -h:  g_1 = expm1(hh)/hh - 1,
 * g_{n+1} = g_n/hh - 1/(n+1)!,  beta_n = g_n*n!/E,  R[n][j] = r_j^(n-1) (n, j = 1..q):
 *   UniP-q (predictor, base b = i):  q = 1: x_p = first;  q = 2: rho = (1/2);  q = 3: rho solves the leading 2x2 block of R against
 *            (beta_1, beta_2);  x_p = first - alpha_p*E*sum_{j<q} rho_j*D_j.       UniP-1 is DDIM at eta = 0, UniP-2 is 2M.
 *   UniC-q (corrector, base b = i + 1, whose target is i; m_new = m_i, D_new = m_new - m_b):  q = 1: rho = (1/2), else rho solves
 *            R*rho = beta (q x q);  x_c = first - alpha_p*E*(sum_{j<q} rho_j*D_j + rho_q*D_new).
 * Both are linear in (x, m...): the host collects the weights in fp64 and rounds them once to fp32.
 * coef: device [num_steps][8] fp32 rows (a, w1_0, w2_0, w2_1, w3_0, w3_1, w3_2, 0), the layout of gdx_dpm_step's rows; columns
 * 0..3 ARE those rows bit for bit, columns 4..6 hold UniP-3.  coef_c: device [num_steps][16] fp32 rows; columns 4(q-1) ..
 * 4(q-1)+3 of row b hold (cn, c0, c1, c2) of UniC-q with base b -- the weights of m_new, m_b, m_{b+1}, m_{b+2}, zero-padded --
 * and columns 12..15 are 0.  Every non-zero weight set sums to -alpha_p*E of its row.  Row 0 of coef is (0, 1, 0, ...): the step
 * at index 0 returns m0; row 0 of coef_c is 0 (its h is infinite).  Entries that would need an index >= num_steps are 0.  Neither
 * kind of zero is selected by the order rule of gdx_unipc_loop.
 * Per element, idx = t[b] if t != NULL else step_index, c = coef[idx], every product / sum rounded separately:
 *   m0 = x0_cond -> CFG blend -> inpainting blend -> clamp, exactly as in gdx_dpm_step
 *   corr_order q >= 1:  (cn, c0, c1, c2) = coef_c[idx + 1][4(q-1) ..],  ab = coef[idx + 1][0];
 *       C = cn*m0;  C = C + c0*hist[0];  q >= 2: C = C + c1*hist[1];  q = 3: C = C + c2*hist[2];  xc = ab*x + C
 *   corr_order 0:  xc = x, bits untouched (row idx + 1 of neither table is read)
 *   pred_order p:  D = w0*m0;  p >= 2: D = D + w1*hist[0];  p = 3: D = D + w2*hist[1];  out = a*xc + D   (w = c's order-p columns)
 * xc goes to base_out (required; may alias x), x_p to out, m0 to pred_out (optional; it must not be a history slot the step
 * reads).  hist[j] = the prediction made j + 1 executed steps ago (index idx + 1 + j); max(corr_order, pred_order - 1) of them
 * are read, the others never.  Only the pairs the order rule of gdx_unipc_loop reaches exist: (corr, pred) = (0,1) (1,1) (1,2)
 * (2,2) (3,2) (2,3) (3,3); any other is refused.  128-bit accesses when J*T % 4 == 0 and every pointer is 16-byte aligned (the
 * mask 4-byte), a scalar path otherwise.  batch <= 65535.  Refusals come before the first HIP call. */
typedef struct {
    int32_t corr_order;        /* 0..3 */
    int32_t pred_order;        /* 1..3 */
    int32_t batch, njoints, frames;
    const float* coef;         /* [num_steps][8], rows as above */
    const float* coef_c;       /* [num_steps][16], rows as above; required when corr_order > 0 */
    const int64_t* t;          /* [B] or NULL */
    int32_t step_index;        /* used when t == NULL */
    const float* x;            /* corr_order > 0: the corrector's base state (index idx + 1, corrected); 0: the state */
    const float* x0_cond;      /* model output (cond pass) */
    const float* x0_uncond;    /* NULL or uncond pass */
    const float* scale;        /* [B] when x0_uncond != NULL */
    const uint8_t* inpaint_mask;   /* NULL or bool bytes [B,J,1,T] */
    const float* inpaint_motion;   /* [B,J,1,T] when mask != NULL */
    int32_t clip_denoised;
    const float* hist[3];      /* older x0 predictions, newest first */
    float* base_out;           /* xc; may alias x */
    float* out;                /* x_p; may alias x, not base_out */
    float* pred_out;           /* NULL or [B,J,1,T]: m0 */
} gdx_unipc_step_args_t;
int gdx_unipc_step(const gdx_unipc_step_args_t* a, void* stream);

/* One DDIM reverse-ODE (inversion) step x_i -> x_{i+1} over [B,J,1,T] in ONE pass (ddim_reverse_sample, gaussian_diffusion.py:841-877):
 * the deterministic DDIM step run towards MORE noise.  There is no noise operand and no random draw.  The operands are those of
 * the step structs above under the same names; this entry and gdx_ddim_reverse_loop take theirs as plain arguments, like
 * gdx_q_sample_t and gdx_mfcc (the set of argument structs of this header is kept as it is).
 *   batch, njoints, frames   the shape [B,J,1,T]
 *   coef                     device [num_steps][8] fp32 rows in the DDIM layout of gdx_sampler_update with the reverse rows of
 *                            coef_table(GDX_SAMPLER_DDIM, "reverse"): c0 = sqrt_recip_alphas_cumprod, c1 = sqrt_recipm1_alphas_cumprod,
 *                            c2 = sqrt(abar_next), c3 = sqrt(1 - abar_next), abar_next = alphas_cumprod_next[i] (0 behind the last
 *                            index: the step at num_steps - 1 returns eps)
 *   t, step_index            [B] or NULL; step_index is used when t == NULL
 *   x                        x_i
 *   x0_cond, x0_uncond, scale   model output (cond pass); NULL or the uncond pass; [B] when x0_uncond != NULL
 *   inpaint_mask, inpaint_motion   NULL or bool bytes [B,J,1,T]; [B,J,1,T] when mask != NULL
 *   clip_denoised
 *   out                      x_{i+1}; may alias x
 *   pred_out, eps_out        NULL or [B,J,1,T]: m0 and eps; they must differ from each other and from out
 * Per element, row c = coef[idx], idx = t[b] if t != NULL else step_index, every product / sum / quotient rounded separately in
 * the reference's op order:
 *   m0  = x0_cond -> CFG blend u + scale*(c - u) -> inpainting blend -> clamp, exactly as in gdx_sampler_update
 *   eps = (c0*x - m0) / c1
 *   out = m0*c2 + c3*eps
 * These are the bits of gdx_sampler_update with those rows and a zero noise tensor, up to the sign of a zero (that path adds
 * 0*0 last).  128-bit accesses when J*T % 4 == 0 and every pointer is 16-byte aligned (the mask 4-byte), a scalar path
 * otherwise; nothing is written past the tensor.  batch <= 65535 (the grid's second dimension is the sample).  Refusals come
 * before the first HIP call. */
int gdx_ddim_reverse_step(int32_t batch, int32_t njoints, int32_t frames, const float* coef, const int64_t* t, int32_t step_index,
                          const float* x, const float* x0_cond, const float* x0_uncond, const float* scale,
                          const uint8_t* inpaint_mask, const float* inpaint_motion, int32_t clip_denoised, float* out,
                          float* pred_out, float* eps_out, void* stream);

/* q_sample (gaussian_diffusion.py:233-251): out = a*x_start + b*noise, a/b per-sample from
 * coef rows (c[5], c[6]) at idx. */
int gdx_q_sample(const float* x_start, const float* noise, const float* coef, int32_t idx,
                 int64_t count, float* out, void* stream);

/* q_sample with per-sample timesteps t [B] (int64, device): the form training_losses uses (:1249). */
int gdx_q_sample_t(const float* x_start, const float* noise, const float* coef, const int64_t* t, int32_t batch,
                   int64_t per_sample, float* out, void* stream);
/* masked_l2 (gaussian_diffusion.py:201-213): out[b] = sum_{j,t} (a-b)^2 mask[b,t] / (J * sum_t mask[b,t]);
 * a, b [B,J,1,T] fp32, mask bool bytes [B,1,1,T], out [B].  Used by the forward half of training_losses (:1227-1352). */
int gdx_masked_l2(const float* a, const float* b, const uint8_t* mask, float* out, int32_t batch, int32_t njoints,
                  int32_t frames, void* stream);

/* Philox N(0,1) fill, same keying as gdx_sampler_update (rng_step) -- used for x_T. */
int gdx_randn(float* out, int32_t batch, int64_t per_sample, uint64_t philox_seed,
              uint64_t sample_offset, uint32_t rng_step, void* stream);

/* ---- chunk post-processing ----------------------------------------------- */
/* replaces the CPU tail of the reference's chunk loop (sample/generate.py:132-146): inv_transform
 * (data * std + mean with the dataset's fp64 statistics, data_loaders/gesture/data/dataset.py:118-119, rounded to
 * fp32 once) and the split of the 6-per-joint feature vector into positions (6j+3..5) and rotations (6j..2).
 * x [B, 6*n_joints, 1, T] fp32, mean / std [6*n_joints] fp64 (device), pos / rot [B, n_joints, 3, T] fp32. */
int gdx_postprocess(const float* x, const double* mean, const double* std, float* pos, float* rot,
                    int32_t batch, int32_t n_joints, int32_t frames, void* stream);

/* ---- conditioning features ---------------------------------------------- */
/* MFCC vectors of one audio chunk, replacing the CPU call at data_loaders/gesture/data/dataset.py:81-95
 * (python_speech_features.mfcc(signal, winlen=0.06, winstep=1/fps, samplerate=sr, numcep=27, nfft=5000) and the z-score):
 * pre-emphasis + rectangular framing, power spectrum by a DFT-as-GEMM on the fp32 MFMA kernel, mel filterbank (GEMM),
 * log, DCT-II (ortho), sinusoidal lifter, log frame energy in coefficient 0, (m - mean) / std.
 * signal [n] fp32 (device); tables and workspace ((numframes + GDX_ROW_PAD) rows per stage) as laid out at the definition (csrc/mfcc.hip); mean / std [numcep] or
 * NULL; out [numframes][numcep] fp32.  The package is absent from this image: parity with it is UNPINNED
 * (oracle/mfcc.py restates its published algorithm). */
int gdx_mfcc(const float* signal, int64_t n, int32_t frame_len, int32_t frame_step, int32_t numframes,
             int32_t nfft, int32_t nfilt, int32_t numcep, float preemph, const float* dft, const float* mel,
             const float* dct, const float* lifter, const float* mean, const float* std, float* work,
             float* out, void* stream);

/* ---- whole loop ------------------------------------------------------------------------ */
/* replaces p_sample_loop / ddim_sample_loop (gaussian_diffusion.py:598-661, 879-926) in the
 * configured mode (START_X, FIXED_SMALL, clip_denoised=False): iterates index = first_index
 * .. 0, model timestep = timestep_map[index] (respace.py:124-129), all work enqueued on
 * `stream` with no host synchronisation. */
typedef struct {
    int32_t kind;              /* GDX_SAMPLER_* */
    int32_t mode;              /* GDX_COND / GDX_UNCOND / GDX_CFG */
    int32_t num_steps;         /* rows of coef / timestep_map */
    int32_t first_index;       /* num_steps - 1 - skip_timesteps */
    const float* coef;         /* device [num_steps][8] */
    const int64_t* timestep_map;   /* HOST [num_steps] */
    float* x;                  /* in: x_T (or q_sample'd init), out: final sample */
    const float* scale;        /* [B] for GDX_CFG */
    const uint8_t* inpaint_mask;
    const float* inpaint_motion;
    const float* noise_tape;   /* NULL -> Philox; else [first_index+1][B,J,1,T], k-th executed step
                                  ([first_index+1][1,J,1,T] when const_noise) */
    int32_t const_noise;
    uint64_t philox_seed;
    uint64_t sample_offset;
    float* dump;               /* NULL or [n_dump][B,J,1,T] */
    const int32_t* dump_steps; /* HOST, ascending executed-step numbers (counted from the start of the whole loop) */
    int32_t n_dump;
    /* Running a loop in blocks (the caller draws the noise of one block at a time from torch's generator, the
     * reference's RNG: gaussian_diffusion.py:532,694; or reports progress per block): this call executes `run_steps`
     * steps starting at index first_index (0 = all the way down to index 0), and the first of them is executed-step
     * number `k_base` of the whole loop (Philox draw number k_base + 1; dump_steps compare against it).  noise_tape
     * always starts at THIS call's first step. */
    int32_t run_steps;
    int32_t k_base;
    int32_t clip_denoised;     /* clamp x0 to [-1, 1] each step, as in the update arguments; the callers of the reference pass False */
} gdx_loop_args_t;
int gdx_sample_loop(gdx_handle_t h, const gdx_loop_args_t* a, void* stream);

/* Resampling (RePaint, Lugmayr et al. 2022, arXiv:2201.09865, section 4.2; no counterpart in the reference): after the chain has
 * come down `jump` steps it is diffused forward `jump` steps again and comes down again, `repeats` times in all, so that the
 * generated part of an inpainted sample catches up with the known part.  repeats = 1 (the state after gdx_create) is the
 * behaviour without the feature: nothing new is launched and every result keeps its bits; alpha_bar may then be NULL.  One
 * rule everywhere (csrc/gdx_resample_plan.h; GaussianDiffusion.resample_plan / resample_coef restate it):
 *   Levels.  Level L is the input of the reverse step at schedule index L - 1, level 0 is the sample; a loop starts at level
 *     N = first_index + 1.
 *   Jump levels.  l in {0, jump, 2 jump, ...} with l + jump < N (RePaint's range(0, t_T - jump, jump), level 0 included); each has
 *     repeats - 1 jumps left.
 *   Walk.  A reverse hop takes level l + 1 -> l.  On arriving at a jump level with jumps left: use one up, take a forward hop
 *     l -> l + jump, go on descending.  N = 6, jump = 2, repeats = 2: r5 r4 r3 r2 f(2->4) r3 r2 r1 r0 f(0->2) r1 r0.
 *     Denoiser calls = N + n_levels * (repeats - 1) * jump; hops = calls + n_levels * (repeats - 1).
 *   Forward hop from -> to.  x <- a x + b z with a = sqrt(r), b = sqrt(1 - r), r = abar[to] / abar[from], abar = [1, alpha_bar ...] by
 *     level; a and b are computed in fp64 and rounded to fp32 once; product and sum are rounded separately; the whole tensor,
 *     an inpainted region included.  One hop of `jump` levels in place of RePaint's `jump` single steps: the same distribution,
 *     one launch, one draw.  Its bits are those of gdx_randn followed by gdx_q_sample on a row with (c[5], c[6]) = (a, b).
 *   Draws.  Executed hops of both kinds are numbered k = 0, 1, ... in one sequence: hop k takes Philox draw k + 1 (x_T is draw
 *     0), or slice k of a noise tape.
 * gdx_set_resample builds the (a, b) row of every forward hop from alpha_bar (HOST, [num_steps], the loop's own -- respaced --
 * schedule: in (0, 1], not increasing); the library owns the device table and uploads it on the stream of the next loop.
 * With repeats > 1, gdx_sample_loop (GDX_SAMPLER_P and GDX_SAMPLER_DDIM) executes the walk: a reverse hop is the denoiser call and
 * the gdx_sampler_update of the plain loop, unchanged; a forward hop is one launch.  first_index is then the WHOLE loop's first
 * index in every block, k_base / run_steps count executed hops of both kinds, and noise_tape starts at the block's first hop,
 * one [B,J,1,T] slice per hop.  The loop takes the pose-layout eager path: there is no token-major variant and no graph
 * capture.  Every reverse hop takes the mode of its own model timestep, so the guidance interval, the rescale and the 3-pass
 * compose apply as they are.  Refused, before the first launch: dump_steps, const_noise, gdx_set_guidance_refresh and
 * gdx_set_layer_cache with every > 1 (a forward hop invalidates what they carry), and a num_steps other than the setter's.
 * gdx_plms_loop, gdx_dpm_loop, gdx_dpm_sde_loop, gdx_unipc_loop, gdx_ddim_reverse_loop, gdx_parallel_loop and gdx_bpd_loop refuse
 * while repeats > 1: their history does not survive a jump.  Nothing is claimed about motion quality on a trained checkpoint
 * (DESIGN.md 4p holds the analytic case).
 * gdx_set_resample makes no HIP call; a null handle, jump < 1, repeats < 1 and, with repeats > 1, a NULL or ill-formed alpha_bar
 * are refused. */
int gdx_set_resample(gdx_handle_t h, int32_t jump, int32_t repeats, const double* alpha_bar, int32_t num_steps);

/* ---- variational bound (evaluation) ----------------------------------------------------- */
/* One term of the variational bound in bits/dim plus the two per-step error curves, fused over [B,J,1,T]: replaces
 * _vb_terms_bpd (gaussian_diffusion.py:1192-1225) with its helpers normal_kl / discretized_gaussian_log_likelihood
 * (diffusion/losses.py:12-77), the body of calc_bpd_loop's step (:1576-1578) and _prior_bpd (:1519-1535).
 * Per element, coefficient row c = coef[idx] = (posterior_mean_coef1, posterior_mean_coef2, posterior_log_variance_clipped,
 * model log-variance, sqrt_recip_alphas_cumprod, sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod,
 * sqrt_recipm1_alphas_cumprod), idx = t[b] if t != NULL else step_index:
 *   pred    = x0_cond -> CFG blend -> inpainting blend -> clamp, exactly as in the sampler update
 *   m_true  = c0*x_start + c1*x_t;   m_model = model_mean if given else c0*pred + c1*x_t
 *   kl      = 0.5*(-1 + c3 - c2 + exp(c2 - c3) + (m_true - m_model)^2 * exp(-c3))
 *   nll     = -log of the discretised Gaussian(m_model, exp(0.5*c3)) at x_start (tanh cdf, +-1/255 bin, 1e-12 clamps)
 *   vb[b]         = mean(idx == 0 ? nll : kl) / ln 2
 *   xstart_mse[b] = mean((pred - x_start)^2);   mse[b] = mean(((c4*x_t - pred)/c7 - noise)^2)
 * each written at [b*ld + col] (an output may be NULL).  prior != 0 selects the prior term instead:
 *   vb[b] = mean(0.5*(-1 - prior_log_variance + exp(prior_log_variance) + (c5*x_start)^2)) / ln 2
 * and needs only coef, x_start, vb and workspace.  All arithmetic is fp32 with separately rounded products / sums and
 * accurate exp / log / tanh.  A sample's numbers are sums in a fixed order (thread, wave, block, then the
 * ceil(J*T / GDX_BPD_CHUNK) blocks of the sample in sequence through `workspace`): no atomics, so they do not depend on the
 * batch the sample sits in.  workspace: device, 4 * batch * ceil(J*T / GDX_BPD_CHUNK) floats, the caller's. */
#define GDX_BPD_CHUNK 4096
typedef struct {
    int32_t batch, njoints, frames;
    int32_t step_index;        /* used when t == NULL */
    const float* coef;         /* [num_steps][8], rows as above */
    const int64_t* t;          /* [B] or NULL */
    const float* x_start;
    const float* x_t;
    const float* noise;        /* the z of x_t = c5*x_start + c6*z; NULL only when mse == NULL */
    const float* x0_cond;      /* START_X model output (cond pass), or an already formed pred_xstart */
    const float* x0_uncond;    /* NULL or uncond pass */
    const float* scale;        /* [B] when x0_uncond != NULL */
    const uint8_t* inpaint_mask;   /* NULL or bool bytes [B,J,1,T] */
    const float* inpaint_motion;
    const float* model_mean;   /* NULL, or the model's posterior mean when it is not c0*pred + c1*x_t (PREVIOUS_X: the raw
                                  output, with x0_cond = the x0 prediction formed by gdx_plms_update kind 8) */
    int32_t clip_denoised;
    int32_t prior;
    float prior_log_variance;  /* log_one_minus_alphas_cumprod[num_steps - 1] rounded to fp32 */
    float* vb;
    float* xstart_mse;
    float* mse;
    int32_t ld, col;
    float* pred_xstart;        /* NULL or [B,J,1,T]: pred */
    float* workspace;
} gdx_bpd_args_t;
int gdx_bpd_terms(const gdx_bpd_args_t* a, void* stream);

/* replaces calc_bpd_loop (gaussian_diffusion.py:1537-1592) for a START_X denoiser with fixed variance: for executed step
 * k = k_base .. (index i = num_steps - 1 - k) it forms x_t = sqrt_alphas_cumprod[i]*x_start + sqrt_one_minus_alphas_cumprod[i]*z_k
 * (q_sample, :233-251), runs the denoiser at timestep_map[i] and the fused terms above, all enqueued on `stream` with no
 * host synchronisation.  z_k is slice k - k_base of noise_tape ([steps of this call][B,J,1,T]) or, when noise_tape == NULL,
 * Philox N(0,1) keyed by (philox_seed; sample_offset + b; draw k; element).  vb / xstart_mse / mse: device [B][num_steps],
 * column k holds timestep num_steps - 1 - k (the reference appends in descending t).  run_steps > 0 executes only that many
 * steps (block-wise issue); 0 = down to index 0.  prior_bpd (NULL or device [B]) receives the prior term.  Graph replay does
 * not apply to this loop.  Refusals come before the first HIP call. */
typedef struct {
    int32_t mode;              /* GDX_COND / GDX_UNCOND / GDX_CFG */
    int32_t num_steps;
    const float* coef;         /* device [num_steps][8], rows of the terms above */
    const int64_t* timestep_map;   /* HOST [num_steps] */
    const float* x_start;
    const float* scale;        /* [B] for GDX_CFG */
    const uint8_t* inpaint_mask;
    const float* inpaint_motion;
    const float* noise_tape;   /* NULL -> Philox */
    uint64_t philox_seed;
    uint64_t sample_offset;
    int32_t clip_denoised;
    int32_t run_steps;
    int32_t k_base;
    float prior_log_variance;
    float* vb;
    float* xstart_mse;
    float* mse;
    float* prior_bpd;
} gdx_bpd_loop_args_t;
int gdx_bpd_loop(gdx_handle_t h, const gdx_bpd_loop_args_t* a, void* stream);

/* replaces plms_sample_loop (gaussian_diffusion.py:1081-1190 around plms_sample :995-1079) for a START_X denoiser without
 * cond_fn / denoised_fn: per executed step one denoiser call through the same forward entry gdx_forward uses (so the loop has
 * the bits of the step-wise protocol) and ONE gdx_plms_step launch, all enqueued on `stream` with no host synchronisation.
 * Executed step k runs index first_index - (k - k_base), model timestep = timestep_map[index]; its eps goes to slot k % order
 * of eps_hist and its kind is min(order, k + 1).  Step 0 of the whole loop (k_base == 0) is the pseudo improved Euler step:
 * forward at index i, kind 6 (eps -> slot 0, predictor -> scratch, pred -> slot 1, free until step 1), forward on the
 * predictor at index (i - 1) mod num_steps (the reference's table gather wraps at i == 0), kind 5 into x; the history keeps
 * the first eps.  run_steps > 0 executes only that many steps of the loop (block-wise issue, same bits as one call: the
 * history lives in the caller's eps_hist between calls, first_index is THIS call's first index and k_base the executed-step
 * number of its first step); 0 = down to index 0.  eps_hist and scratch are the caller's; the library owns only its weights
 * and workspace.  There is neither graph replay nor a token-major variant of this loop.  Refusals come before the first HIP
 * call. */
typedef struct {
    int32_t mode;              /* GDX_COND / GDX_UNCOND / GDX_CFG */
    int32_t order;             /* 2..4 */
    int32_t num_steps;         /* rows of coef / timestep_map */
    int32_t first_index;       /* index of this call's first step (whole loop: num_steps - 1 - skip_timesteps) */
    const float* coef;         /* device [num_steps][8], DDIM rows at eta = 0 */
    const int64_t* timestep_map;   /* HOST [num_steps] */
    float* x;                  /* in: x_T (or q_sample'd init), out: the sample */
    const float* scale;        /* [B] for GDX_CFG */
    const uint8_t* inpaint_mask;
    const float* inpaint_motion;
    int32_t clip_denoised;
    int32_t run_steps;
    int32_t k_base;
    float* eps_hist;           /* device [order][B,J,1,T] */
    float* scratch;            /* device [B,J,1,T]: the predictor of step 0 */
} gdx_plms_loop_args_t;
int gdx_plms_loop(gdx_handle_t h, const gdx_plms_loop_args_t* a, void* stream);

/* DPM-Solver++ multistep sampling loop (dpm_solver_sample_loop; the update, the coefficient rows and their source are at
 * gdx_dpm_step) for a START_X denoiser without cond_fn / denoised_fn: per executed step one denoiser call through the same
 * forward entry gdx_forward uses (so the loop has the bits of the step-wise protocol) and ONE gdx_dpm_step launch, all enqueued
 * on `stream` with no host synchronisation.  Executed step k runs index i = first_index - (k - k_base), model timestep =
 * timestep_map[i], at order min(order, k + 1, i + 1): a warm-up at the start and a lower order at the end, the step to sigma = 0
 * (index 0) always first order, x' = m0.  Its prediction goes to slot k % order of hist.  run_steps > 0 executes only that many
 * steps of the loop (block-wise issue, same bits as one call: the history lives in the caller's hist between calls,
 * first_index is THIS call's first index and k_base the executed-step number of its first step); 0 = down to index 0.  hist is
 * the caller's; the library owns only its weights and workspace.  There is neither graph replay nor a token-major variant of
 * this loop.  Argument checks come first, then the null handle, then readiness: every refusal precedes the first HIP call. */
typedef struct {
    int32_t mode;              /* GDX_COND / GDX_UNCOND / GDX_CFG */
    int32_t order;             /* 1..3 */
    int32_t num_steps;         /* rows of coef / timestep_map */
    int32_t first_index;       /* index of this call's first step (whole loop: num_steps - 1 - skip_timesteps) */
    const float* coef;         /* device [num_steps][8], rows of gdx_dpm_step */
    const int64_t* timestep_map;   /* HOST [num_steps] */
    float* x;                  /* in: x_T (or q_sample'd init), out: the sample */
    const float* scale;        /* [B] for GDX_CFG */
    const uint8_t* inpaint_mask;
    const float* inpaint_motion;
    int32_t clip_denoised;
    int32_t run_steps;
    int32_t k_base;
    float* hist;               /* device [order][B,J,1,T]; required when order > 1 */
} gdx_dpm_loop_args_t;
int gdx_dpm_loop(gdx_handle_t h, const gdx_dpm_loop_args_t* a, void* stream);

/* SDE-DPM-Solver++ multistep sampling loop (dpm_solver_sde_sample_loop; the update and its rows are at gdx_dpm_sde_step): the
 * loop of gdx_dpm_loop -- same step numbering, order rule min(order, k + 1, i + 1), history slots, run_steps / k_base block-wise
 * issue and order of refusals -- with ONE gdx_dpm_sde_step launch per executed step.  Executed step k takes its noise from
 * slice k - k_base of noise_tape, or, without a tape, from Philox draw k + 1 (x_T is draw 0: the convention of
 * gdx_sample_loop).  Block-wise issue gives the bits of one call.  There is neither graph replay nor a token-major variant. */
typedef struct {
    int32_t mode;              /* GDX_COND / GDX_UNCOND / GDX_CFG */
    int32_t order;             /* 1..2 */
    int32_t num_steps;         /* rows of coef / timestep_map */
    int32_t first_index;       /* index of this call's first step */
    const float* coef;         /* device [num_steps][8], rows of gdx_dpm_sde_step */
    const int64_t* timestep_map;   /* HOST [num_steps] */
    float* x;                  /* in: x_T (or q_sample'd init), out: the sample */
    const float* scale;        /* [B] for GDX_CFG */
    const uint8_t* inpaint_mask;
    const float* inpaint_motion;
    int32_t clip_denoised;
    int32_t run_steps;
    int32_t k_base;
    float* hist;               /* device [order][B,J,1,T]; required when order > 1 */
    const float* noise_tape;   /* NULL -> Philox; else device [steps of THIS call][B,J,1,T], slice 0 = this call's first step */
    uint64_t philox_seed;
    uint64_t sample_offset;
} gdx_dpm_sde_loop_args_t;
int gdx_dpm_sde_loop(gdx_handle_t h, const gdx_dpm_sde_loop_args_t* a, void* stream);

/* UniPC sampling loop (unipc_sample_loop; the update, the coefficient rows and their source are at gdx_unipc_step): the loop of
 * gdx_dpm_loop -- same step numbering, run_steps / k_base block-wise issue, order of refusals and guided calls (guidance
 * interval, rescale and refresh: one guided call per step) -- with ONE gdx_unipc_step launch per executed step.  x is always the
 * denoiser's input: x_T (or the q_sample'd init) on entry, the sample (m_0) on completion.  Executed step k at index i:
 *   1. the denoiser runs on x and gives m_i, which goes to slot k % (order + 1) of hist;
 *   2. corrector: order qc = 0 when k == 0 or i == 0 (nothing to correct / its result would not be used), else min(order, k), with
 *      base index i + 1, the base state in `base`, m_new = m_i and the history m_{i+1}, ...;  the corrected state (qc = 0: x
 *      itself) is written to `base`;
 *   3. predictor from the corrected state: order qp = min(order, k + 1, i + 1), base i, history m_i, m_{i+1}, ...;
 *   4. its output is written to x, the next denoiser input.  The step at index 0 is first order: x = m_0.
 * The ring of predictions holds order + 1 buffers: the corrector reads up to `order` older predictions, and the new one must not
 * overwrite any of them.  Block-wise issue gives the bits of one call: hist and base carry the state between calls.  hist and
 * base are the caller's; the library owns only its weights and workspace.  There is neither graph replay nor a token-major variant
 * of this loop.  Argument checks come first, then the null handle, then readiness: every refusal precedes the first HIP call. */
typedef struct {
    int32_t mode;              /* GDX_COND / GDX_UNCOND / GDX_CFG */
    int32_t order;             /* 1..3 */
    int32_t num_steps;         /* rows of coef / coef_c / timestep_map */
    int32_t first_index;       /* index of this call's first step (whole loop: num_steps - 1 - skip_timesteps) */
    const float* coef;         /* device [num_steps][8], predictor rows of gdx_unipc_step */
    const int64_t* timestep_map;   /* HOST [num_steps] */
    float* x;                  /* in: x_T (or q_sample'd init), out: the sample */
    const float* scale;        /* [B] for GDX_CFG */
    const uint8_t* inpaint_mask;
    const float* inpaint_motion;
    int32_t clip_denoised;
    int32_t run_steps;
    int32_t k_base;
    float* hist;               /* device [order + 1][B,J,1,T] */
    float* base;               /* device [B,J,1,T]: the corrected state between steps */
    const float* coef_c;       /* device [num_steps][16], corrector rows of gdx_unipc_step */
} gdx_unipc_loop_args_t;
int gdx_unipc_loop(gdx_handle_t h, const gdx_unipc_loop_args_t* a, void* stream);

/* DDIM inversion loop (ddim_reverse_sample_loop; the update and its rows are at gdx_ddim_reverse_step) for a START_X denoiser
 * without denoised_fn: the one loop that runs its indices ASCENDING.  It executes idx = first_index, first_index + 1, ...,
 * first_index + run_steps - 1: per step one denoiser call on x at model timestep timestep_map[idx], through the same forward
 * entry gdx_forward uses (so the loop has the bits of the step-wise protocol), and ONE gdx_ddim_reverse_step launch in place,
 * all enqueued on `stream` with no host synchronisation.  x holds the state at index first_index on entry (a whole inversion:
 * first_index = 0, the data itself, read as the state at abar_0 like the reference's method) and the state at index
 * first_index + run_steps on return; a loop issued in blocks gives the bits of one call, and carries nothing but x between calls.
 * The guidance interval and the guidance rescale apply per step as in every other loop (an unguided step of a GDX_CFG loop runs B
 * samples).  The guidance refresh does not: its numbering of guided calls is defined for descending loops, so a handle with
 * gdx_set_guidance_refresh's every > 1 is refused.  There is neither graph replay nor a token-major variant of this loop.
 * Argument checks come first, then the null handle, then readiness: every refusal precedes the first HIP call.
 *   mode                     GDX_COND / GDX_UNCOND / GDX_CFG
 *   num_steps                rows of coef / timestep_map
 *   first_index, run_steps   index of the first step this call executes (0 for a whole inversion); run_steps >= 1,
 *                            first_index + run_steps <= num_steps
 *   coef                     device [num_steps][8], reverse rows of gdx_ddim_reverse_step
 *   timestep_map             HOST [num_steps]
 *   x                        in: the state at first_index, out: the state at first_index + run_steps
 *   scale                    [B] for GDX_CFG
 *   inpaint_mask, inpaint_motion, clip_denoised   as in the other loops */
int gdx_ddim_reverse_loop(gdx_handle_t h, int32_t mode, int32_t num_steps, int32_t first_index, int32_t run_steps,
                          const float* coef, const int64_t* timestep_map, float* x, const float* scale,
                          const uint8_t* inpaint_mask, const float* inpaint_motion, int32_t clip_denoised, void* stream);

/* ---- parallel-in-time sampling ----------------------------------------------------------- */
/* ParaDiGMS (Shih et al. 2023, arXiv:2305.16317) over the ancestral and the DDIM step: a window of W consecutive states is
 * evaluated by ONE batched denoiser call, the known update chain is re-run over the window with those W predictions held fixed,
 * and the window advances past every state that has stopped changing.  It shortens the chain of denoiser calls that must run
 * one after the other at the price of more total denoiser work.
 *
 * The rule.  A loop executes steps k = 0 .. K-1 (K = first_index + 1) at indices i_k = first_index - k; s_k is the state after
 * k steps, s_0 the start state.  The sequential step is s_{k+1} = step_k(s_k, m_k): m_k = the denoiser's x0 prediction on s_k at
 * timestep_map[i_k]; step_k = gdx_sampler_update's formula at row i_k (x0 -> inpainting -> clamp, then the P or DDIM update);
 * its noise z_k = Philox draw k + 1 keyed by (philox_seed; sample_offset + b; element) or slice k of a tape: gdx_sample_loop's
 * convention.  The window state is an anchor a (steps finished) and planes P_0 .. P_W, each [B,J,1,T]: P_0 = s_a, P_j the current
 * guess of s_{a+j}; initially a = 0 and every plane is a copy of the start state.  One iteration, n = min(W, K - a):
 *   1. one denoiser call on P_0 .. P_{W-1} as a batch of W*B samples (2*W*B under GDX_CFG), row j*B + b, slot j at
 *      timestep_map[i_{a+j}] (slots j >= n run at index 0 and are never read), through gdx_forward: blended predictions M_0 .. M_{n-1};
 *   2. one gdx_window_sweep: per element v = P_0; for j = 0 .. n-1: v' = step_{a+j}(v, M_j), the error sum of (j, b) takes
 *      ((double)v' - (double)P_{j+1})^2, P_{j+1} = v', v = v'; err[j][b] = that sum / (J*T) in fp64;
 *   3. the stride: E_j = max_b err[j][b] (a NaN never passes); s = 1 + the number of LEADING j = 0, 1, ... with
 *      E_j <= threshold[i_{a+j}], capped at n.  Plane 1 is always final; plane j + 1 is accepted when planes 1 .. j did not move
 *      by more than their thresholds;
 *   4. the slide: a += s, P_j <- P_{j+s}, the planes that fall off the end become copies of the old P_W.  Done when a = K; the
 *      sample is P_0.
 * threshold[i] = tau^2 * exp(posterior_log_variance_clipped[i]) is the caller's (fp64).  What follows: tau = 0 accepts a plane only
 * when it did not change, so the fp32 result has the bits of the sequential loop under the same noise; W = 1 is the sequential
 * loop for any tau; tau -> infinity strides n every time, ceil(K / W) iterations; every iteration strides at least 1, so the loop
 * ends after at most K iterations, NaNs included; and for tau > 0 the maximum over b couples the samples: a sample's result
 * depends on the batch it runs in (on the shard under multi-GPU), at tau = 0 it does not.
 *
 * gdx_window_sweep: step 2 alone, stateless, plain arguments like gdx_ddim_reverse_step.
 *   kind                     GDX_SAMPLER_P / GDX_SAMPLER_DDIM
 *   batch, njoints, frames   the shape [B,J,1,T] of one plane
 *   n_slots                  n, 1 .. 64
 *   coef                     device [num_steps][8], rows of gdx_sampler_update
 *   first_index              the schedule index of slot 0; slot j runs at first_index - j (>= 0)
 *   planes                   [n_slots + 1][B,J,1,T], updated in place; plane 0 is only read
 *   x0                       [n_slots][B,J,1,T]: M_j
 *   inpaint_mask, inpaint_motion   NULL or [B,J,1,T], indexed by b, not by slot
 *   clip_denoised
 *   noise                    NULL -> Philox; else [n_slots][B,J,1,T], slice 0 is slot 0's
 *   philox_seed, sample_offset, rng_step   rng_step = the Philox draw of slot 0; slot j draws rng_step + j
 *   err                      device double [n_slots][B]
 *   workspace                device double [n_slots * B * ceil(J*T / GDX_BPD_CHUNK)]
 * The planes have the bits of n successive gdx_sampler_update launches on the same operands (one definition of each formula).
 * A thread owns one 4-element group and walks the slots with the state in registers; 128-bit accesses when J*T % 4 == 0 and
 * every pointer is 16-byte aligned (the mask 4-byte), a scalar path otherwise; nothing is written in front of plane 1 or behind
 * plane n.  The error sums are accumulated in a fixed order without atomics: per-chunk partials of GDX_BPD_CHUNK elements (one
 * block each) in `workspace`, added in chunk order by a second, tiny launch.  Streaming: 2n planes read, n written.  batch <= 65535.
 * Refusals come before the first HIP call. */
int gdx_window_sweep(int32_t kind, int32_t batch, int32_t njoints, int32_t frames, int32_t n_slots, const float* coef,
                     int32_t first_index, float* planes, const float* x0, const uint8_t* inpaint_mask, const float* inpaint_motion,
                     int32_t clip_denoised, const float* noise, uint64_t philox_seed, uint64_t sample_offset, uint32_t rng_step,
                     double* err, double* workspace, void* stream);

/* The loop of the rule above.  The handle is prepared for window * B samples and conditioned on seed / mfcc (and text) repeated
 * window-major (row j*B + b = sample b); B = the prepared batch / window.  THE ONE LOOP THAT SYNCHRONISES `stream`: once per
 * iteration, to read the n error rows the stride depends on.  Issued in blocks (max_iterations) it carries nothing between calls
 * but the planes and *anchor and gives the bits of one call.  The guidance interval and the guidance rescale apply per sample as in
 * gdx_forward (a partly guided window keeps the double batch).  Refused, before the first launch: a handle whose guidance refresh
 * or layer cache has every > 1 (both need memory across SEQUENTIAL calls); window outside 1 .. 64; a prepared batch the window
 * does not divide; window * B * (2 under GDX_CFG) > 65535.  Neither graph replay nor the token-major path applies.
 * gdx_forward_samples advances by window * B * (1 or 2) per iteration, ignored tail slots included.
 *   kind, mode               GDX_SAMPLER_P / _DDIM; GDX_COND / GDX_UNCOND / GDX_CFG
 *   num_steps, first_index   rows of coef / timestep_map / threshold; the loop's first index (K = first_index + 1 steps)
 *   coef                     device [num_steps][8]
 *   timestep_map             HOST [num_steps]
 *   threshold                HOST double [num_steps]
 *   window                   W
 *   planes                   device [window + 1][B,J,1,T]; in: every plane the start state (or a block's planes), out: P_0 = the sample
 *   scale                    [B] for GDX_CFG
 *   inpaint_mask, inpaint_motion, clip_denoised   as in the other loops, [B,J,1,T]
 *   noise_tape               device [K][B,J,1,T] (slice k = executed step k of the WHOLE loop) or NULL -> Philox draw k + 1
 *   philox_seed, sample_offset
 *   anchor                   HOST, in / out: steps finished (0 at the start, K at the end)
 *   max_iterations           0 = run to the end
 *   strides_out, strides_capacity   HOST array or NULL: this call's strides, the first strides_capacity of them
 *   iterations_out           HOST: this call's iterations */
int gdx_parallel_loop(gdx_handle_t h, int32_t kind, int32_t mode, int32_t num_steps, int32_t first_index, const float* coef,
                      const int64_t* timestep_map, const double* threshold, int32_t window, float* planes, const float* scale,
                      const uint8_t* inpaint_mask, const float* inpaint_motion, int32_t clip_denoised, const float* noise_tape,
                      uint64_t philox_seed, uint64_t sample_offset, int32_t* anchor, int32_t max_iterations, int32_t* strides_out,
                      int32_t strides_capacity, int32_t* iterations_out, void* stream);

/* Replay ONE captured step as a hipGraph inside gdx_sample_loop (device-resident step state; the graph runs on an
 * internal stream ordered after / before `stream` by events).  Results are bit-identical to the eager loop.  A call whose
 * steps do not all take the same mode (a guidance interval that begins or ends inside it) runs eagerly.  Off by
 * default: on ROCm 7.2 the replay measured ~10 % slower than eager launches even for launch-dominated small batches
 * (csrc/loops.hip, gdx_sample_loop).  Ignored while taps, dump_steps or in-situ profiling are active. */
int gdx_set_graph_replay(gdx_handle_t h, int32_t on);

/* ---- measurement helpers (bench.py only) ------------------------------------------------ */
/* Time `iters` launches of the FFN-1 GEMM (bias+GELU epilogue) of layer 0 on the current
 * workspace shape with HIP events on `stream`; returns average microseconds per launch. */
int gdx_bench_ffn_gemm(gdx_handle_t h, int32_t iters, float* avg_us, void* stream);
/* In-situ timing of the FFN linear1 GEMM launches of subsequent forwards / loops: HIP events recorded on the
 * launch stream around each of the next (at most `max_launches`) launches; gdx_profile_end synchronises on them
 * and returns their average duration. */
int gdx_profile_begin(gdx_handle_t h, int32_t max_launches);
int gdx_profile_end(gdx_handle_t h, float* avg_us, int32_t* launches);
/* Time `iters` launches of a stand-alone C[M,N] = A[M,K] W[N,K]^T GEMM with epilogue `epi`
 * (0 bias, 1 bias+GELU, 2 bias+residual) on scratch buffers filled with N(0,1). */
int gdx_bench_gemm(int32_t M, int32_t N, int32_t K, int32_t epi, int32_t iters, float* avg_us, void* stream);
/* Time `iters` launches of the self-attention core on scratch qkv [B*S][3d] (version 1 = attention.hip,
 * 3 = the fp16 kernel attentionh.hip, 4 = attention3.hip where supported). */
int gdx_bench_attention(int32_t B, int32_t S, int32_t H, int32_t d, int32_t version, int32_t iters,
                        float* avg_us, void* stream);
/* ---- reduced-precision building blocks (tests / measurement) ---------------------------- */
/* out = act(A W^T + bias) through the fp16-input / fp32-accumulate MFMA GEMM of the fp16 mode
 * (csrc/gemmh.hip): A [M][K], W [N][K], bias [N] or NULL are fp32 device arrays that the call
 * converts to fp16 (weights are packed exactly as gdx_set_weight packs them); C32 [M][N] receives
 * the fp32 epilogue output and/or C16 [M][N] the fp16-rounded output widened back to fp32 (either
 * may be NULL).  K % 64 == 0, N % 64 == 0.  Synchronises the stream (scratch is freed on return). */
int gdx_linear_f16(const float* A, const float* W, const float* bias, float* C32, float* C16,
                   int32_t M, int32_t N, int32_t K, int32_t gelu, void* stream);
/* The same GEMM with the whole epilogue the forwards use, element type `dtype` (GDX_DTYPE_F16 / _BF16, not the process-wide
 * setting):  C[row_out][n] = act(A W^T + bias[n] + R[row_out * ldr + n] + V[(m / T) * ldv + n]),  act = GELU if gelu,
 * row_out = rowmap ? m + m/T + 1 : m  (token 0 of every sample of a [B, T+1] layout skipped).  bias, R, V may each be NULL.
 * C32 (fp32, written in place) and / or C16 (the 16-bit output widened to fp32) hold c_rows >= the stored rows
 * (rowmap ? M + (M-1)/T + 1 : M) rows of N; the 16-bit output is staged from C16's own values, so rows the kernel does not
 * store come back unchanged.  (tile_mb, tile_nbw) forces a tile shape as gdx_set_test_gemmh_tile does, for this call only
 * ((0, 0) = the cost model, with its row cut).  launched (optional, 5 entries) receives what ran: the (mb, nbw) of the
 * first launch (mb = 16: the eight-wave kernel), the rows of the row cut's main part (0: no cut) and the (mb, nbw) of the
 * tail launch.  K % 64 == 0, N % 64 == 0.  Synchronises the stream. */
int gdx_linear_half(const float* A, const float* W, const float* bias, const float* R, int32_t ldr, const float* V,
                    int32_t ldv, float* C32, float* C16, int32_t c_rows, int32_t M, int32_t N, int32_t K, int32_t T,
                    int32_t rowmap, int32_t gelu, int32_t dtype, int32_t tile_mb, int32_t tile_nbw, int32_t* launched,
                    void* stream);
/* out = LayerNorm(x + res) over rows of d (eps 1e-5, biased variance; csrc/norm.hip) as the forwards launch it.
 * half_input = 0: fp32 x / res (the fp32 kernels, with a 16-bit copy out16 in element type dtype when out16 is given);
 * half_input = 1: x / res rounded to dtype (GDX_DTYPE_F16 / _BF16) by the call, the 16-bit kernels (out16 required, out32
 * optional).  res may be NULL.  compact_S > 0: rows are [B, S] tokens and token 0 of every sample is dropped from the output.
 * out32 / out16 are fp32 device arrays of out_rows >= the stored rows; out16 receives the 16-bit output widened, staged
 * from its own values like gdx_linear_half's C16.  d % 32 == 0, d <= 2048.  Synchronises the stream. */
int gdx_layernorm(const float* x, const float* res, const float* gamma, const float* beta, float* out32, float* out16,
                  int32_t out_rows, int32_t rows, int32_t d, int32_t compact_S, int32_t half_input, int32_t dtype,
                  void* stream);
/* V2 front end (RoPE -> causal local attention, window `window`, look back one window -> RoPE at t+1) through the same
 * dispatch as the forward of compute dtype `dtype`: xseq [B, T, d] fp32 (rounded to dtype by the call when the 16-bit kernel
 * runs), cos / sin [>= T+1][d / heads / 2], enc [B, T+1, d] fp32 (rows b*(T+1) stay untouched) and / or enc16 (the 16-bit
 * output widened, staged from its own values), each of enc_rows >= B*(T+1) rows.  The fp32 kernels need enc, the 16-bit one
 * enc16; GDX_DTYPE_F32 takes no enc16.  kernel (optional) receives what ran: 0 the scalar fp32 kernel, 1 the fp32 MFMA
 * kernel, 2 the 16-bit kernel.  T % window == 0.  Synchronises the stream. */
int gdx_local_attention(const float* xseq, const float* cosT, const float* sinT, float* enc, float* enc16, int32_t enc_rows,
                        int32_t B, int32_t T, int32_t d, int32_t heads, int32_t window, int32_t dtype, int32_t* kernel,
                        void* stream);
/* ---- the boundary kernels of the denoiser step (csrc/boundary.hip, csrc/boundaryh.hip; tests) -------------------- */
/* Each of the six calls below runs one launcher exactly as the forwards call it.  Inputs are fp32 device arrays read in
 * place, with the caller's strides.  Every output is an fp32 device array of a stated row capacity (at least the rows the
 * kernel stores); it is staged from the caller's own values and copied back whole, so elements the kernel does not store
 * come back unchanged (NaN stays NaN); a 16-bit output travels as fp32, rounded to dtype on the way in and widened on the
 * way out.  Every refusal (a null pointer, a non-positive size, a stride below the row it must hold, a capacity below the
 * stored rows, an unknown dtype or act) comes before the first HIP call.  Each call synchronises the stream. */
/* Pose tensor x [Bsrc, J, T] -> token-major xt[(b*T + t)*ldx + j] for b < B (source sample b % Bsrc: B = 2*Bsrc feeds both
 * halves of a CFG batch), columns J..ldx-1 zeroed.  xt [xt_rows >= B*T][ldx >= J].  dtype GDX_DTYPE_F32: the fp32 kernel;
 * GDX_DTYPE_F16 / _BF16: the 16-bit kernel of that element type, xt = its output widened.  Bsrc <= B. */
int gdx_transpose_in(const float* x, float* xt, int32_t xt_rows, int32_t B, int32_t Bsrc, int32_t J, int32_t T, int32_t ldx,
                     int32_t dtype, void* stream);
/* Token-major prediction yt[(b*T + t)*ldy + j] -> y[(b*J + j)*T + t].  yt [B*T][ldy >= J] (columns J..ldy-1 are not read),
 * y [y_rows >= B*J][T]. */
int gdx_transpose_out(const float* yt, float* y, int32_t y_rows, int32_t B, int32_t J, int32_t T, int32_t ldy, void* stream);
/* out[m*ldo + n] = act(sum_{k<K} A[m*lda + k] * W[n*ldw + k] + bias[n]) for m < M, n < N; act 0 = none, 1 = SiLU; bias may
 * be NULL.  The timestep MLP, the seed-pose encoder and the coarse slices of project_to_lat.  lda, ldw >= K; out
 * [out_rows >= M][ldo >= N]. */
int gdx_small_linear(const float* A, int32_t lda, const float* W, int32_t ldw, const float* bias, float* out, int32_t out_rows,
                     int32_t ldo, int32_t M, int32_t N, int32_t K, int32_t act, void* stream);
/* out[m][:] = table[clamp(idx[m], 0, max_rows - 1)][:] (timestep -> positional-encoding row).  table [>= max_rows][d],
 * idx [M] int64 (device), out [out_rows >= M][d]. */
int gdx_gather_rows(const float* table, const int64_t* idx, float* out, int32_t out_rows, int32_t M, int32_t d,
                    int32_t max_rows, void* stream);
/* The hoisted MFCC slice of the input linear:
 *   out[(b*rps + t + off)*d + n] = sum_{c<C} mfcc[((b % Bsrc)*C + c)*T + t] * W[n*ldw + c] + bias[n] (+ pe[(t+1)*d + n])
 * for b < B, t < T, n < d.  V1 passes rps = T + 1, off = 1 and pe; V2 rps = T, off = 0 and no pe.  mfcc [Bsrc, C, T],
 * W [d][ldw >= C], bias [d], pe [>= T+1][d] or NULL, out [out_rows >= (B-1)*rps + off + T][d].  C <= 32, rps >= T + off,
 * Bsrc <= B. */
int gdx_mfcc_project(const float* mfcc, const float* W, int32_t ldw, const float* bias, const float* pe, float* out,
                     int32_t out_rows, int32_t B, int32_t Bsrc, int32_t C, int32_t T, int32_t d, int32_t rps, int32_t off,
                     void* stream);
/* The conditioning token: enc[b*S*d + n] = temb[(b % Bsrc)*tstride + n] + seed_emb[b*d + n] (+ pe0[n]) for b < B, n < d
 * (row 0 of each sample's S rows; the others are not stored), and enc16 (optional, 16-bit modes) the same value rounded to
 * dtype.  tstride = 0: one temb row for the batch, else >= d.  c2t, c2_seed, c2 (all three or none; V2):
 * c2[b*d + n] = c2t[(b % Bsrc)*tstride + n] + c2_seed[b*d + n].  state (optional; graph replay): a device int[2]; temb and
 * c2t are then table bases and row state[0] of them is used.  enc / enc16 [enc_rows >= (B-1)*S + 1][d], c2 [c2_rows >= B][d].
 * GDX_DTYPE_F32 takes no enc16.  Bsrc <= B. */
int gdx_token0(const float* temb, int32_t tstride, const float* seed_emb, const float* pe0, float* enc, float* enc16,
               int32_t enc_rows, const float* c2t, const float* c2_seed, float* c2, int32_t c2_rows, const int32_t* state,
               int32_t B, int32_t Bsrc, int32_t S, int32_t d, int32_t dtype, void* stream);
/* ctx = softmax(Q K^T / sqrt(hd)) V per (sample, head) through the fp16 attention kernel
 * (csrc/attentionh.hip): qkv [B*S][3d] and ctx [B*S][d] are fp32 device arrays converted to / from
 * fp16 by the call.  head_dim = d / H in {32, 64, 96, 128, 192, 256}.  Synchronises the stream. */
int gdx_attention_f16(const float* qkv, float* ctx, int32_t B, int32_t S, int32_t H, int32_t d, void* stream);
/* The same attention with the element type as an argument (GDX_DTYPE_F16 / _BF16, not the process-wide setting) and a
 * forced kernel: qkv [qkv_rows][3d] fp32 (qkv_rows >= B*S), ALL of it converted to dtype; the kernel reads qkv_rows rows, as
 * the forward reads its padded workspace (rows past B*S are the caller's).  ctx [ctx_rows][d] fp32 (ctx_rows >= B*S) receives
 * the 16-bit output widened, staged from ctx's own values: rows the kernel does not store come back unchanged.
 * kernel: 0 = the forward's dispatch, 1 = attentionh8_kernel (8 waves x 1 query block), 2 = attentionh8q_kernel (8 x 2),
 * 3 = attentionh8p_kernel (persistent); 2 and 3 exist for head_dim 64 / 128 / 256 only (32, 96 and 192 are
 * refused for them; the forward's dispatch keeps those widths on kernel 1).  head_dim in {32, 64, 96, 128, 192, 256}.  grid > 0 (kernel 3 only): workgroups
 * of the persistent kernel (0 = min(work items, CUs)).  launched (optional, 3 entries) receives the kernel that ran (1-3), its
 * grid and its work-item count.  Every refusal comes before the first HIP call.  Synchronises the stream. */
int gdx_attention_half(const float* qkv, int32_t qkv_rows, float* ctx, int32_t ctx_rows, int32_t B, int32_t S, int32_t H,
                       int32_t d, int32_t dtype, int32_t kernel, int32_t grid, int32_t* launched, void* stream);
/* The fp32 self-attention kernels on the caller's own extents, with a forced kernel (test entry point, the fp32 counterpart of
 * gdx_attention_half): the kernels run on device copies of exactly qkv [qkv_rows][3d] -- no hidden pad: rows past B*S are the
 * caller's, finite by contract -- and of the whole ctx [ctx_rows][d], which is copied back whole, so rows the kernel does not
 * store come back unchanged.  kernel: 0 = the choice gdx_forward makes (attention3.hip where it takes the shape, and its own
 * choice of the persistent form), 1 = attention_kernel (attention.hip), 3 = attention3.hip item-resident, 5 = attention3.hip
 * persistent on `grid` workgroups (0 < grid < B*H; grid must be 0 for every other kernel).  3 and 5 need head_dim 64 / 128
 * and S <= 256.  Whenever attention3.hip runs, qkv_rows >= B*S + 64 (it stages whole 64-key tiles); attention.hip clamps
 * and takes qkv_rows = B*S.  launched (optional, 3 entries) receives the kernel that ran (1, 3 or 5), its grid (grid.x for
 * kernel 1) and the (sample, head) item count.  Every refusal comes before the first HIP call.  Synchronises the stream. */
int gdx_attention_f32_rows(const float* qkv, int32_t qkv_rows, float* ctx, int32_t ctx_rows, int32_t B, int32_t S, int32_t H,
                           int32_t d, int32_t kernel, int32_t grid, int32_t* launched, void* stream);
/* element type (GDX_DTYPE_F16, the default, or GDX_DTYPE_BF16) of the stand-alone entry points gdx_linear_f16,
 * gdx_attention_f16, gdx_bench_gemm_f16 and gdx_bench_attention's reduced-precision version; process-wide, tests only */
int gdx_set_test_half_dtype(int32_t dtype);
/* tile shape of the reduced-precision GEMM (csrc/gemmh.hip) for every later call of the stand-alone entry points
 * gdx_linear_f16 and gdx_bench_gemm_f16: 16 * mb rows x 64 * nbw columns (the fifteen shapes of gemmh.hip's GH_CONFIGS: four
 * MFMA + four loader waves, three slots of 64-deep K slabs), (16, 4) = the 256 x 256 eight-wave kernel with its
 * grouped tile order, (0, 0) = the cost model (with its row cut; GDX_GEMMH_TILE ignored).  It applies to those entry points
 * only, NOT to a model's forwards in the same process: the GDX_GEMMH_TILE=mb,nbw environment variable remains the way to
 * force a tile for a whole forward.  Process-wide, tests only */
int gdx_set_test_gemmh_tile(int32_t mb, int32_t nbw);
/* ctx = softmax(Q K^T / sqrt(hd)) V per (sample, head) through the fp32 attention kernels: the SDPA inside
 * nn.MultiheadAttention of the encoder layers (model/mdm.py:90-96).  qkv [B*S][3d], ctx [B*S][d] fp32 device arrays.
 * version 0 = the choice gdx_forward makes, 1 = 32x32-block kernel (attention.hip, the general fallback),
 * 3 = attention3.hip, 5 = attention3.hip's persistent variant on ceil(B*H / 3) workgroups.  Test entry point: works on
 * a padded scratch copy and synchronises the stream. */
int gdx_attention_f32(const float* qkv, float* ctx, int32_t B, int32_t S, int32_t H, int32_t d, int32_t version,
                      void* stream);
/* C = epilogue(A W^T) through the fp32 GEMM of the encoder projections (csrc/gemm2.hip; the nn.Linear calls of
 * model/mdm.py:90-96,350-356,372-380): A [M][K], W [N][K], bias [N] or NULL, R [M][N] (epi 2) fp32 device arrays, C [M][N].
 * epi 0 = + bias, 1 = gelu(. + bias), 2 = + bias + R.  K % 32 == 0.  (tile_mb, tile_nbw, tile_bk) != 0 forces that tile
 * shape of the persistent kernel (16*mb rows x 64*nbw columns, K slab bk) instead of the cost model's choice.  Test entry
 * point: works on padded scratch copies and synchronises the stream. */
int gdx_linear_f32(const float* A, const float* W, const float* bias, const float* R, float* C, int32_t M, int32_t N,
                   int32_t K, int32_t epi, int32_t tile_mb, int32_t tile_nbw, int32_t tile_bk, void* stream);
/* The same GEMM path with the whole epilogue the fp32 forwards use, through the forwards' own dispatcher:
 *   C[row_out][n] = act(A W^T + bias[n] + R[row_out * ldr + n] + V[(m / T) * ldv + n]),  act = GELU if gelu,
 *   row_out = rowmap ? m + m/T + 1 : m  (token 0 of every sample of a [B, T+1] layout skipped).
 * bias [N], R [rowmap ? M + (M-1)/T + 1 : M][ldr] and V [ceil(M / T)][ldv] may each be NULL, but only the operand sets the
 * forwards launch are taken: bias (gelu or not); R (+ bias); R with the row map (+ bias); R + V.  Any other combination is
 * refused.  C [c_rows][N], c_rows >= the stored rows, is staged from the caller's own values into a scratch with GDX_ROW_PAD
 * further rows and all c_rows rows are copied back: rows the kernel does not store come back unchanged, and whole-tile stores
 * past M (plain and residual epilogues of gemm2.hip) show up in the caller's rows past M.  The scratch copies of A and R carry
 * GDX_ROW_PAD rows of NaN behind the caller's rows.  kernel: 0 = the dispatcher's choice, 1 = csrc/gemm2.hip only (an error
 * where it does not take the problem, instead of the fallback), 2 = csrc/gemm.hip only.  (tile_mb, tile_nbw, tile_bk) as in
 * gdx_linear_f32 (kernel 0 or 1); a forced shape that is not valid for the problem is not an error: the cost model's choice
 * runs and `launched` says so.  launched (optional, 6 entries) receives what ran: the file (1 = gemm2.hip, 2 = gemm.hip) and,
 * for gemm2.hip, the tile's (mb, nbw, bk), its LDS ring depth and 1 if it was the residual-prefetch (RESP) instantiation.
 * K % 32 == 0.  Every refusal comes before the first HIP call.  Synchronises the stream. */
int gdx_linear_full(const float* A, const float* W, const float* bias, const float* R, int32_t ldr, const float* V,
                    int32_t ldv, float* C, int32_t c_rows, int32_t M, int32_t N, int32_t K, int32_t T, int32_t rowmap,
                    int32_t gelu, int32_t kernel, int32_t tile_mb, int32_t tile_nbw, int32_t tile_bk, int32_t* launched,
                    void* stream);
/* Time `iters` launches of the fp16 GEMM on scratch operands filled with N(0,1).  With GDX_GEMM_DEBUG set, one more launch
 * carries in-kernel stamps and prints them to stderr: `[gemmh8 stamps]` (eight-wave kernel, per tile) and `[gemmh stamps]`
 * (a loader wave of the 4 + 4-wave kernel that ran; its "step" is one 64-deep K slab of whole 128-byte lines). */
int gdx_bench_gemm_f16(int32_t M, int32_t N, int32_t K, int32_t gelu, int32_t iters, float* avg_us,
                       void* stream);
/* Algorithmic FLOPs of one forward at the prepared shape (SURVEY.md 8d formula). */
int gdx_forward_flops(gdx_handle_t h, int32_t mode, double* flops);

#ifdef __cplusplus
}
#endif
#endif /* GDX_H */
