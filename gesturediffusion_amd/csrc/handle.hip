// libgdx.so host side: the model handle -- the error text, the workspace and its guards and taps, the conditioning, the per-handle
// settings and counters, profiling.  C ABI in include/gdx.h; the handle's weights are in weights.hip, the per-step kernel sequence
// in forward.hip, the sampling loops in loops.hip.
#include "gdx_host.h"

#include <string>
#include <vector>

namespace gdx {

static thread_local std::string g_err;

int fail(const std::string& m) {
    g_err = m;
    return -1;
}

void clear_error() { g_err.clear(); }

}  // namespace gdx

using namespace gdx;

static constexpr size_t GUARD_BYTES = 64 * 1024;
static constexpr int GUARD_BYTE = 0xA5;

int gdx::dev_alloc(std::vector<void*>& pool, void** p, size_t bytes) {
    hipError_t e = hipMalloc(p, bytes ? bytes : 16);
    if (e != hipSuccess) return fail(std::string("hipMalloc: ") + hipGetErrorString(e));
    pool.push_back(*p);
    return 0;
}

extern "C" int gdx_set_error_(const char* msg) { return fail(msg); }

extern "C" const char* gdx_last_error(void) { return g_err.c_str(); }

extern "C" int gdx_create(const gdx_config_t* cfg, gdx_handle_t* out) {
    if (!cfg || !out) return fail("gdx_create: null argument");
    if (cfg->arch != GDX_ARCH_MDM && cfg->arch != GDX_ARCH_MDM_OLD) return fail("gdx_create: unknown arch");
    if (cfg->compute_dtype != GDX_DTYPE_F32 && cfg->compute_dtype != GDX_DTYPE_F16 && cfg->compute_dtype != GDX_DTYPE_BF16)
        return fail("gdx_create: unknown compute_dtype");
    if (cfg->compute_dtype != GDX_DTYPE_F32 && (cfg->latent_dim % 64 || cfg->ff_size % 64))
        return fail("gdx_create: the fp16 / bf16 modes need latent_dim and ff_size to be multiples of 64");
    if (cfg->latent_dim <= 0 || cfg->latent_dim % 32) return fail("gdx_create: latent_dim must be a multiple of 32");
    if (cfg->ff_size <= 0 || cfg->ff_size % 32) return fail("gdx_create: ff_size must be a multiple of 32");
    if (cfg->num_heads <= 0 || cfg->latent_dim % cfg->num_heads) return fail("gdx_create: latent_dim % num_heads != 0");
    const int hd = cfg->latent_dim / cfg->num_heads;
    if (!head_dim_supported(hd)) return fail("gdx_create: head_dim must be " GDX_HEAD_DIMS);
    if (cfg->njoints <= 0 || cfg->num_layers <= 0 || cfg->seed_poses <= 0 || cfg->mfcc_dim <= 0 || cfg->mfcc_dim > 32)
        return fail("gdx_create: bad njoints/num_layers/seed_poses/mfcc_dim");
    if (cfg->arch == GDX_ARCH_MDM) {
        if (cfg->cl_head <= 0 || cfg->latent_dim % cfg->cl_head || (cfg->latent_dim / cfg->cl_head) % 2)
            return fail("gdx_create: latent_dim / cl_head must be an even integer");
        if (cfg->window <= 0 || cfg->window > 16) return fail("gdx_create: window must be in 1..16");
    }
    // use_text (model/mdm.py:36-50): 0, 0 = no text
    if (cfg->text_dim < 0) return fail("gdx_create: text_dim must not be negative");
    if (cfg->text_dim > 0 && cfg->arch == GDX_ARCH_MDM_OLD) return fail("gdx_create: text_dim > 0 needs GDX_ARCH_MDM (MDM_Old has no text path)");
    if (cfg->text_dim >= cfg->latent_dim)
        return fail("gdx_create: text_dim must be smaller than latent_dim (the seed-pose encoder gets latent_dim - text_dim rows)");
    if (cfg->text_dim > 0 && cfg->clip_dim <= 0) return fail("gdx_create: text_dim > 0 needs clip_dim > 0");
    if (cfg->text_dim == 0 && cfg->clip_dim != 0) return fail("gdx_create: clip_dim without text_dim (0, 0 means no text)");
    hipError_t e = gemm_init();
    if (e != hipSuccess) return fail(std::string("gemm_init: ") + hipGetErrorString(e));
    gdx_model* h = new gdx_model();
    h->cfg = *cfg;
    h->f16 = cfg->compute_dtype != GDX_DTYPE_F32;
    h->bf16 = cfg->compute_dtype == GDX_DTYPE_BF16;
    // bf16 keeps 8 significant bits: rounding the residual stream to it after every sublayer and every LayerNorm is the
    // largest single error term of the mode, so its stream stays fp32
    h->stream32 = h->bf16;                                        // A/B record: profiles/r03a_bf16_stream32_ab.txt
    h->d = cfg->latent_dim; h->J = cfg->njoints; h->ff = cfg->ff_size; h->L = cfg->num_layers; h->H = cfg->num_heads;
    h->layers.resize(h->L);
    describe_weights(h);
    *out = h;
    return 0;
}

void gdx::free_pool(std::vector<void*>& pool) {
    for (void* p : pool) (void)hipFree(p);
    pool.clear();
}

extern "C" int gdx_destroy(gdx_handle_t h) {
    if (!h) return 0;
    free_pool(h->allocs);
    free_pool(h->ws_allocs);
    for (hipEvent_t e : h->prof_ev) (void)hipEventDestroy(e);
    if (h->gstream) (void)hipStreamSynchronize(h->gstream);
    if (h->gexec) (void)hipGraphExecDestroy(h->gexec);
    if (h->ggraph) (void)hipGraphDestroy(h->ggraph);
    if (h->gev_in) (void)hipEventDestroy(h->gev_in);
    if (h->gev_out) (void)hipEventDestroy(h->gev_out);
    if (h->gstream) (void)hipStreamDestroy(h->gstream);
    if (h->gstate) (void)hipFree(h->gstate);
    delete h;
    return 0;
}

int gdx::ws_alloc(gdx_model* h, void** p, size_t bytes, hipStream_t s) {
    if (dev_alloc(h->ws_allocs, p, bytes + (h->guards ? GUARD_BYTES : 0))) return -1;
    unsigned char* g = (unsigned char*)*p + bytes;
    if (h->guards) h->guard_zones.emplace_back(g, bytes);
    if (hipMemsetAsync(*p, 0, bytes, s) != hipSuccess || (h->guards && hipMemsetAsync(g, GUARD_BYTE, GUARD_BYTES, s) != hipSuccess))
        return fail("workspace: hipMemsetAsync failed");
    return 0;
}

// Results stored under another conditioning, shape or setting are not reused: the refresh's difference, the layer cache's change
static void forget_stored(gdx_model* h, bool difference = true, bool change = true) {
    if (difference) h->late.gd_valid = false;
    if (change) h->late.lc_valid = false;
}

extern "C" int gdx_prepare(gdx_handle_t h, int32_t batch, int32_t frames) {
    if (!h) return fail("gdx_prepare: null handle");
    if (batch <= 0 || frames <= 0) return fail("gdx_prepare: batch and frames must be positive");
    if (h->cfg.arch == GDX_ARCH_MDM && frames % h->cfg.window)
        return fail("gdx_prepare: sequence length must be divisible by window size for local attention");
    if (h->pe && frames + 1 > h->pe_rows) return fail("gdx_prepare: frames exceed positional table");
    if (h->cfg.arch == GDX_ARCH_MDM && h->rope_cos && frames + 1 > h->rope_rows)
        return fail("gdx_prepare: frames exceed rotary table");
    forget_stored(h);                                             // also by a prepare that keeps the shape (and the step tables)
    if (h->B == batch && h->T == frames && h->G == h->groups()) return 0;
    free_pool(h->ws_allocs);
    h->late = {};                                                 // everything that pointed into the pool
    h->guard_zones.clear(); h->taps.clear();
    // the shape is recorded only once every allocation has succeeded: after a failed hipMalloc a retry with the same
    // shape must allocate again instead of returning early on partial buffers
    h->B = 0; h->T = 0; h->S = frames + 1; h->cond_set = false;
    // + GDX_ROW_PAD rows: the persistent GEMM reads / stores whole tiles past the last logical row (gemm2.hip; its
    // tallest tile is checked against the pad at compile time)
    // B2: the samples of the largest forward, G row groups (2; 3 in a 3-pass compose mode).  The conditioning rows always have
    // room for three groups: modes 1 and 2 run two but keep the all-dropped rows in a third for GDX_UNCOND
    const size_t B2 = (size_t)h->groups() * batch, B3 = 3 * (size_t)batch, N = B2 * h->S + GDX_ROW_PAD, d = h->d;
    h->rows_alloc = (long)N;
    // zero-filled: the padding rows are read by whole-tile GEMMs / K-V tiles and must stay finite
    auto raw = [&](void** p, size_t bytes) { return ws_alloc(h, p, bytes, nullptr); };
    auto A = [&](float** p, size_t n) { return raw((void**)p, n * sizeof(float)); };
    // the sides of an activation pair this mode uses; every fp32 side is allocated before the first 16-bit one, in the order below
    // (the order of the guard zones gdx_check_guards reports)
    auto act = [&](Act& a, size_t n, bool want_f32, bool want_16) {
        return (want_f32 && A(&a.f, n)) || (want_16 && raw((void**)&a.h, n * 2));
    };
    const bool half = h->f16, f32 = !half, v2 = h->cfg.arch == GDX_ARCH_MDM;
    const bool res32 = f32 || h->stream32;                         // the residual stream is fp32 (add_norm)
    if (act(h->xa, N * d, true, false) || A(&h->addend, N * d) || A(&h->seed_cat, B3 * d) || A(&h->temb_in, B2 * d) ||
        A(&h->temb_h, B2 * d) || A(&h->temb, B2 * d) || A(&h->coa, B2 * d) || A(&h->c2, (B2 + 1) * d) ||
        A(&h->c2_seed, B3 * d) ||
        A(&h->x0, B2 * h->J * (size_t)frames))
        return -1;
    if (act(h->xb, N * d, res32, false) || act(h->qkv, N * 3 * d, f32, false) || act(h->ctx, N * d, f32, false) ||
        act(h->tmp, N * d, res32, false) || act(h->ffb, N * h->ff, f32, false))
        return -1;
    h->ldo = round_up(h->J, 64);
    const size_t NT = B2 * frames + GDX_ROW_PAD;
    const size_t ldx = round_up(h->J, half ? 64 : 32);             // row stride of xt: the K padding of the input GEMM's weight
    // xt.f in the 16-bit modes: the fp32 loop state of the token-major fast path (gdx_sample_loop)
    if (A(&h->x0t, NT * h->ldo) || act(h->xt, NT * ldx, true, false) || act(h->xc, NT * d, f32, false) ||
        act(h->xseq, NT * d, v2, false) || act(h->emb, NT * d, v2 && f32, false))
        return -1;
    if (act(h->xt, NT * ldx, false, half) || act(h->xa, N * d, false, half) || act(h->xb, N * d, false, half) ||
        act(h->qkv, N * 3 * d, false, half) || act(h->ctx, N * d, false, half) || act(h->tmp, N * d, false, half) ||
        act(h->ffb, N * h->ff, false, half) || act(h->xc, NT * d, false, half) || act(h->emb, NT * d, false, half && v2) ||
        act(h->xseq, NT * d, false, half && v2))
        return -1;
    if (h->keep_taps) {
        h->taps.resize(h->L + 2);                                 // L + 1: the output GEMM's operand (gdx_get_tap)
        for (auto& t : h->taps)
            if (A(&t, N * d)) return -1;
    }
    // gdx_prepare takes no stream: its fills are on the null stream, and nothing orders the first stores (gdx_set_condition, on the
    // caller's stream) behind that stream when the caller's is non-blocking
    HIPCHK(hipStreamSynchronize(nullptr));
    h->B = batch; h->T = frames; h->G = h->groups();
    return 0;
}

// the workspace again at the current shape, after a setting that shapes it has changed
static int reprepare(gdx_model* h) {
    const int B = h->B, T = h->T;
    if (!B) return 0;
    h->B = 0;
    return gdx_prepare(h, B, T);
}

// gdx_set_guards / gdx_set_keep_taps: the flag shapes the workspace, so a change re-prepares it at the current shape
static int set_workspace_flag(gdx_model* h, bool& flag, bool on) {
    if (flag == on) return 0;
    flag = on;
    return reprepare(h);
}

extern "C" int gdx_set_guards(gdx_handle_t h, int32_t on) {
    if (!h) return fail("gdx_set_guards: null handle");
    return set_workspace_flag(h, h->guards, on != 0);
}

extern "C" int gdx_check_guards(gdx_handle_t h, int64_t* bad_bytes, int32_t* first_bad_zone, void* stream) {
    if (!h || !bad_bytes) return fail("gdx_check_guards: null argument");
    if (!h->guards) return fail("gdx_check_guards: guards are off (gdx_set_guards)");
    if (h->guard_zones.size() != h->ws_allocs.size())            // ws_alloc alone adds to either
        return fail("gdx_check_guards: " + std::to_string(h->ws_allocs.size()) + " workspace allocations but " +
                    std::to_string(h->guard_zones.size()) + " guard zones: an allocation did not go through ws_alloc");
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    std::vector<unsigned char> host(GUARD_BYTES);
    int64_t bad = 0;
    int first = -1;
    for (size_t z = 0; z < h->guard_zones.size(); ++z) {
        HIPCHK(hipMemcpy(host.data(), h->guard_zones[z].first, GUARD_BYTES, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < GUARD_BYTES; ++i)
            if (host[i] != GUARD_BYTE) { ++bad; if (first < 0) first = (int)z; }
    }
    *bad_bytes = bad;
    if (first_bad_zone) *first_bad_zone = first;
    return 0;
}

extern "C" int gdx_set_keep_taps(gdx_handle_t h, int32_t keep) {
    if (!h) return fail("gdx_set_keep_taps: null handle");
    return set_workspace_flag(h, h->keep_taps, keep != 0);
}

extern "C" int gdx_get_tap(gdx_handle_t h, int32_t which, float* out, int64_t count, void* stream) {
    if (!h || !out) return fail("gdx_get_tap: null argument");
    if (!h->keep_taps || which < 0 || which > h->L + 1 || h->taps.empty()) return fail("gdx_get_tap: taps not kept");
    const int64_t maxc = (int64_t)h->G * h->B * h->S * h->d;
    if (count > maxc) return fail("gdx_get_tap: count too large");
    HIPCHK(hipMemcpyAsync(out, h->taps[which], count * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

// what a conditioning does once seed_cat holds its rows (2B under JOINT, else the 3B of F, M, U): the audio term of every row group
// of a forward (audio is never dropped), the seed half of the coarse slice, the flags
static int finish_condition(gdx_model* h, const float* mfcc, hipStream_t s) {
    const int B = h->B, T = h->T, S = h->S, d = h->d;
    const int GB = h->G * B, rows = (h->u_group() + 1) * B;
    // perturbed-attention guidance: group 1 = P has the conditioning rows of F (gdx_set_attention_guidance)
    if (h->pag()) HIPCHK(hipMemcpyAsync(h->seed_cat + (size_t)B * d, h->seed_cat, sizeof(float) * B * d, hipMemcpyDeviceToDevice, s));
    if (h->cfg.arch == GDX_ARCH_MDM_OLD) {
        // addend[b, t+1, :] = W_in[:, J:] mfcc[b,:,t] + b_in + pe[t+1]      (model/mdm_old.py:104-112)
        HIPCHK(launch_mfcc_project(mfcc, h->in_mfcc.w, h->in_mfcc.kpad, h->in_x.bias, h->pe, h->addend, GB, B,
                                   h->cfg.mfcc_dim, T, d, S, 1, s));
    } else {
        // audio_term[b*T+t, :] = W_proj[:, d:d+26] mfcc[b,:,t] + b_proj     (model/mdm.py:151-169)
        HIPCHK(launch_mfcc_project(mfcc, h->proj_audio.w, h->proj_audio.kpad, h->proj_pose.bias, nullptr, h->addend,
                                   GB, B, h->cfg.mfcc_dim, T, d, T, 0, s));
        // seed half of the coarse slice of project_to_lat (model/mdm.py:154-169), the rows of every group
        HIPCHK(launch_small_linear(h->seed_cat, d, h->proj_coa.w, h->proj_coa.kpad, nullptr, h->c2_seed, d, rows, d, d, 0, s));
    }
    h->cond_set = true;
    forget_stored(h);
    return 0;
}

extern "C" int gdx_set_condition(gdx_handle_t h, const float* seed, const float* mfcc, void* stream) {
    if (!h || !seed || !mfcc) return fail("gdx_set_condition: null argument");
    if (h->cfg.text_dim > 0) return fail("gdx_set_condition: this handle has text_dim > 0: call gdx_set_condition_text");
    if (gdx_weights_ready(h)) return -1;
    if (!h->B) return fail("gdx_set_condition: call gdx_prepare first");
    hipStream_t s = (hipStream_t)stream;
    const int B = h->B, d = h->d;
    // cond rows 0..B-1: Linear(flat seed); uncond rows (group u_group()): Linear(0) = bias   (model/mdm.py:125-127,242-250)
    HIPCHK(launch_small_linear(seed, h->J * h->cfg.seed_poses, h->seed.w, h->seed.kpad, h->seed.bias, h->seed_cat, d, B,
                               d, h->J * h->cfg.seed_poses, 0, s));
    for (int b = 0; b < B; ++b)
        HIPCHK(hipMemcpyAsync(h->seed_cat + (size_t)(h->u_group() * B + b) * d, h->seed.bias, sizeof(float) * d,
                              hipMemcpyDeviceToDevice, s));
    return finish_condition(h, mfcc, s);
}

extern "C" int gdx_set_condition_text(gdx_handle_t h, const float* seed, const float* mfcc, const float* text, void* stream) {
    if (!h || !seed || !mfcc || !text) return fail("gdx_set_condition_text: null argument");
    if (h->cfg.text_dim <= 0) return fail("gdx_set_condition_text: this handle has no text (text_dim = 0): call gdx_set_condition");
    if (gdx_weights_ready(h)) return -1;
    if (!h->B) return fail("gdx_set_condition_text: call gdx_prepare first");
    hipStream_t s = (hipStream_t)stream;
    const int B = h->B, d = h->d, td = h->cfg.text_dim, cd = h->cfg.clip_dim, ks = h->J * h->cfg.seed_poses;
    // row b = [embed_text(text_b) | seed_embed(seed_b)]: two Linears into one row of stride d   (model/mdm.py:118-127,154-155)
    HIPCHK(launch_small_linear(text, cd, h->text.w, h->text.kpad, h->text.bias, h->seed_cat, d, B, td, cd, 0, s));
    HIPCHK(launch_small_linear(seed, ks, h->seed.w, h->seed.kpad, h->seed.bias, h->seed_cat + td, d, B, d - td, ks, 0, s));
    // uncond rows (group 1 under JOINT, else group 2): both inputs zeroed before their Linear = [embed_text.bias | seed_embed.bias]:
    // the same launches over no input column (K = 0)
    float* un = h->seed_cat + (size_t)h->u_group() * B * d;
    HIPCHK(launch_small_linear(text, cd, h->text.w, h->text.kpad, h->text.bias, un, d, B, td, 0, 0, s));
    HIPCHK(launch_small_linear(seed, ks, h->seed.w, h->seed.kpad, h->seed.bias, un + td, d, B, d - td, 0, 0, s));
    if (h->guide_compose != GDX_GUIDE_JOINT) {
        // group 1 = M, one input dropped (gdx_set_guidance_compose): S = [embed_text.bias | seed_embed(seed)] where the text is the
        // steered condition (TEXT, SEED_TEXT), X = [embed_text(text) | seed_embed.bias] where the seed is (SEED, TEXT_SEED)
        const bool drop_text = h->guide_compose == GDX_GUIDE_TEXT || h->guide_compose == GDX_GUIDE_SEED_TEXT;
        float* mid = h->seed_cat + (size_t)B * d;
        HIPCHK(launch_small_linear(text, cd, h->text.w, h->text.kpad, h->text.bias, mid, d, B, td, drop_text ? 0 : cd, 0, s));
        HIPCHK(launch_small_linear(seed, ks, h->seed.w, h->seed.kpad, h->seed.bias, mid + td, d, B, d - td, drop_text ? ks : 0, 0, s));
    }
    return finish_condition(h, mfcc, s);
}

int gdx::check_ready(gdx_model* h, const char* who) {
    if (!h) return fail(std::string(who) + ": null handle");
    if (!h->B) return fail(std::string(who) + ": call gdx_prepare first");
    if (!h->cond_set) return fail(std::string(who) + ": call gdx_set_condition first");
    return 0;
}

int gdx::check_mode(const char* who, int mode, const float* scale) {
    if (mode < GDX_COND || mode > GDX_CFG) return fail(std::string(who) + ": bad mode");
    if (mode == GDX_CFG && !scale) return fail(std::string(who) + ": GDX_CFG needs scale");
    return 0;
}

// Guidance interval (gdx.h): the model timesteps, bounds inclusive, at which GDX_CFG means guidance.  Per-handle state like the
// conditioning; the default is every timestep.
extern "C" int gdx_set_guidance_interval(gdx_handle_t h, int64_t lo, int64_t hi) {
    if (!h) return fail("gdx_set_guidance_interval: null handle");
    h->guide_lo = lo; h->guide_hi = hi;
    return 0;
}

// Per-condition guidance (gdx.h): which passes a guided call contrasts.  Refusals precede any HIP call; the conditioning rows
// depend on the mode, so the caller conditions again, and the number of row groups shapes the workspace
extern "C" int gdx_set_guidance_compose(gdx_handle_t h, int32_t mode) {
    if (!h) return fail("gdx_set_guidance_compose: null handle");
    if (mode < GDX_GUIDE_JOINT || mode > GDX_GUIDE_TEXT_SEED) return fail("gdx_set_guidance_compose: unknown mode");
    if (mode != GDX_GUIDE_JOINT && h->cfg.text_dim == 0)
        return fail("gdx_set_guidance_compose: this handle has no text (text_dim = 0): one droppable condition, nothing to compose");
    h->guide_compose = mode;
    h->cond_set = false;
    forget_stored(h);
    return h->G == h->groups() ? 0 : reprepare(h);
}

// Perturbed-attention guidance (gdx.h): what a guided call contrasts F with, and the layers whose attention map P replaces by the
// identity.  Refusals precede any HIP call and leave the handle as it was
extern "C" int gdx_set_attention_guidance(gdx_handle_t h, int32_t kind, uint64_t layer_mask) {
    if (!h) return fail("gdx_set_attention_guidance: null handle");
    if (kind < GDX_PAG_OFF || kind > GDX_PAG_CFG) return fail("gdx_set_attention_guidance: unknown kind");
    if (kind != GDX_PAG_OFF && h->L > 64) return fail("gdx_set_attention_guidance: layer_mask names 64 layers, this handle has more");
    if (h->L < 64 && (layer_mask >> h->L))
        return fail("gdx_set_attention_guidance: layer_mask names a layer beyond num_layers = " + std::to_string(h->L));
    const int u_before = h->u_group();
    h->pag_kind = kind; h->pag_mask = layer_mask;
    if (h->u_group() != u_before) h->cond_set = false;            // the rows of U, and of P, change place
    forget_stored(h);
    return h->G == h->groups() ? 0 : reprepare(h);
}

int gdx::pag_conflict(const gdx_model* h, const char* who, int mode) {
    if (mode != GDX_CFG || h->pag_kind == GDX_PAG_OFF || h->guide_compose == GDX_GUIDE_JOINT) return 0;
    return fail(std::string(who) + ": perturbed-attention guidance (gdx_set_attention_guidance) adds a row group to a guided call, and "
                                   "four are not supported: set the compose mode to GDX_GUIDE_JOINT (gdx_set_guidance_compose)");
}

// Guidance rescale (gdx.h): per-handle phi, 0 = off.  Refusals precede any HIP call.
extern "C" int gdx_set_guidance_rescale(gdx_handle_t h, float phi) {
    if (!h) return fail("gdx_set_guidance_rescale: null handle");
    if (!(phi >= 0.0f && phi <= 1.0f)) return fail("gdx_set_guidance_rescale: phi must lie in [0, 1]");
    h->guide_phi = phi;
    return 0;
}

// Guidance refresh (gdx.h): per-handle `every`, 1 = off.  Refusals precede any HIP call.
extern "C" int gdx_set_guidance_refresh(gdx_handle_t h, int32_t every) {
    if (!h) return fail("gdx_set_guidance_refresh: null handle");
    if (every < 1) return fail("gdx_set_guidance_refresh: every must be at least 1");
    h->guide_every = every;
    forget_stored(h, true, false);
    return 0;
}

extern "C" int gdx_forward_samples(gdx_handle_t h, int64_t* samples) {
    if (!h || !samples) return fail("gdx_forward_samples: null argument");
    *samples = h->forward_samples;
    return 0;
}

// Layer cache (gdx.h): per-handle (every, keep), every = 1 = off.  Refusals precede any HIP call.
extern "C" int gdx_set_layer_cache(gdx_handle_t h, int32_t every, int32_t keep) {
    if (!h) return fail("gdx_set_layer_cache: null handle");
    if (every < 1) return fail("gdx_set_layer_cache: every must be at least 1");
    if (every > 1 && (keep < 1 || keep > h->L - 1))
        return fail("gdx_set_layer_cache: keep must lie in 1 .. num_layers - 1 = " + std::to_string(h->L - 1));
    h->lc_every = every; h->lc_keep = every > 1 ? keep : 0;
    forget_stored(h, false, true);
    return 0;
}

// Resampling (gdx.h): per-handle (jump, repeats), repeats = 1 = off, and the fp32 (a, b) row of every forward hop the schedule
// admits.  Refusals precede any HIP call, and the setter makes none: gdx_sample_loop uploads the rows on its own stream.
extern "C" int gdx_set_resample(gdx_handle_t h, int32_t jump, int32_t repeats, const double* alpha_bar, int32_t num_steps) {
    if (!h) return fail("gdx_set_resample: null handle");
    if (jump < 1) return fail("gdx_set_resample: jump must be at least 1");
    if (repeats < 1) return fail("gdx_set_resample: repeats must be at least 1");
    std::vector<float> rows;
    if (repeats > 1) {
        if (!alpha_bar || num_steps <= 0) return fail("gdx_set_resample: repeats > 1 needs alpha_bar [num_steps]");
        for (int i = 0; i < num_steps; ++i)
            if (!(alpha_bar[i] > 0.0 && alpha_bar[i] <= 1.0 && (i == 0 || alpha_bar[i] <= alpha_bar[i - 1])))
                return fail("gdx_set_resample: alpha_bar must lie in (0, 1] and must not increase");
        rows.assign(2 * (size_t)num_steps, 0.0f);
        for (int l = 0; l + jump <= num_steps; ++l) resample_coef(alpha_bar, l, l + jump, &rows[2 * l], &rows[2 * l + 1]);
    }
    h->rp_jump = jump; h->rp_repeats = repeats; h->rp_steps = repeats > 1 ? num_steps : 0;
    h->rp_rows.swap(rows);
    h->late.rp_tab_valid = false;
    return 0;
}

int gdx::refuse_resampling(const gdx_model* h, const char* who) {
    if (h->rp_repeats == 1) return 0;
    return fail(std::string(who) + ": resampling is on (gdx_set_resample, repeats > 1), and this loop's history does not survive a "
                                   "forward hop: gdx_sample_loop resamples; set repeats = 1");
}

extern "C" int gdx_forward_layer_samples(gdx_handle_t h, int64_t* n) {
    if (!h || !n) return fail("gdx_forward_layer_samples: null argument");
    *n = h->forward_layer_samples;
    return 0;
}

extern "C" int gdx_set_graph_replay(gdx_handle_t h, int32_t on) {
    if (!h) return fail("gdx_set_graph_replay: null handle");
    h->graph_replay = on != 0;
    return 0;
}

extern "C" int gdx_profile_begin(gdx_handle_t h, int32_t max_launches) {
    if (!h || max_launches <= 0) return fail("gdx_profile_begin: bad argument");
    while (h->prof_ev.size() < 2 * (size_t)max_launches) {
        hipEvent_t e;
        HIPCHK(hipEventCreate(&e));
        h->prof_ev.push_back(e);
    }
    h->prof_used = 0;
    h->prof = true;
    return 0;
}

extern "C" int gdx_profile_end(gdx_handle_t h, float* avg_us, int32_t* launches) {
    if (!h || !avg_us || !launches) return fail("gdx_profile_end: null argument");
    h->prof = false;
    double sum = 0.0;
    for (size_t i = 0; i + 1 < h->prof_used; i += 2) {
        HIPCHK(hipEventSynchronize(h->prof_ev[i + 1]));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, h->prof_ev[i], h->prof_ev[i + 1]));
        sum += ms;
    }
    *launches = (int32_t)(h->prof_used / 2);
    *avg_us = *launches ? (float)(sum * 1000.0 / *launches) : 0.f;
    return 0;
}

extern "C" int gdx_forward_flops(gdx_handle_t h, int32_t mode, double* flops) {
    if (!h || !flops) return fail("gdx_forward_flops: null argument");
    if (!h->B) return fail("gdx_forward_flops: call gdx_prepare first");
    // SURVEY.md section 8d
    const double B = (mode == GDX_CFG ? (double)h->groups() : 1.0) * h->B, T = h->T, S = h->S, d = h->d, J = h->J, ff = h->ff;
    const double N = B * S, Sp = h->cfg.seed_poses, mf = h->cfg.mfcc_dim;
    double f = 2 * B * d * d * 2 + 2 * B * J * Sp * d;
    if (h->cfg.arch == GDX_ARCH_MDM)
        f += 2 * B * T * J * d + 2 * B * T * (2 * d + mf) * d + 4 * B * T * 2 * h->cfg.window * d;
    else
        f += 2 * B * T * (J + mf) * d;
    f += h->L * (2 * N * d * 3 * d + 4 * B * S * S * d + 2 * N * d * d + 4 * N * d * ff);
    f += 2 * B * T * d * J;
    // perturbed-attention guidance: group P's rows skip QK^T, the softmax and PV in the masked layers
    if (mode == GDX_CFG && h->pag()) f -= __builtin_popcountll(h->pag_mask) * (4.0 * h->B * S * S * d);
    *flops = f;
    return 0;
}

extern "C" int gdx_bench_ffn_gemm(gdx_handle_t h, int32_t iters, float* avg_us, void* stream) {
    if (!h || !avg_us) return fail("gdx_bench_ffn_gemm: null argument");
    if (!h->B) return fail("gdx_bench_ffn_gemm: call gdx_prepare first");
    if (h->f16) return fail("gdx_bench_ffn_gemm: fp32 mode only (use gdx_bench_gemm_f16)");
    if (gdx_weights_ready(h)) return -1;
    hipStream_t s = (hipStream_t)stream;
    const int N = h->B * h->S, d = h->d;
    const Layer& ly = h->layers[0];
    GemmParams p{h->xb.f, d, ly.ff1.w, ly.ff1.kpad, ly.ff1.bias, nullptr, 0, nullptr, 0, h->ffb.f, h->ff, N, h->ff, d, h->T};
    return time_launches(1, iters, s, avg_us, [&] { return gemm(OUT_ROWS, EPI_GELU, p, s); });
}
