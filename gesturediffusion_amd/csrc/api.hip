// libgdx.so host side: handle, workspace, the per-step kernel sequence of the
// denoiser (V1 = reference model/mdm_old.py:84-122, V2 = model/mdm.py:105-224; forward_core, once for the three compute modes
// on top of linear / attend / add_norm) and the sampling
// loops (diffusion/gaussian_diffusion.py:598-730, 879-993).  C ABI in include/gdx.h; the handle's weights are in weights.hip.
#include "gdx_host.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace gdx {

static thread_local std::string g_err;

int fail(const std::string& m) {
    g_err = m;
    return -1;
}

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

// A zero-filled workspace buffer of the handle, with its canary zone behind it under gdx_set_guards (`who`: the entry that asks)
static int ws_alloc(gdx_model* h, const char* who, void** p, size_t bytes) {
    if (dev_alloc(h->ws_allocs, p, bytes + (h->guards ? GUARD_BYTES : 0))) return -1;
    if (hipMemset(*p, 0, bytes) != hipSuccess) return fail(std::string(who) + ": hipMemset failed");
    if (h->guards) {
        unsigned char* g = (unsigned char*)*p + bytes;
        if (hipMemset(g, GUARD_BYTE, GUARD_BYTES) != hipSuccess) return fail(std::string(who) + ": hipMemset failed");
        h->guard_zones.emplace_back(g, bytes);
    }
    return 0;
}

extern "C" int gdx_prepare(gdx_handle_t h, int32_t batch, int32_t frames) {
    if (!h) return fail("gdx_prepare: null handle");
    if (batch <= 0 || frames <= 0) return fail("gdx_prepare: batch and frames must be positive");
    if (h->cfg.arch == GDX_ARCH_MDM && frames % h->cfg.window)
        return fail("gdx_prepare: sequence length must be divisible by window size for local attention");
    if (h->pe && frames + 1 > h->pe_rows) return fail("gdx_prepare: frames exceed positional table");
    if (h->cfg.arch == GDX_ARCH_MDM && h->rope_cos && frames + 1 > h->rope_rows)
        return fail("gdx_prepare: frames exceed rotary table");
    h->gd_valid = false;                                          // guidance refresh: a stored difference never outlives a prepare
    h->lc_valid = false;                                          // layer cache: nor does a stored change
    if (h->B == batch && h->T == frames) return 0;
    free_pool(h->ws_allocs);
    h->guard_zones.clear();
    h->taps.clear();
    h->temb_table = nullptr; h->temb_table_rows = 0; h->tmap_dev = nullptr; h->c2t_table = nullptr; h->c2t_valid = false;
    h->tables_valid = false;
    h->bpd_xt = h->bpd_z = h->bpd_part = nullptr;
    h->rs_part = nullptr; h->rs_factor = nullptr; h->gd = nullptr; h->lc_delta = nullptr; h->lc_in = nullptr;
    // the shape is recorded only once every allocation has succeeded: after a failed hipMalloc a retry with the same
    // shape must allocate again instead of returning early on partial buffers
    h->B = 0; h->T = 0; h->S = frames + 1; h->cond_set = false;
    // + GDX_ROW_PAD rows: the persistent GEMM reads / stores whole tiles past the last logical row (gemm2.hip; its
    // tallest tile is checked against the pad at compile time)
    const size_t B2 = 2 * (size_t)batch, N = B2 * h->S + GDX_ROW_PAD, d = h->d;
    h->rows_alloc = (long)N;
    // zero-filled: the padding rows are read by whole-tile GEMMs / K-V tiles and must stay finite
    auto raw = [&](void** p, size_t bytes) { return ws_alloc(h, "gdx_prepare", p, bytes); };
    auto A = [&](float** p, size_t n) { return raw((void**)p, n * sizeof(float)); };
    // the sides of an activation pair this mode uses; every fp32 side is allocated before the first 16-bit one, in the order below
    // (the order of the guard zones gdx_check_guards reports)
    auto act = [&](Act& a, size_t n, bool want_f32, bool want_16) {
        return (want_f32 && A(&a.f, n)) || (want_16 && raw((void**)&a.h, n * 2));
    };
    const bool half = h->f16, f32 = !half, v2 = h->cfg.arch == GDX_ARCH_MDM;
    const bool res32 = f32 || h->stream32;                         // the residual stream is fp32 (add_norm)
    if (act(h->xa, N * d, true, false) || A(&h->addend, N * d) || A(&h->seed_cat, B2 * d) || A(&h->temb_in, B2 * d) ||
        A(&h->temb_h, B2 * d) || A(&h->temb, B2 * d) || A(&h->coa, B2 * d) || A(&h->c2, (B2 + 1) * d) ||
        A(&h->c2_seed, B2 * d) ||
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
    h->B = batch; h->T = frames;
    return 0;
}

// gdx_set_guards / gdx_set_keep_taps: the flag shapes the workspace, so a change re-prepares it at the current shape
static int set_workspace_flag(gdx_model* h, bool& flag, bool on) {
    if (flag == on) return 0;
    flag = on;
    const int B = h->B, T = h->T;
    if (!B) return 0;
    h->B = 0;
    return gdx_prepare(h, B, T);
}

extern "C" int gdx_set_guards(gdx_handle_t h, int32_t on) {
    if (!h) return fail("gdx_set_guards: null handle");
    return set_workspace_flag(h, h->guards, on != 0);
}

extern "C" int gdx_check_guards(gdx_handle_t h, int64_t* bad_bytes, int32_t* first_bad_zone, void* stream) {
    if (!h || !bad_bytes) return fail("gdx_check_guards: null argument");
    if (!h->guards) return fail("gdx_check_guards: guards are off (gdx_set_guards)");
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
    const int64_t maxc = 2LL * h->B * h->S * h->d;
    if (count > maxc) return fail("gdx_get_tap: count too large");
    HIPCHK(hipMemcpyAsync(out, h->taps[which], count * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

// what a conditioning does once seed_cat holds its 2B rows: the audio term, the seed half of the coarse slice, the flags
static int finish_condition(gdx_model* h, const float* mfcc, hipStream_t s) {
    const int B = h->B, T = h->T, S = h->S, d = h->d;
    if (h->cfg.arch == GDX_ARCH_MDM_OLD) {
        // addend[b, t+1, :] = W_in[:, J:] mfcc[b,:,t] + b_in + pe[t+1]      (model/mdm_old.py:104-112)
        HIPCHK(launch_mfcc_project(mfcc, h->in_mfcc.w, h->in_mfcc.kpad, h->in_x.bias, h->pe, h->addend, 2 * B, B,
                                   h->cfg.mfcc_dim, T, d, S, 1, s));
    } else {
        // audio_term[b*T+t, :] = W_proj[:, d:d+26] mfcc[b,:,t] + b_proj     (model/mdm.py:151-169)
        HIPCHK(launch_mfcc_project(mfcc, h->proj_audio.w, h->proj_audio.kpad, h->proj_pose.bias, nullptr, h->addend,
                                   2 * B, B, h->cfg.mfcc_dim, T, d, T, 0, s));
        // seed half of the coarse slice of project_to_lat (model/mdm.py:154-169), cond and uncond rows
        HIPCHK(launch_small_linear(h->seed_cat, d, h->proj_coa.w, h->proj_coa.kpad, nullptr, h->c2_seed, d, 2 * B, d, d, 0, s));
    }
    h->cond_set = true;
    h->gd_valid = false;                                          // guidance refresh: the difference of another conditioning
    h->lc_valid = false;                                          // layer cache: the change under another conditioning
    return 0;
}

extern "C" int gdx_set_condition(gdx_handle_t h, const float* seed, const float* mfcc, void* stream) {
    if (!h || !seed || !mfcc) return fail("gdx_set_condition: null argument");
    if (h->cfg.text_dim > 0) return fail("gdx_set_condition: this handle has text_dim > 0: call gdx_set_condition_text");
    if (gdx_weights_ready(h)) return -1;
    if (!h->B) return fail("gdx_set_condition: call gdx_prepare first");
    hipStream_t s = (hipStream_t)stream;
    const int B = h->B, d = h->d;
    // cond rows 0..B-1: Linear(flat seed); uncond rows B..2B-1: Linear(0) = bias   (model/mdm.py:125-127,242-250)
    HIPCHK(launch_small_linear(seed, h->J * h->cfg.seed_poses, h->seed.w, h->seed.kpad, h->seed.bias, h->seed_cat, d, B,
                               d, h->J * h->cfg.seed_poses, 0, s));
    for (int b = 0; b < B; ++b)
        HIPCHK(hipMemcpyAsync(h->seed_cat + (size_t)(B + b) * d, h->seed.bias, sizeof(float) * d,
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
    // uncond rows B..2B-1: both inputs zeroed before their Linear = [embed_text.bias | seed_embed.bias]: the same launches over
    // no input column (K = 0)
    float* un = h->seed_cat + (size_t)B * d;
    HIPCHK(launch_small_linear(text, cd, h->text.w, h->text.kpad, h->text.bias, un, d, B, td, 0, 0, s));
    HIPCHK(launch_small_linear(seed, ks, h->seed.w, h->seed.kpad, h->seed.bias, un + td, d, B, d - td, 0, 0, s));
    return finish_condition(h, mfcc, s);
}

// ctl (test / bench entry points only): a forced file or tile, the stamp buffer and the report of what ran (gdx_internal.h)
int gdx::gemm(int om, int ep, const GemmParams& p, hipStream_t s, GemmCtl* ctl) {
    hipError_t e;
    const int file = ctl ? ctl->file : 0;
    // Operands beyond the 2 GiB range of a buffer descriptor: the persistent kernel cannot address them and the 128 x 128 kernel
    // of gemm.hip would silently produce other bits for the same rows (another summation order).  Refuse instead: the caller
    // splits the batch (bench.py's config 4 runs sub-batches of 256 for this reason).
    if ((long)(p.M + ROW_PAD) * p.lda * 4 >= (1L << 31) || (long)(p.M + ROW_PAD) * p.ldc * 4 >= (1L << 31))
        return fail("gemm: an operand exceeds the 2 GiB buffer-descriptor range; run the batch in smaller pieces");
    // persistent kernel: residual / per-sample-vector terms are selected by the pointers, not by the mode
    GemmParams q = p;
    int ep2 = ep;
    if (ep == EPI_BIAS || ep == EPI_GELU) { q.R = nullptr; q.V = nullptr; }
    if (ep == EPI_RES) { q.V = nullptr; ep2 = EPI_BIAS; }
    if (ep == EPI_RES_VEC) { q.bias = nullptr; ep2 = EPI_BIAS; }
    if (file != 2 && gemm2_supported(om, ep2, q)) {
        e = launch_gemm2(om, ep2, q, s, ctl);
        if (e == hipSuccess) return 0;
        if (e != hipErrorNotSupported) return fail(std::string("launch_gemm2: ") + hipGetErrorString(e));
    }
    if (file == 1) return fail("gemm: the persistent kernel (gemm2.hip) does not take this problem");
    // shapes the persistent kernel does not take (N not a multiple of 64, K not a multiple of 32, unaligned rows)
    e = launch_gemm(om, ep, p, s, ctl);
    if (e != hipSuccess) return fail(std::string("launch_gemm: ") + hipGetErrorString(e));
    return 0;
}

bool gdx::local_attention_half(int dtype, int d, int heads, int window) {
    return dtype != GDX_DTYPE_F32 && HFN(dtype == GDX_DTYPE_BF16, local_attention_f16_supported, d, heads, window);
}
hipError_t gdx::launch_local_attention_any(int dtype, const float* xseq, const _Float16* xseq16, const float* cosT,
                                           const float* sinT, float* enc, _Float16* enc16, int B, int T, int d, int heads,
                                           int window, hipStream_t s) {
    const bool bf = dtype == GDX_DTYPE_BF16;
    if (local_attention_half(dtype, d, heads, window))
        return HFN(bf, launch_local_attention_f16, xseq16, cosT, sinT, enc16, enc, B, T, d, heads, window, s);
    return HFN(bf, launch_local_attention, xseq, cosT, sinT, enc, enc16, B, T, d, heads, window, s);
}

// ---- the per-step kernel sequence: three helpers that hide the compute mode, and the sequence itself, written once ----

// One GEMM launch, out = act(in W^T + bias + R + V); rowmap: frames into rows (b, t + 1) of [B, T+1, d], token 0 skipped
struct Terms {
    const float* bias = nullptr;
    const float* R = nullptr; int ldr = 0;   // fp32 per-output-row term
    const float* V = nullptr; int ldv = 0;   // fp32 per-sample vector
    bool gelu = false, rowmap = false;
};
// fp32 mode: in.f -> out.f through gemm().  16-bit modes: gemmh.hip reads in.h ([M][kpad16] halves with exactly M readable rows)
// and writes each side of `out` that is given.  Rows of `in` are W's padded K wide, rows of `out` ldc.
static int linear(gdx_model* h, const Act& in, const Packed& W, const Terms& t, Act out, int ldc, int M, int N, hipStream_t s) {
    if (!h->f16) {
        const int ep = t.gelu ? EPI_GELU : t.R && t.V ? EPI_RES_VEC : t.R ? EPI_RES : EPI_BIAS;
        const GemmParams p{in.f, W.kpad, W.w, W.kpad, t.bias, t.R, t.ldr, t.V, t.ldv, out.f, ldc, M, N, W.kpad, h->T};
        return gemm(t.rowmap ? OUT_TOKROWS : OUT_ROWS, ep, p, s);
    }
    const size_t ab = (size_t)M * W.kpad16 * 2, wb = (size_t)W.npad16 * W.kpad16 * 2;
    if (ab >= (1ull << 31) || wb >= (1ull << 31)) return fail("gemm_f16: an operand exceeds the 2 GiB buffer-descriptor range; run the batch in smaller pieces");
    if (N > W.npad16) return fail("gemm_f16: N exceeds the packed weight");
    GemmHParams p{in.h, W.kpad16, W.w16, W.kpad16, (int)ab, (int)wb, t.bias, t.R, t.ldr, t.V, t.ldv, out.f, out.f ? ldc : 0,
                  out.h, out.h ? ldc : 0, M, N, W.kpad16, h->T, t.rowmap, t.gelu};
    hipError_t e = HFN(h->bf16, launch_gemmh, p, s);
    if (e != hipSuccess) return fail(std::string("launch_gemmh: ") + hipGetErrorString(e));
    return 0;
}

// Self-attention of Beff samples: qkv -> ctx
static int attend(gdx_model* h, int Beff, hipStream_t s) {
    if (h->f16)
        HIPCHK(HFN(h->bf16, launch_attentionh, h->qkv.h, h->ctx.h, Beff, h->S, h->H, h->d, h->rows_alloc, s));
    else if (attention3_supported(h->S, h->H, h->d))
        HIPCHK(launch_attention3(h->qkv.f, h->ctx.f, Beff, h->S, h->H, h->d, s));
    else                                              // other head dims / more than 256 tokens: the general 32 x 32-block kernel
        HIPCHK(launch_attention(h->qkv.f, h->ctx.f, Beff, h->S, h->H, h->d, s));
    return 0;
}

// out = LayerNorm(resid + Linear(in)) over N token rows, through h->tmp: into *out (if given) and, without token 0 of every
// sample, into *compact (if given); each side of them that is named is written.  The one place that knows where the residual is
// added.  fp32 residual stream (the fp32 mode, and the 16-bit modes under stream32): in the GEMM epilogue (prefetched one tile
// ahead, gemm2.hip), which writes fp32; the LayerNorm writes the fp32 stream and / or the 16-bit copy the next GEMM reads.
// 16-bit stream: the GEMM rounds its output to 16 bits and the LayerNorm adds the 16-bit residual.
static int add_norm(gdx_model* h, const Act& in, const Packed& W, const Act& resid, const float* gamma, const float* beta,
                    const Act* out, const Act* compact, int N, hipStream_t s) {
    const int d = h->d;
    const bool res32 = !h->f16 || h->stream32;
    if (res32 ? linear(h, in, W, {.bias = W.bias, .R = resid.f, .ldr = d}, Act{h->tmp.f, nullptr}, d, N, d, s)
              : linear(h, in, W, {.bias = W.bias}, Act{nullptr, h->tmp.h}, d, N, d, s))
        return -1;
    for (const Act* o : {out, compact}) {
        if (!o) continue;
        const int cS = o == compact ? h->S : 0;
        if (res32) HIPCHK(HFN(h->bf16, launch_layernorm, h->tmp.f, nullptr, gamma, beta, o->f, o->h, N, d, cS, s));
        else HIPCHK(HFN(h->bf16, launch_layernorm_f16, h->tmp.h, resid.h, gamma, beta, o->h, o->f, N, d, cS, s));
    }
    return 0;
}

// The denoiser: x0 for Beff samples into x0_out ([Beff, J, T]).  temb: [*, d] rows (row stride tstride, 0 = shared by the batch).
// c2t (V2 only): W_coa * temb rows with the same row stride as temb -- the timestep half of the coarse slice of
// project_to_lat (model/mdm.py:154-169), computed by the caller with the row-independent small_linear kernel: per
// sample in gdx_forward, once per kept step in gdx_sample_loop, hence the same bits on both sides of the seam.
// state != nullptr (graph replay, gdx_sample_loop): temb / c2t are the BASES of the loop's tables and the row index is
// read from device memory (state[0]) by the conditioning-token kernel.
// tm (gdx_sample_loop's token-major fast path): the pose operand is already in h->xt and the prediction is left in h->x0t,
// both token-major -- neither transpose runs (x / x0_out unused).
// 16-bit modes: GEMM and attention operands are 16-bit, and so is the residual stream unless stream32; every accumulation (MFMA,
// the terms of the GEMM epilogues, LayerNorm statistics, softmax) is fp32, and so are the two boundary tensors: the pose tensor
// read by the input transpose and the x0 prediction.
// lc (layer cache, gdx.h gdx_set_layer_cache; the loops' layer_call decides): LC_FULL = today's forward, which also keeps the
// stream after layer lc_keep - 1 and stores the change of the deeper layers; LC_PARTIAL = layers 0 .. lc_keep - 1 only, the output
// GEMM's operand formed from their output plus the stored change.  LC_OFF issues exactly the launches of a handle without a cache.
enum { LC_OFF = 0, LC_FULL = 1, LC_PARTIAL = 2 };

// gdx_layer_delta on device buffers whose pairing is already one of the three: the fp32 instance, or the build of the 16-bit type
static int layer_delta(int op, int in_dtype, int out_dtype, int B, int T, int d, const void* in, void* outc, float* delta,
                       hipStream_t s) {
    if (out_dtype == GDX_DTYPE_F32) HIPCHK(launch_layer_delta(op, (const float*)in, (float*)outc, delta, B, T, d, s));
    else HIPCHK(HFN(out_dtype == GDX_DTYPE_BF16, launch_layer_delta_h, op, in_dtype == GDX_DTYPE_F32, in, (_Float16*)outc, delta, B, T, d, s));
    return 0;
}

static int forward_core(gdx_model* h, const float* x, const float* temb, int tstride, const float* c2t, int mode,
                        float* x0_out, hipStream_t s, const int* state = nullptr, bool tm = false, int lc = LC_OFF) {
    const int B = h->B, T = h->T, S = h->S, d = h->d, J = h->J;
    const int Beff = mode == GDX_CFG ? 2 * B : B;
    const int layers = lc == LC_PARTIAL ? h->lc_keep : h->L;     // encoder layers this call launches
    h->forward_samples += Beff;                                   // gdx_forward_samples (host side only)
    h->forward_layer_samples += (int64_t)Beff * layers;           // gdx_forward_layer_samples
    // layer cache: the residual stream is fp32 in the fp32 mode and under stream32, else the 16-bit type; the operand of the
    // output GEMM is fp32 in the fp32 mode only
    const bool res32 = !h->f16 || h->stream32;
    const int lc_in_dt = res32 ? GDX_DTYPE_F32 : h->cfg.compute_dtype, lc_out_dt = h->cfg.compute_dtype;
    const void* lc_stream = res32 ? (const void*)h->xa.f : (const void*)h->xa.h;
    void* lc_xc = h->f16 ? (void*)h->xc.h : (void*)h->xc.f;
    if (lc != LC_OFF) {
        if (lc == LC_PARTIAL && (!h->lc_valid || !h->lc_delta)) return fail("forward_core: a partial call without a stored layer change");
        if (!h->lc_delta) {
            const size_t rows = 2 * (size_t)B * S;
            if (ws_alloc(h, "layer cache", (void**)&h->lc_delta, sizeof(float) * 2 * B * T * d) ||
                ws_alloc(h, "layer cache", &h->lc_in, rows * d * (res32 ? 4 : 2)))
                return -1;
            HIPCHK(hipStreamSynchronize(nullptr));                 // the fills are on the null stream, the first store on s
        }
    }
    const float* seed_emb = mode == GDX_UNCOND ? h->seed_cat + (size_t)B * d : h->seed_cat;
    const int N = Beff * S;
    // the encoder stream as the sublayers write it: in the 16-bit stream its fp32 side only for the parity taps
    const Act xa{!h->f16 || h->stream32 || h->keep_taps ? h->xa.f : nullptr, h->xa.h};
    // pose tensor [B, J, 1, T] -> token-major [Beff*T, Jpad] once (CFG: the same x feeds both halves); tm: the update kernel wrote it
    if (!tm && !h->f16) HIPCHK(launch_transpose_in(x, h->xt.f, Beff, B, J, T, h->in_x.kpad, s));
    if (!tm && h->f16) HIPCHK(HFN(h->bf16, launch_transpose_in_f16, x, h->xt.h, Beff, B, J, T, h->in_x.kpad16, s));
    if (h->cfg.arch == GDX_ARCH_MDM_OLD) {
        HIPCHK(HFN(h->bf16, launch_token0, temb, tstride, seed_emb, h->pe, h->xa.f, h->xa.h, nullptr, nullptr, nullptr, state, Beff, B, S, d, s));
        // frames -> rows (b, t+1) of the encoder input, + hoisted MFCC/bias/PE term      (model/mdm_old.py:104-112)
        if (linear(h, h->xt, h->in_x, {.R = h->addend, .ldr = d, .rowmap = true}, xa, d, Beff * T, d, s)) return -1;
    } else {
        // coarse slice of project_to_lat = W_coa temb (c2t, from the caller) + W_coa seed_emb (c2_seed, per conditioning)
        if (!c2t) return fail("forward_core: V2 needs the W_coa * temb rows");
        const float* c2s = mode == GDX_UNCOND ? h->c2_seed + (size_t)B * d : h->c2_seed;
        HIPCHK(HFN(h->bf16, launch_token0, temb, tstride, seed_emb, nullptr, h->xa.f, h->xa.h, c2t, c2s, h->c2, state, Beff, B, S, d, s));
        if (linear(h, h->xt, h->in_x, {.bias = h->in_x.bias}, h->emb, d, Beff * T, d, s)) return -1;
        // proj_pose writes the operand the front end's kernel reads: 16-bit xseq.h, or fp32 xseq.f for the fp32 kernels
        const int dt = h->cfg.compute_dtype;
        const bool la16 = local_attention_half(dt, d, h->cfg.cl_head, h->cfg.window);
        const Act xseq = la16 ? Act{nullptr, h->xseq.h} : Act{h->xseq.f, nullptr};
        if (linear(h, h->emb, h->proj_pose, {.R = h->addend, .ldr = d, .V = h->c2, .ldv = d}, xseq, d, Beff * T, d, s)) return -1;
        HIPCHK(launch_local_attention_any(dt, h->xseq.f, h->xseq.h, h->rope_cos, h->rope_sin, la16 ? xa.f : h->xa.f, h->xa.h, Beff, T,
                                          d, h->cfg.cl_head, h->cfg.window, s));
    }
    auto tap = [&](int l) {
        if (h->keep_taps) HIPCHK(hipMemcpyAsync(h->taps[l], h->xa.f, sizeof(float) * (size_t)N * d, hipMemcpyDeviceToDevice, s));
        return 0;
    };
    if (tap(0)) return -1;
    for (int l = 0; l < layers; ++l) {
        const Layer& ly = h->layers[l];
        if (linear(h, h->xa, ly.qkv, {.bias = ly.qkv.bias}, h->qkv, 3 * d, N, 3 * d, s) || attend(h, Beff, s)) return -1;
        if (add_norm(h, h->ctx, ly.out, h->xa, ly.g1, ly.b1, &h->xb, nullptr, N, s)) return -1;        // x = LN1(x + out_proj(ctx))
        const bool stamp = h->prof && h->prof_used + 2 <= h->prof_ev.size();
        if (stamp) HIPCHK(hipEventRecord(h->prof_ev[h->prof_used], s));
        if (linear(h, h->xb, ly.ff1, {.bias = ly.ff1.bias, .gelu = true}, h->ffb, h->ff, N, h->ff, s)) return -1;
        if (stamp) {
            HIPCHK(hipEventRecord(h->prof_ev[h->prof_used + 1], s));
            h->prof_used += 2;
        }
        // x = LN2(x + ff2(.)); the last layer's output is only needed without token 0 (model/mdm.py:219): compacted [Beff*T, d]
        const bool last = l + 1 == h->L;
        if (add_norm(h, h->ffb, ly.ff2, h->xb, ly.g2, ly.b2, !last || h->keep_taps ? &xa : nullptr, last ? &h->xc : nullptr, N, s))
            return -1;
        if (tap(l + 1)) return -1;
        // layer cache, full call: the stream after layer lc_keep - 1 outlives the deeper layers, which overwrite xa
        if (lc == LC_FULL && l + 1 == h->lc_keep)
            HIPCHK(hipMemcpyAsync(h->lc_in, lc_stream, (size_t)N * d * (res32 ? 4 : 2), hipMemcpyDeviceToDevice, s));
    }
    if (lc == LC_FULL) {                                          // change of layers lc_keep .. L-1 on the rows the output GEMM reads
        if (layer_delta(0, lc_in_dt, lc_out_dt, Beff, T, d, h->lc_in, lc_xc, h->lc_delta, s)) return -1;
        h->lc_valid = true; h->lc_mode = mode;
    }
    // partial call: the operand from this call's own shallow layers plus the stored change (a GDX_COND call under a stored
    // GDX_CFG reads the conditional rows, the first B)
    if (lc == LC_PARTIAL && layer_delta(1, lc_in_dt, lc_out_dt, Beff, T, d, lc_stream, lc_xc, h->lc_delta, s)) return -1;
    if (h->keep_taps) {                                           // tap L + 1: the output GEMM's operand, widened
        if (h->f16) HIPCHK(HFN(h->bf16, launch_convert_f32, h->xc.h, h->taps[h->L + 1], (int64_t)Beff * T * d, s));
        else HIPCHK(hipMemcpyAsync(h->taps[h->L + 1], h->xc.f, sizeof(float) * (size_t)Beff * T * d, hipMemcpyDeviceToDevice, s));
    }
    // OutputProcess (model/mdm.py:372-380): token-major fp32 GEMM, then the permute back to [B, J, 1, T]
    if (linear(h, h->xc, h->outp, {.bias = h->outp.bias}, Act{h->x0t, nullptr}, h->ldo, Beff * T, h->ldo, s)) return -1;
    if (!tm) HIPCHK(launch_transpose_out(h->x0t, x0_out, Beff, J, T, h->ldo, s));
    return 0;
}

static int check_ready(gdx_model* h, const char* who) {
    if (!h) return fail(std::string(who) + ": null handle");
    if (!h->B) return fail(std::string(who) + ": call gdx_prepare first");
    if (!h->cond_set) return fail(std::string(who) + ": call gdx_set_condition first");
    return 0;
}

static int check_mode(const char* who, int mode, const float* scale) {
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
    h->gd_valid = false;
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
    h->lc_valid = false;
    return 0;
}

extern "C" int gdx_forward_layer_samples(gdx_handle_t h, int64_t* n) {
    if (!h || !n) return fail("gdx_forward_layer_samples: null argument");
    *n = h->forward_layer_samples;
    return 0;
}

// The stand-alone delta pass (gdx.h); every refusal precedes the first HIP call
extern "C" int gdx_layer_delta(int32_t op, int32_t in_dtype, int32_t out_dtype, int32_t batch, int32_t frames, int32_t width,
                               const void* in, void* outc, float* delta, void* stream) {
    if (op != 0 && op != 1) return fail("gdx_layer_delta: op must be 0 (store) or 1 (apply)");
    const bool pairing = (in_dtype == GDX_DTYPE_F32 && out_dtype == GDX_DTYPE_F32) || (in_dtype == GDX_DTYPE_F16 && out_dtype == GDX_DTYPE_F16) ||
                         (in_dtype == GDX_DTYPE_F32 && out_dtype == GDX_DTYPE_BF16);
    if (!pairing) return fail("gdx_layer_delta: the (in, out) element types must be (fp32, fp32), (fp16, fp16) or (fp32, bf16)");
    if (batch <= 0 || frames <= 0 || width <= 0) return fail("gdx_layer_delta: batch, frames and width must be positive");
    if (width % 32) return fail("gdx_layer_delta: width must be a multiple of 32 (there is only a 128-bit path)");
    if (!in || !outc || !delta) return fail("gdx_layer_delta: null argument");
    if (((uintptr_t)in | (uintptr_t)outc | (uintptr_t)delta) & 15) return fail("gdx_layer_delta: every pointer must be 16-byte aligned");
    return layer_delta(op, in_dtype, out_dtype, batch, frames, width, in, outc, delta, (hipStream_t)stream);
}

// step_mode's internal answers under the guidance refresh (gdx.h), never a loop's own mode: a guided call that stores the
// difference c - u, and one that runs the conditional pass alone and reuses the stored difference
static constexpr int GDX_CFG_REFRESH = GDX_CFG + 1, GDX_CFG_REUSE = GDX_CFG + 2;

// The sequence of denoiser calls a call belongs to, as far as the numbering of its guided calls needs it: the loop's mode and
// timestep map, the WHOLE loop's first index (first_index + k_base of a block), the index of the second call of gdx_plms_loop's
// step 0 (-1: the loop has none), and whether the loop takes part in the refresh and in the layer cache at all (gdx_bpd_loop and
// gdx_ddim_reverse_loop do not)
struct CallSeq {
    int mode;
    const int64_t* timestep_map;
    int first, second;
    bool refresh;
    bool cache = false;
};
template <typename A>
static CallSeq call_seq(const A* a, bool two_calls) {
    const int first = a->first_index + a->k_base;
    return CallSeq{a->mode, a->timestep_map, first, two_calls ? (first - 1 + a->num_steps) % a->num_steps : -1, true, true};
}

static bool guided_at(const gdx_model* h, const CallSeq& q, int idx) {
    const int64_t tau = q.timestep_map[idx];
    return q.mode == GDX_CFG && h->guide_lo <= tau && tau <= h->guide_hi;
}

// The mode of ONE denoiser call of a loop, at index idx (second: the second call of gdx_plms_loop's step 0, at q.second):
// guidance only while the call's model timestep lies in the handle's interval, else the plain conditional pass (B samples, no
// blend).  With gdx_set_guidance_refresh's every > 1 a guided call is numbered n = the guided calls of the loop before it, in
// execution order q.first, q.second, q.first - 1, q.first - 2, ..., and n % every decides between GDX_CFG_REFRESH and
// GDX_CFG_REUSE.  Every in-library loop asks here.
// mode_after: the same answer from n itself, for a caller that walks the calls in order (layer_call).
static int mode_after(const gdx_model* h, const CallSeq& q, int idx, int n) {
    if (q.mode != GDX_CFG) return q.mode;
    if (!guided_at(h, q, idx)) return GDX_COND;
    if (h->guide_every == 1 || !q.refresh) return GDX_CFG;
    return n % h->guide_every == 0 ? GDX_CFG_REFRESH : GDX_CFG_REUSE;
}
static int step_mode(const gdx_model* h, const CallSeq& q, int idx, bool second = false) {
    int n = 0;
    if (q.mode == GDX_CFG && h->guide_every > 1 && q.refresh && guided_at(h, q, idx)) {
        if (second) {
            n = guided_at(h, q, q.first);
        } else {
            for (int j = q.first; j > idx; --j) n += guided_at(h, q, j);
            if (q.second >= 0 && idx < q.first) n += guided_at(h, q, q.second);
        }
    }
    return mode_after(h, q, idx, n);
}

// what forward_core is run with for step_mode's answer m: a refresh is the full guided forward, a reuse the conditional pass alone
static int forward_mode(int m) { return m == GDX_CFG_REFRESH ? GDX_CFG : m == GDX_CFG_REUSE ? GDX_COND : m; }

// Layer cache (gdx.h, gdx_set_layer_cache): what ONE denoiser call of q's loop does -- lc = LC_FULL or LC_PARTIAL (LC_OFF: no
// cache on the handle, or a loop that takes no part) -- and K, the forward mode stored by the loop's most recent full call
// before it (-1: none).  The loop's calls are walked from its first one, in execution order q.first, q.second, q.first - 1, ...:
// call m is full when m % every == 0 or the stored mode does not cover its own.  No counter lives in the handle, so a block of
// a loop gets the plan of the whole loop.  Every in-library loop asks here.
struct LayerCall { int lc, K; };
static LayerCall layer_call(const gdx_model* h, const CallSeq& q, int idx, bool second = false) {
    if (h->lc_every == 1 || !q.cache) return {LC_OFF, -1};
    int K = -1, n = 0, m = 0;
    auto visit = [&](int j) {
        const int sm = mode_after(h, q, j, n), c = forward_mode(sm);
        n += sm >= GDX_CFG;
        const bool covers = K == c || (K == GDX_CFG && c == GDX_COND);
        const LayerCall r{m % h->lc_every == 0 || !covers ? LC_FULL : LC_PARTIAL, K};
        if (r.lc == LC_FULL) K = c;
        ++m;
        return r;
    };
    LayerCall r = visit(q.first);
    if (!second && idx == q.first) return r;
    if (q.second >= 0) {
        r = visit(q.second);
        if (second) return r;
    }
    for (int j = q.first - 1; j >= idx; --j) r = visit(j);
    return r;
}

// A block that issues q's loop from first_index must not begin with a partial call whose stored change is missing or of another
// mode than the plan's: asked before the call's first launch
static int check_layer_cache(const gdx_model* h, const char* who, const CallSeq& q, int first_index) {
    const LayerCall c = layer_call(h, q, first_index);
    if (c.lc == LC_PARTIAL && !(h->lc_valid && h->lc_mode == c.K))
        return fail(std::string(who) + ": a partial call would add the stored change of the deep layers, but none of the planned mode "
                    "is stored: a block-wise call (run_steps / k_base) must continue the loop that stored the change");
    return 0;
}

// A call that issues the steps first_index .. last_idx of q's loop must not begin with a reuse that has nothing to reuse: asked
// before the call's first launch
static int check_reuse(const gdx_model* h, const char* who, const CallSeq& q, int first_index, int last_idx) {
    for (int idx = first_index; idx >= last_idx; --idx) {
        const int m = step_mode(h, q, idx);
        if (m == GDX_CFG_REUSE && !h->gd_valid)
            return fail(std::string(who) + ": a guided call would reuse the guidance difference, but none is stored: a block-wise "
                        "call (run_steps / k_base) must continue the loop that stored the difference");
        if (m >= GDX_CFG) break;
    }
    return 0;
}

// gdx_cfg_rescale on the handle's buffers: c, u -> out for the B samples of the workspace, guided where t == nullptr or
// lo <= t[b] <= hi.  The chunk sums and factors belong to the handle (first use allocates, gdx_prepare resets).
static int rescale_x0(gdx_model* h, const float* c, const float* u, const float* scale, const int64_t* t, float* out, hipStream_t s) {
    const size_t per = (size_t)h->J * h->T, chunks = (per + GDX_BPD_CHUNK - 1) / GDX_BPD_CHUNK;
    if (!h->rs_part && dev_alloc(h->ws_allocs, (void**)&h->rs_part, sizeof(double) * 4 * h->B * chunks)) return -1;
    if (!h->rs_factor && dev_alloc(h->ws_allocs, (void**)&h->rs_factor, sizeof(float) * h->B)) return -1;
    gdx_cfg_rescale_args_t r;
    memset(&r, 0, sizeof(r));
    r.batch = h->B; r.njoints = h->J; r.frames = h->T;
    r.x0_cond = c; r.x0_uncond = u; r.scale = scale; r.phi = h->guide_phi;
    r.t = t; r.lo = h->guide_lo; r.hi = h->guide_hi;
    r.workspace = h->rs_part; r.factor = h->rs_factor; r.out = out;
    return gdx_cfg_rescale(&r, (void*)s);
}

// What the step kernel of a loop step in mode m gets as (x0_uncond, scale) after denoise_step left the prediction in h->x0.
// Guided without rescale: the uncond half and the scales, the kernel blends.  Guided with the handle's phi > 0: the rescaled
// guided prediction is formed here, in place on the cond half, and the kernel is called like on an unguided step (NULL, NULL).
// Under the guidance refresh (m = GDX_CFG_REFRESH / GDX_CFG_REUSE) the difference is stored or applied first (gdx_cfg_delta on
// the handle's buffer), and the step then continues as a guided one with (c, u or u', scale).  Every in-library loop asks here.
static int guided_operands(gdx_model* h, int m, const float* scale, hipStream_t s, const float** x0_uncond, const float** sc) {
    *x0_uncond = nullptr; *sc = nullptr;
    if (m < GDX_CFG) return 0;
    const size_t n = (size_t)h->B * h->J * h->T;
    float* u = h->x0 + n;
    if (m != GDX_CFG) {
        // guidance refresh: a refresh stores d = c - u; a reuse, whose forward left only c, forms u' = c - d in u's place
        if (!h->gd) {
            if (ws_alloc(h, "guidance refresh", (void**)&h->gd, sizeof(float) * n)) return -1;
            HIPCHK(hipStreamSynchronize(nullptr));                 // the fill is on the null stream, the first store on s
        }
        const bool store = m == GDX_CFG_REFRESH;
        const gdx_cfg_delta_args_t g{(int64_t)n, h->x0, store ? u : h->gd, store ? h->gd : u};
        if (gdx_cfg_delta(&g, (void*)s)) return -1;
        if (store) h->gd_valid = true;
    }
    if (h->guide_phi > 0.0f) return rescale_x0(h, h->x0, u, scale, nullptr, h->x0, s);
    *x0_uncond = u; *sc = scale;
    return 0;
}

// timestep embedding rows for idx[M] (model/mdm.py:296-310): pe gather -> Linear -> SiLU -> Linear.  The same
// row-independent kernel serves the per-sample rows of gdx_forward and the whole-loop table of gdx_sample_loop, so a
// timestep's embedding has the same bits on both sides of the seam (fused loop == step-wise protocol, bit for bit).
static int time_embed(gdx_model* h, const int64_t* idx, int M, float* gathered, float* hidden, float* out, hipStream_t s) {
    const int d = h->d;
    HIPCHK(launch_gather_rows(h->pe, idx, gathered, M, d, h->pe_rows, s));
    HIPCHK(launch_small_linear(gathered, d, h->time0.w, h->time0.kpad, h->time0.bias, hidden, d, M, d, d, 1, s));
    HIPCHK(launch_small_linear(hidden, d, h->time2.w, h->time2.kpad, h->time2.bias, out, d, M, d, d, 0, s));
    return 0;
}

extern "C" int gdx_forward(gdx_handle_t h, const float* x, const int64_t* timesteps, int32_t mode, const float* scale,
                           float* out, void* stream) {
    if (check_ready(h, "gdx_forward")) return -1;
    if (!x || !timesteps || !out) return fail("gdx_forward: null argument");
    if (check_mode("gdx_forward", mode, scale)) return -1;
    hipStream_t s = (hipStream_t)stream;
    if (time_embed(h, timesteps, h->B, h->temb_in, h->temb_h, h->temb, s)) return -1;
    const float* c2t = nullptr;
    if (h->cfg.arch == GDX_ARCH_MDM) {       // W_coa * temb per sample (h->coa doubles as the [B, d] buffer for it)
        HIPCHK(launch_small_linear(h->temb, h->d, h->proj_coa.w, h->proj_coa.kpad, nullptr, h->coa, h->d, h->B, h->d, h->d, 0, s));
        c2t = h->coa;
    }
    if (mode != GDX_CFG) return forward_core(h, x, h->temb, h->d, c2t, mode, out, s);
    if (forward_core(h, x, h->temb, h->d, c2t, mode, h->x0, s)) return -1;
    const int64_t per = (int64_t)h->J * h->T;
    // the timesteps are on the device: the double batch stays, the blend selects per sample (guided: blend, else c)
    if (h->guide_phi > 0.0f) return rescale_x0(h, h->x0, h->x0 + (size_t)h->B * per, scale, timesteps, out, s);
    HIPCHK(launch_cfg_blend(h->x0, h->x0 + (size_t)h->B * per, scale, timesteps, h->guide_lo, h->guide_hi, out, h->B, per, s));
    return 0;
}

// timestep-embedding table (and, V2, its W_coa image) for every kept step of a loop, shared by gdx_sample_loop and gdx_bpd_loop
static int build_step_tables(gdx_model* h, int num_steps, const int64_t* timestep_map, hipStream_t s) {
    const int d = h->d;
    // timestep-embedding table for every kept step, once per loop (same t for the whole batch:
    // gaussian_diffusion.py:712), through the respacing map (respace.py:124-129)
    if (h->temb_table_rows < num_steps) {
        float* t3 = nullptr;
        // + GDX_ROW_PAD rows behind the last of the three tables: the table linears run on the persistent GEMM, which
        // reads / stores whole tiles
        if (dev_alloc(h->ws_allocs, (void**)&t3, sizeof(float) * (3 * (size_t)num_steps + GDX_ROW_PAD) * d)) return -1;
        HIPCHK(hipMemsetAsync(t3, 0, sizeof(float) * (3 * (size_t)num_steps + GDX_ROW_PAD) * d, s));
        if (h->cfg.arch == GDX_ARCH_MDM && dev_alloc(h->ws_allocs, (void**)&h->c2t_table, sizeof(float) * ((size_t)num_steps + GDX_ROW_PAD) * d))
            return -1;
        if (dev_alloc(h->ws_allocs, (void**)&h->tmap_dev, sizeof(int64_t) * num_steps)) return -1;
        h->temb_table = t3;
        h->temb_table_rows = num_steps;
        h->tables_valid = false; h->c2t_valid = false;
    }
    float* table = h->temb_table;
    // the tables depend on the weights and the timestep map only: a loop run in blocks (run_steps) builds them once
    const bool tables_live = h->tables_valid && (int)h->tmap_host.size() == num_steps &&
                             !memcmp(h->tmap_host.data(), timestep_map, sizeof(int64_t) * num_steps) &&
                             (h->cfg.arch != GDX_ARCH_MDM || h->c2t_valid);
    if (tables_live) return 0;
    h->tmap_host.assign(timestep_map, timestep_map + num_steps);
    HIPCHK(hipMemcpyAsync(h->tmap_dev, h->tmap_host.data(), sizeof(int64_t) * num_steps, hipMemcpyHostToDevice, s));
    float* scratch0 = table + (size_t)h->temb_table_rows * d;
    float* scratch1 = scratch0 + (size_t)h->temb_table_rows * d;
    if (time_embed(h, h->tmap_dev, num_steps, scratch0, scratch1, table, s)) return -1;
    if (h->cfg.arch == GDX_ARCH_MDM) {
        // timestep half of the coarse slice of project_to_lat for every kept step, once per loop (same kernel as
        // gdx_forward's per-sample rows)
        HIPCHK(launch_small_linear(table, d, h->proj_coa.w, h->proj_coa.kpad, nullptr, h->c2t_table, d, num_steps, d, d, 0, s));
        h->c2t_valid = true;
    }
    h->tables_valid = true;
    return 0;
}

// The denoiser at schedule index `idx` of the loop tables build_step_tables left: x0_out (pose layout) from the state x; tm:
// the token-major variant (x / x0_out unused); state: a captured step, which reads its row number from the device (idx = 0)
static int denoise_step(gdx_model* h, const float* x, int idx, int mode, float* x0_out, hipStream_t s, const int* state = nullptr,
                        bool tm = false, int lc = LC_OFF) {
    const size_t row = (size_t)idx * h->d;
    return forward_core(h, x, h->temb_table + row, 0, h->c2t_table ? h->c2t_table + row : nullptr, forward_mode(mode), x0_out, s,
                        state, tm, lc);
}

// Executed step k's slice of a noise tape that starts at step k_base and holds `rows` samples ([rows][per]) per step
static const float* tape_slice(const float* tape, int k, int k_base, size_t rows, size_t per) {
    return tape ? tape + (ptrdiff_t)(k - k_base) * (ptrdiff_t)(rows * per) : nullptr;
}

// One forward of a loop at schedule index idx on the state x, in the mode of its own timestep (guidance interval), and the
// step kernel's view of its output in h->x0: (x0_uncond, scale).  Every in-library loop's eager step asks here; q: the loop's
// call sequence, sc_in: its scales, second: step_mode's.
static int denoise_guided(gdx_model* h, const CallSeq& q, const float* sc_in, const float* x, int idx, hipStream_t s,
                          const float** x0_uncond, const float** scale, bool second = false) {
    const int m = step_mode(h, q, idx, second);
    const int lc = layer_call(h, q, idx, second).lc;
    return denoise_step(h, x, idx, m, h->x0, s, nullptr, false, lc) || guided_operands(h, m, sc_in, s, x0_uncond, scale) ? -1 : 0;
}

// calc_bpd_loop (gaussian_diffusion.py:1537-1592): per step q_sample -> denoiser -> fused bound terms, through the SAME forward
// entry (pose-layout x_t, forward_core) the step-wise protocol reaches via gdx_forward, so both give the same bits.
extern "C" int gdx_bpd_loop(gdx_handle_t h, const gdx_bpd_loop_args_t* a, void* stream) {
    if (!h) return fail("gdx_bpd_loop: null handle");
    if (!a) return fail("gdx_bpd_loop: null argument");
    if (check_ready(h, "gdx_bpd_loop")) return -1;
    if (!a->coef || !a->timestep_map || !a->x_start || !a->vb || !a->xstart_mse || !a->mse)
        return fail("gdx_bpd_loop: null argument");
    if (check_mode("gdx_bpd_loop", a->mode, a->scale)) return -1;
    if (a->num_steps <= 0 || a->k_base < 0 || a->k_base >= a->num_steps || a->run_steps < 0 || a->k_base + a->run_steps > a->num_steps)
        return fail("gdx_bpd_loop: bad step range");
    if (a->inpaint_mask && !a->inpaint_motion) return fail("gdx_bpd_loop: mask without motion");
    hipStream_t s = (hipStream_t)stream;
    const int B = h->B;
    const size_t per = (size_t)h->J * h->T;
    const size_t chunks = (per + GDX_BPD_CHUNK - 1) / GDX_BPD_CHUNK;
    if (!h->bpd_xt && dev_alloc(h->ws_allocs, (void**)&h->bpd_xt, sizeof(float) * B * per)) return -1;
    if (!h->bpd_part && dev_alloc(h->ws_allocs, (void**)&h->bpd_part, sizeof(float) * 4 * B * chunks)) return -1;
    if (!a->noise_tape && !h->bpd_z && dev_alloc(h->ws_allocs, (void**)&h->bpd_z, sizeof(float) * B * per)) return -1;
    if (build_step_tables(h, a->num_steps, a->timestep_map, s)) return -1;
    gdx_bpd_args_t u;
    memset(&u, 0, sizeof(u));
    u.batch = B; u.njoints = h->J; u.frames = h->T;
    u.coef = a->coef; u.x_start = a->x_start; u.x_t = h->bpd_xt;
    u.x0_cond = h->x0;
    u.inpaint_mask = a->inpaint_mask; u.inpaint_motion = a->inpaint_motion;
    u.clip_denoised = a->clip_denoised;
    u.vb = a->vb; u.xstart_mse = a->xstart_mse; u.mse = a->mse; u.ld = a->num_steps;
    u.workspace = h->bpd_part;
    const int k_end = a->run_steps > 0 ? a->k_base + a->run_steps : a->num_steps;
    // no guidance refresh here: the steps draw independent x_t, so every guided call is a full one
    const CallSeq q{a->mode, a->timestep_map, a->num_steps - 1, -1, false};
    for (int k = a->k_base; k < k_end; ++k) {
        const int idx = a->num_steps - 1 - k;
        if (a->noise_tape) {
            u.noise = tape_slice(a->noise_tape, k, a->k_base, B, per);
            if (gdx_q_sample(a->x_start, u.noise, a->coef, idx, (int64_t)(B * per), h->bpd_xt, stream)) return -1;
        } else {
            u.noise = h->bpd_z;
            if (gdx_bpd_xt_(a->x_start, a->coef, idx, B, (long)per, a->philox_seed, a->sample_offset, (uint32_t)k, h->bpd_z, h->bpd_xt,
                            stream))
                return -1;
        }
        if (denoise_guided(h, q, a->scale, h->bpd_xt, idx, s, &u.x0_uncond, &u.scale)) return -1;
        u.step_index = idx; u.col = k;
        if (gdx_bpd_terms(&u, stream)) return -1;
    }
    if (a->prior_bpd) {
        u.prior = 1; u.prior_log_variance = a->prior_log_variance; u.step_index = a->num_steps - 1;
        u.vb = a->prior_bpd; u.ld = 1; u.col = 0;
        if (gdx_bpd_terms(&u, stream)) return -1;
    }
    return 0;
}

// The arguments U of a loop's step kernel at index idx, as far as every pose-layout step struct names them alike: the handle's
// shape, the loop's coefficients / state (updated in place) / inpainting / clip, and the denoiser's output as denoise_guided left it
template <typename U, typename A>
static U step_args(const gdx_model* h, const A* a, int idx, const float* x0_uncond, const float* scale) {
    U u;
    memset(&u, 0, sizeof(u));
    u.batch = h->B; u.njoints = h->J; u.frames = h->T;
    u.coef = a->coef; u.step_index = idx; u.x = a->x; u.out = a->x;
    u.x0_cond = h->x0; u.x0_uncond = x0_uncond; u.scale = scale;
    u.inpaint_mask = a->inpaint_mask; u.inpaint_motion = a->inpaint_motion; u.clip_denoised = a->clip_denoised;
    return u;
}

// The scaffold of the multistep loops gdx_plms_loop, gdx_dpm_loop, gdx_dpm_sde_loop and gdx_unipc_loop (`who`), whose argument
// structs A name the fields mode .. k_base alike: per step the denoiser through forward_core on the pose-layout state (the entry
// gdx_forward uses: same bits as the step-wise protocol), then step(idx, k, x0_uncond, scale, slot), the entry's own fused launch;
// slot(k) = executed step k's place in the caller's ring of `ring` buffers (0: a->order of them) at a->*hist; two_calls: step 0
// makes a second denoiser call (call_seq; the entry's step issues it).  No graph replay and no token-major variant:
// these solvers run 10-50 steps.  The argument checks need no handle and come first (then null handle, then not prepared), so
// every refusal precedes the first HIP call; missing() gives the entry's history refusal or nullptr.  A new multistep sampler
// is one more caller of this function ("Where a new in-library loop goes").
template <typename A, typename Missing, typename Step>
static int multistep_loop(const char* who, gdx_model* h, const A* a, int order_lo, int order_hi, const char* order_msg,
                          float* A::*hist, Missing missing, hipStream_t s, Step step, bool two_calls = false, int ring = 0) {
    const std::string w = std::string(who) + ": ";
    if (!a || !a->coef || !a->timestep_map || !a->x) return fail(w + "null argument");
    if (check_mode(who, a->mode, a->scale)) return -1;
    if (a->num_steps <= 0 || a->first_index < 0 || a->k_base < 0 || a->run_steps < 0 || a->first_index + a->k_base >= a->num_steps ||
        a->run_steps > a->first_index + 1)
        return fail(w + "bad step range");
    if (a->order < order_lo || a->order > order_hi) return fail(w + order_msg);
    if (a->inpaint_mask && !a->inpaint_motion) return fail(w + "mask without motion");
    if (const char* m = missing()) return fail(w + m);
    if (check_ready(h, who)) return -1;
    if (h->B > 65535) return fail(w + "batch exceeds 65535");
    const int last_idx = a->run_steps > 0 ? a->first_index - a->run_steps + 1 : 0;
    const CallSeq q = call_seq(a, two_calls);
    if (check_reuse(h, who, q, a->first_index, last_idx) || check_layer_cache(h, who, q, a->first_index)) return -1;
    if (build_step_tables(h, a->num_steps, a->timestep_map, s)) return -1;
    const size_t n = (size_t)h->B * h->J * h->T;
    const int depth = ring > 0 ? ring : a->order;
    auto slot = [&](int k) { return a->*hist + (size_t)(k % depth) * n; };
    int k = a->k_base;
    for (int idx = a->first_index; idx >= last_idx; --idx, ++k) {
        const float *x0u, *sc;
        if (denoise_guided(h, q, a->scale, a->x, idx, s, &x0u, &sc) || step(idx, k, x0u, sc, slot)) return -1;
    }
    return 0;
}

// plms_sample_loop (gaussian_diffusion.py:995-1190): one fused plms_step_kernel launch per step (sampler.hip); the first step
// needs the state in the reference layout twice.
extern "C" int gdx_plms_loop(gdx_handle_t h, const gdx_plms_loop_args_t* a, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    return multistep_loop(
        "gdx_plms_loop", h, a, 2, 4, "order must be 2, 3 or 4", &gdx_plms_loop_args_t::eps_hist,
        [&] { return !a->eps_hist || !a->scratch ? "missing history (eps_hist and scratch are the caller's)" : nullptr; }, s,
        [&](int idx, int k, const float* x0u, const float* sc, auto slot) -> int {
            auto u = step_args<gdx_plms_step_args_t>(h, a, idx, x0u, sc);
            if (k == 0) {                               // pseudo improved Euler (:1043-1052): predictor, second forward, corrector
                u.kind = 6; u.eps_out = slot(0); u.out = a->scratch; u.pred_xstart = slot(1);
                if (gdx_plms_step(&u, stream)) return -1;
                const int idx2 = (idx - 1 + a->num_steps) % a->num_steps;
                if (denoise_guided(h, call_seq(a, true), a->scale, a->scratch, idx2, s, &u.x0_uncond, &u.scale, true)) return -1;
                u.kind = 5; u.step_index_eps = idx2; u.x_eps = a->scratch; u.eps_hist[0] = slot(0); u.pred_prev = slot(1);
                u.eps_out = nullptr; u.out = a->x; u.pred_xstart = nullptr;
                return gdx_plms_step(&u, stream);
            }
            u.kind = k + 1 < a->order ? k + 1 : a->order;
            u.eps_out = slot(k);
            for (int j = 0; j < u.kind - 1; ++j) u.eps_hist[j] = slot(k - 1 - j);
            return gdx_plms_step(&u, stream);
        },
        true);
}

// dpm_solver_sample_loop (DPM-Solver++ multistep, gdx.h): one fused dpm_step_kernel launch per step (sampler.hip)
extern "C" int gdx_dpm_loop(gdx_handle_t h, const gdx_dpm_loop_args_t* a, void* stream) {
    return multistep_loop(
        "gdx_dpm_loop", h, a, 1, 3, "order must be 1, 2 or 3", &gdx_dpm_loop_args_t::hist,
        [&] { return a->order > 1 && !a->hist ? "missing history (hist is the caller's)" : nullptr; }, (hipStream_t)stream,
        [&](int idx, int k, const float* x0u, const float* sc, auto slot) -> int {
            auto u = step_args<gdx_dpm_step_args_t>(h, a, idx, x0u, sc);
            u.order = std::min(a->order, std::min(k + 1, idx + 1));      // warm-up at the start, lower order at the end
            for (int j = 0; j < u.order - 1; ++j) u.hist[j] = slot(k - 1 - j);
            u.pred_out = a->order > 1 ? slot(k) : nullptr;
            return gdx_dpm_step(&u, stream);
        });
}

// dpm_solver_sde_sample_loop (SDE-DPM-Solver++ multistep, gdx.h): gdx_dpm_loop with the noisy instantiation of dpm_step_kernel,
// whose noise is slice k - k_base of the tape or Philox draw k + 1
extern "C" int gdx_dpm_sde_loop(gdx_handle_t h, const gdx_dpm_sde_loop_args_t* a, void* stream) {
    return multistep_loop(
        "gdx_dpm_sde_loop", h, a, 1, 2, "order must be 1 or 2", &gdx_dpm_sde_loop_args_t::hist,
        [&] { return a->order > 1 && !a->hist ? "missing history (hist is the caller's)" : nullptr; }, (hipStream_t)stream,
        [&](int idx, int k, const float* x0u, const float* sc, auto slot) -> int {
            auto u = step_args<gdx_dpm_sde_step_args_t>(h, a, idx, x0u, sc);
            u.order = std::min(a->order, std::min(k + 1, idx + 1));      // warm-up at the start, first order on the step to sigma = 0
            u.hist[0] = u.order > 1 ? slot(k - 1) : nullptr;
            u.pred_out = a->order > 1 ? slot(k) : nullptr;
            u.noise = tape_slice(a->noise_tape, k, a->k_base, h->B, (size_t)h->J * h->T);
            u.philox_seed = a->philox_seed; u.sample_offset = a->sample_offset; u.rng_step = (uint32_t)(k + 1);
            return gdx_dpm_sde_step(&u, stream);
        });
}

// unipc_sample_loop (UniPC, gdx.h): one fused unipc_step_kernel launch per step (sampler.hip) -- the corrector of the step that
// led to a->x, then the predictor of the next input; a->base holds the corrected state, the ring is one deeper than the order
extern "C" int gdx_unipc_loop(gdx_handle_t h, const gdx_unipc_loop_args_t* a, void* stream) {
    return multistep_loop(
        "gdx_unipc_loop", h, a, 1, 3, "order must be 1, 2 or 3", &gdx_unipc_loop_args_t::hist,
        [&] { return !a->hist || !a->base || !a->coef_c ? "missing history (hist, base and coef_c are the caller's)" : nullptr; },
        (hipStream_t)stream,
        [&](int idx, int k, const float* x0u, const float* sc, auto slot) -> int {
            auto u = step_args<gdx_unipc_step_args_t>(h, a, idx, x0u, sc);
            u.corr_order = k == 0 || idx == 0 ? 0 : std::min(a->order, k);
            u.pred_order = std::min(a->order, std::min(k + 1, idx + 1));
            if (u.corr_order) u.x = a->base;                              // else the state itself: a->x
            u.coef_c = a->coef_c; u.base_out = a->base;
            for (int j = 0; j < std::max(u.corr_order, u.pred_order - 1); ++j) u.hist[j] = slot(k - 1 - j);
            u.pred_out = slot(k);
            return gdx_unipc_step(&u, stream);
        },
        false, a ? a->order + 1 : 0);
}

// ddim_reverse_sample_loop (DDIM inversion, gdx.h): multistep_loop's per-step pair -- denoise_guided on the pose-layout state, then
// one fused launch (ddim_reverse_step_kernel, sampler.hip) with step_args -- over ASCENDING indices.  An ascending twin and not a
// direction flag on multistep_loop: nothing else of that function applies here (no order, no history ring, no k_base, no second
// call, no check_reuse), and its step range and CallSeq are both written for first_index counting down.  The
// guidance refresh is off in the CallSeq, as in gdx_bpd_loop: the stored difference's numbering is defined for descending loops.
extern "C" int gdx_ddim_reverse_loop(gdx_handle_t h, int32_t mode, int32_t num_steps, int32_t first_index, int32_t run_steps,
                                     const float* coef, const int64_t* timestep_map, float* x, const float* scale,
                                     const uint8_t* inpaint_mask, const float* inpaint_motion, int32_t clip_denoised, void* stream) {
    const char* who = "gdx_ddim_reverse_loop";
    const std::string w = std::string(who) + ": ";
    if (!coef || !timestep_map || !x) return fail(w + "null argument");
    if (check_mode(who, mode, scale)) return -1;
    if (num_steps <= 0 || first_index < 0 || first_index >= num_steps || run_steps < 1 || run_steps > num_steps - first_index)
        return fail(w + "bad step range");
    if (inpaint_mask && !inpaint_motion) return fail(w + "mask without motion");
    if (check_ready(h, who)) return -1;
    if (h->B > 65535) return fail(w + "batch exceeds 65535");
    if (h->guide_every > 1)
        return fail(w + "the guidance refresh (gdx_set_guidance_refresh, every > 1) does not apply to the inversion: its numbering of "
                        "guided calls is defined for descending loops; set every = 1");
    hipStream_t s = (hipStream_t)stream;
    if (build_step_tables(h, num_steps, timestep_map, s)) return -1;
    const CallSeq q{mode, timestep_map, num_steps - 1, -1, false};
    // the loop's operands under the names step_args reads
    const struct { const float* coef; float* x; const uint8_t* inpaint_mask; const float* inpaint_motion; int32_t clip_denoised; }
        a{coef, x, inpaint_mask, inpaint_motion, clip_denoised};
    for (int idx = first_index; idx < first_index + run_steps; ++idx) {
        const float *x0u, *sc;
        if (denoise_guided(h, q, scale, x, idx, s, &x0u, &sc)) return -1;
        if (gdx_ddim_reverse_step_(step_args<gdx::DdimReverseStepArgs>(h, &a, idx, x0u, sc), stream)) return -1;
    }
    return 0;
}

extern "C" int gdx_sample_loop(gdx_handle_t h, const gdx_loop_args_t* a, void* stream) {
    if (check_ready(h, "gdx_sample_loop")) return -1;
    if (!a || !a->coef || !a->timestep_map || !a->x) return fail("gdx_sample_loop: null argument");
    if (check_mode("gdx_sample_loop", a->mode, a->scale)) return -1;
    if (a->num_steps <= 0 || a->first_index >= a->num_steps || a->first_index < 0 || a->run_steps < 0 || a->k_base < 0)
        return fail("gdx_sample_loop: bad step range");
    if (a->kind == GDX_SAMPLER_DDIM && (a->const_noise || a->n_dump))
        return fail("gdx_sample_loop: ddim_sample_loop supports neither const_noise nor dump_steps");  // :903-906
    hipStream_t s = (hipStream_t)stream;
    const int B = h->B;
    const int last_idx = a->run_steps > 0 && a->run_steps <= a->first_index ? a->first_index - a->run_steps + 1 : 0;
    // guidance refresh: the guided calls are numbered from the whole loop's first index
    // ... and so are the calls of the layer cache
    const bool refresh_on = (h->guide_every > 1 && a->mode == GDX_CFG) || h->lc_every > 1;
    if (refresh_on && a->first_index + a->k_base >= a->num_steps) return fail("gdx_sample_loop: bad step range");
    const CallSeq q{a->mode, a->timestep_map, a->first_index + a->k_base, -1, true, true};  // first: read only when refresh_on
    if (check_reuse(h, "gdx_sample_loop", q, a->first_index, last_idx) || check_layer_cache(h, "gdx_sample_loop", q, a->first_index))
        return -1;
    if (build_step_tables(h, a->num_steps, a->timestep_map, s)) return -1;

    const int64_t per = (int64_t)h->J * h->T;
    const size_t tape_rows = a->const_noise ? 1 : B;             // samples per step of the noise tape
    int dump_i = 0;
    while (dump_i < a->n_dump && a->dump_steps[dump_i] < a->k_base) ++dump_i;     // entries of earlier blocks
    auto mode_at = [&](int idx) { return step_mode(h, q, idx); };
    // (x0_uncond, scale): guided_operands' answer for the step
    auto fill_update = [&](gdx_update_args_t& u, int idx, int k, const float* x0_uncond, const float* scale) {
        u = step_args<gdx_update_args_t>(h, a, idx, x0_uncond, scale);
        u.kind = a->kind;
        u.noise = tape_slice(a->noise_tape, k, a->k_base, tape_rows, per);
        u.const_noise = a->const_noise;
        u.philox_seed = a->philox_seed; u.sample_offset = a->sample_offset; u.rng_step = (uint32_t)(k + 1);
    };
    auto eager_step = [&](int idx, int k) -> int {
        const float *x0u, *sc;
        if (denoise_guided(h, q, a->scale, a->x, idx, s, &x0u, &sc)) return -1;
        gdx_update_args_t u;
        fill_update(u, idx, k, x0u, sc);
        if (gdx_sampler_update(&u, stream)) return -1;
        while (a->dump && dump_i < a->n_dump && a->dump_steps[dump_i] <= k) {      // duplicates / stale entries never stall
            if (a->dump_steps[dump_i] == k)
                HIPCHK(hipMemcpyAsync(a->dump + (size_t)dump_i * B * per, a->x, sizeof(float) * B * per,
                                      hipMemcpyDeviceToDevice, s));
            ++dump_i;
        }
        return 0;
    };

    // Optional hipGraph replay of the step (gdx_set_graph_replay): ONE step is captured and replayed; everything that
    // changes from step to step (timestep-embedding row, coefficient row, Philox draw number, noise-tape slice) is read
    // from a two-int device state that a one-thread kernel advances at the end of the step.  Measured on MI355X /
    // ROCm 7.2 (tools/small_loop.py, 1000 steps, B=4 T=60 d=512 fp16): eager 0.307 ms/step, graph replay 0.337 -- the
    // ~65 small kernels of a step are bound by their GPU-side dispatch + ramp, not by host launch time, and a graph
    // node costs slightly more than a stream launch; so it is OFF by default and kept as a switch.
    // guidance interval: the modes this call's steps take (all the loop's own mode unless it is GDX_CFG)
    const int mode0 = mode_at(a->first_index);
    bool uniform = true, any_guided = false;
    for (int i = a->first_index; i >= last_idx; --i) {
        const int m = mode_at(i);
        uniform = uniform && m == mode0;
        any_guided = any_guided || m >= GDX_CFG;
    }
    // Token-major fast path (sampler.hip, update_tm_kernel): with nothing but the noise tape living in the reference layout
    // (no inpainting, no dumps; the tape is read in place), the state stays in the input GEMM's operand layout for the whole
    // call -- one transpose in front, none per step (2 launches and ~40 MB per step less), the last update also writes the
    // sample in the reference layout.  Bit-identical to the general path (tests: fused Philox loop == step-wise Philox loop).
    // the guidance rescale has no token-major variant: a call that rescales a step takes the general path; nor has the guidance
    // refresh, whose calls also run eagerly under graph replay (the stored difference is host-tracked state)
    const bool rescales = h->guide_phi > 0.0f && any_guided;
    const bool refreshes = h->guide_every > 1 && any_guided;
    if (!((uintptr_t)a->noise_tape & 15) && !a->inpaint_mask && !a->n_dump && !h->graph_replay && !h->keep_taps && h->T % 4 == 0 &&
        !rescales && !refreshes) {
        // guided loop: the state holds both halves (the same x feeds both passes).  An unguided step reads and writes the cond
        // half and mirrors into the uncond half only when the NEXT step of this call is guided (every call transposes the
        // state in afresh); a call without a guided step keeps one half, like a loop that is not guided at all.
        // GDX_TM_MIRROR=always mirrors on every unguided step of such a call (the A/B of DESIGN 4f).
        static const bool mirror_always = [] { const char* e = getenv("GDX_TM_MIRROR"); return e && !strcmp(e, "always"); }();
        const int Beff = any_guided ? 2 * B : B;
        // half modes: the fp32 state keeps the half operand's row stride, and the update kernel also writes that operand
        const int ldx = h->f16 ? h->in_x.kpad16 : h->in_x.kpad;
        HIPCHK(launch_transpose_in(a->x, h->xt.f, Beff, B, h->J, h->T, ldx, s));
        if (h->f16) HIPCHK(HFN(h->bf16, launch_transpose_in_f16, a->x, h->xt.h, Beff, B, h->J, h->T, ldx, s));
        gdx::UpdateTmDev u;
        memset(&u, 0, sizeof(u));
        u.kind = a->kind; u.B = B; u.J = h->J; u.T = h->T; u.ldx = ldx; u.ldo = h->ldo;
        u.coef = a->coef; u.xt = h->xt.f; u.x0t = h->x0t;
        u.const_noise = a->const_noise; u.seed = a->philox_seed; u.sample_offset = a->sample_offset;
        u.clip = a->clip_denoised;
        u.xt16 = h->xt.h; u.half_dtype = h->cfg.compute_dtype;
        int k = a->k_base;
        for (int idx = a->first_index; idx >= last_idx; --idx, ++k) {
            const int m = mode_at(idx);
            if (denoise_step(h, nullptr, idx, m, nullptr, s, nullptr, true, layer_call(h, q, idx).lc)) return -1;
            u.scale = m == GDX_CFG ? a->scale : nullptr;
            u.mirror = any_guided && m != GDX_CFG && (mirror_always || (idx > last_idx && mode_at(idx - 1) == GDX_CFG));
            u.step_index = idx; u.rng_step = (uint32_t)(k + 1);
            u.out_pose = idx == last_idx ? a->x : nullptr;
            u.noise = tape_slice(a->noise_tape, k, a->k_base, tape_rows, per);
            if (gdx_sampler_update_tm_(u, stream)) return -1;
        }
        return 0;
    }
    // the graph is ONE captured step: only a call whose steps all take the same mode can replay it
    const bool want_graph = h->graph_replay && !h->prof && !h->keep_taps && !a->n_dump && a->first_index - last_idx >= 8 && uniform && !refreshes &&
                            h->lc_every == 1;                     // the layer cache's calls differ from one another: eager
    int idx = a->first_index, k = a->k_base;
    if (want_graph) {
        if (eager_step(idx, k)) return -1;                        // step 0 eagerly: it also sets every kernel attribute
        --idx; ++k;
        bool ok = true;
        if (!h->gstream) {
            ok = hipStreamCreateWithFlags(&h->gstream, hipStreamNonBlocking) == hipSuccess &&
                 hipEventCreateWithFlags(&h->gev_in, hipEventDisableTiming) == hipSuccess &&
                 hipEventCreateWithFlags(&h->gev_out, hipEventDisableTiming) == hipSuccess &&
                 hipMalloc((void**)&h->gstate, 64) == hipSuccess;
            if (!ok) { (void)hipGetLastError(); }
        }
        if (ok && h->gexec) {                                     // the previous loop's graph: its launches must have drained
            (void)hipStreamSynchronize(h->gstream);
            (void)hipGraphExecDestroy(h->gexec); h->gexec = nullptr;
            (void)hipGraphDestroy(h->ggraph); h->ggraph = nullptr;
        }
        if (ok) {
            ok = launch_set_state(h->gstate, idx, k, s) == hipSuccess && hipEventRecord(h->gev_in, s) == hipSuccess &&
                 hipStreamWaitEvent(h->gstream, h->gev_in, 0) == hipSuccess;
        }
        if (ok && hipStreamBeginCapture(h->gstream, hipStreamCaptureModeThreadLocal) == hipSuccess) {
            const int64_t counted = h->forward_samples;          // the capture enqueues no forward: the replays are counted
            int rc = denoise_step(h, a->x, 0, mode0, h->x0, h->gstream, h->gstate);
            h->forward_samples = counted;
            const float *x0u = nullptr, *sc = nullptr;           // the rescale's launches depend on no per-step state: captured as they are
            if (!rc) rc = guided_operands(h, mode0, a->scale, h->gstream, &x0u, &sc);
            if (!rc) {
                gdx_update_args_t u;
                fill_update(u, 0, 0, x0u, sc);                    // noise: step 0's slice; the kernel adds state[1] * stride
                rc = gdx_sampler_update_state_(&u, h->gstate, (long)(tape_rows * per), (void*)h->gstream);
            }
            if (!rc && launch_advance_state(h->gstate, h->gstream) != hipSuccess) rc = -1;
            hipGraph_t g = nullptr;
            const hipError_t ee = hipStreamEndCapture(h->gstream, &g);
            if (rc || ee != hipSuccess || !g) {
                if (g) (void)hipGraphDestroy(g);
                (void)hipGetLastError();
                ok = false;
            } else if (hipGraphInstantiate(&h->gexec, g, nullptr, nullptr, 0) != hipSuccess) {
                (void)hipGraphDestroy(g);
                (void)hipGetLastError();
                h->gexec = nullptr;
                ok = false;
            } else {
                h->ggraph = g;
            }
        } else {
            ok = false;
            (void)hipGetLastError();
        }
        if (ok) {
            for (; idx >= last_idx; --idx, ++k) {
                HIPCHK(hipGraphLaunch(h->gexec, h->gstream));
                h->forward_samples += mode0 == GDX_CFG ? 2 * B : B;
            }
            HIPCHK(hipEventRecord(h->gev_out, h->gstream));
            HIPCHK(hipStreamWaitEvent(s, h->gev_out, 0));
            return 0;
        }
        g_err.clear();                                            // capture unavailable: finish the loop eagerly
    }
    for (; idx >= last_idx; --idx, ++k)
        if (eager_step(idx, k)) return -1;
    return 0;
}

// MFCC front end (reference data_loaders/gesture/data/dataset.py:81-95).  The caller supplies the tables (built once on the
// host in fp64, stored fp32) and the workspace; layouts:
//   dft  [2*nbp][Lp]   rows k < nbins: cos(2 pi k i / nfft), rows nbp + k: -sin(...), zero elsewhere; Lp = frame_len up to 32,
//                      nbp = nbins up to 64
//   mel  [64][nbp]     rows j < nfilt: triangular filter j over the nbins power bins, zero elsewhere
//   work               (numframes + GDX_ROW_PAD) * (Lp + 2*nbp + nbp + 64) + numframes floats
extern "C" int gdx_mfcc(const float* signal, int64_t n, int32_t frame_len, int32_t frame_step, int32_t numframes,
                        int32_t nfft, int32_t nfilt, int32_t numcep, float preemph, const float* dft, const float* mel,
                        const float* dct, const float* lifter, const float* mean, const float* stdv, float* work,
                        float* out, void* stream) {
    if (!signal || !dft || !mel || !dct || !lifter || !work || !out) return fail("gdx_mfcc: null argument");
    if (n <= 0 || frame_len <= 0 || frame_step <= 0 || numframes <= 0 || nfft < frame_len || nfilt <= 0 || nfilt > 64 ||
        numcep <= 0 || numcep > nfilt)
        return fail("gdx_mfcc: bad geometry");
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = gemm_init();
    if (e != hipSuccess) return fail(std::string("gemm_init: ") + hipGetErrorString(e));
    const int nbins = nfft / 2 + 1, Lp = round_up(frame_len, 32), nbp = round_up(nbins, 64), rows = numframes + GDX_ROW_PAD;
    float* frames = work;
    float* spec = frames + (size_t)rows * Lp;
    float* pw = spec + (size_t)rows * 2 * nbp;
    float* melv = pw + (size_t)rows * nbp;
    float* energy = melv + (size_t)rows * 64;
    HIPCHK(launch_mfcc_frames(signal, (long)n, frames, numframes, frame_len, frame_step, Lp, preemph, s));
    GemmParams p{frames, Lp, dft, Lp, nullptr, nullptr, 0, nullptr, 0, spec, 2 * nbp, numframes, 2 * nbp, Lp, 1};
    if (gemm(OUT_ROWS, EPI_BIAS, p, s)) return -1;                       // DFT: [F, L] x [2*nbins, L]^T
    HIPCHK(launch_mfcc_power(spec, 2 * nbp, nbp, pw, nbp, energy, numframes, nbins, nfft, s));
    GemmParams q{pw, nbp, mel, nbp, nullptr, nullptr, 0, nullptr, 0, melv, 64, numframes, 64, nbp, 1};
    if (gemm(OUT_ROWS, EPI_BIAS, q, s)) return -1;                       // mel energies
    HIPCHK(launch_mfcc_cepstrum(melv, 64, energy, dct, lifter, mean, stdv, out, numframes, nfilt, numcep, s));
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
    const double B = (mode == GDX_CFG ? 2.0 : 1.0) * h->B, T = h->T, S = h->S, d = h->d, J = h->J, ff = h->ff;
    const double N = B * S, Sp = h->cfg.seed_poses, mf = h->cfg.mfcc_dim;
    double f = 2 * B * d * d * 2 + 2 * B * J * Sp * d;
    if (h->cfg.arch == GDX_ARCH_MDM)
        f += 2 * B * T * J * d + 2 * B * T * (2 * d + mf) * d + 4 * B * T * 2 * h->cfg.window * d;
    else
        f += 2 * B * T * (J + mf) * d;
    f += h->L * (2 * N * d * 3 * d + 4 * B * S * S * d + 2 * N * d * d + 4 * N * d * ff);
    f += 2 * B * T * d * J;
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
