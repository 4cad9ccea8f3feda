// Host side shared by handle.hip (the model handle and its settings), forward.hip (the per-step kernel sequence), loops.hip (the
// in-library loops), weights.hip (what the handle's weights are and how they get there) and testapi.hip (the handle-free test /
// bench entry points); the helpers declared here are defined in the first three.
#pragma once
#include "gdx_call_plan.h"
#include "gdx_resample_plan.h"
#include "gdx_window_stride.h"
#include "gdx_internal.h"

#include <set>
#include <string>
#include <vector>

namespace gdx {

int fail(const std::string& m);   // records the text of gdx_last_error (thread-local); returns -1
void clear_error();               // ... and empties it again (a fallback that recovered)
#define HIPCHK(expr)                                                                       \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) return fail(std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

static inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// half-type dispatch: the reduced-precision kernels exist as gdx:: (fp16) and gdx::b16:: (bf16) builds of one source
#define HFN(bf, fn, ...) ((bf) ? gdx::b16::fn(__VA_ARGS__) : gdx::h16::fn(__VA_ARGS__))

int dev_alloc(std::vector<void*>& pool, void** p, size_t bytes);   // hipMalloc, recorded in pool
void free_pool(std::vector<void*>& pool);

// the fp32 GEMM dispatch every forward GEMM goes through: gemm2.hip where it takes the problem, else gemm.hip
int gemm(int om, int ep, const GemmParams& p, hipStream_t s, GemmCtl* ctl = nullptr);

// dst [npad][kpad] halves = src[r*src_ld + col0 + c] for r < n, c < k, zero elsewhere
int pack_f16_into(_Float16* dst, const float* src, int n, int src_ld, int col0, int k, int npad, int kpad, hipStream_t s,
                  bool bf = false);

// V2 front end (RoPE -> causal local attention -> RoPE at t+1) for compute dtype `dtype`: the one dispatch of the forwards and
// of the test entry point gdx_local_attention.  The 16-bit kernel (local_attention_half) reads xseq16 and writes enc16 plus the
// optional fp32 copy enc; otherwise the fp32 kernel (MFMA, or the scalar one for other head widths / windows) reads xseq and
// writes enc plus the optional 16-bit copy enc16.
bool local_attention_half(int dtype, int d, int heads, int window);
hipError_t launch_local_attention_any(int dtype, const float* xseq, const _Float16* xseq16, const float* cosT, const float* sinT,
                                      float* enc, _Float16* enc16, int B, int T, int d, int heads, int window, hipStream_t s);

// Average microseconds of `iters` calls of launch() after `warm` warm-up calls, between two events on s.  launch() returns 0,
// or -1 with the error recorded.  The events are destroyed on every path.
template <class F>
int time_launches(int warm, int iters, hipStream_t s, float* avg_us, F launch) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto timed = [&]() -> int {
        HIPCHK(hipEventCreate(&e0));
        HIPCHK(hipEventCreate(&e1));
        for (int i = 0; i < warm; ++i)
            if (launch()) return -1;
        HIPCHK(hipEventRecord(e0, s));
        for (int i = 0; i < iters; ++i)
            if (launch()) return -1;
        HIPCHK(hipEventRecord(e1, s));
        HIPCHK(hipEventSynchronize(e1));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, e0, e1));
        *avg_us = ms * 1000.0f / (float)iters;
        return 0;
    };
    const int rc = timed();
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    return rc;
}

// ---- the model handle ---------------------------------------------------------------------------------------------------
struct Packed {          // a Linear weight [n][k] packed to [npad][kpad] (+ bias [npad])
    float* w = nullptr;
    float* bias = nullptr;
    int n = 0, k = 0, npad = 0, kpad = 0;
    _Float16* w16 = nullptr;             // fp16 mode: [npad16][kpad16], rows padded to 256, K to 64 (gemmh.hip)
    int npad16 = 0, kpad16 = 0;          // 0 in the fp32 mode
    bool has_bias = false;               // a state-dict key supplies `bias`
    // n .. has_bias depend on the configuration only: describe_weights sets them, nothing else writes them
};

struct Layer {
    Packed qkv, out, ff1, ff2;
    float *g1 = nullptr, *b1 = nullptr, *g2 = nullptr, *b2 = nullptr;
};

// An activation buffer of the forward, fp32 side and 16-bit side: gdx_prepare allocates the sides the compute mode uses, the
// helpers of the per-step sequence (forward.hip: linear, attend, add_norm) pick the side they read and write
struct Act { float* f = nullptr; _Float16* h = nullptr; };

// One state-dict key of the handle's configuration: the shape it must have and the device buffers it becomes.  The handle's
// table of these (weights.hip: describe_weights) is the only list of the model's tensors: gdx_set_weight, the
// "missing weights" report and the packed image are all read off it.
struct WeightSlice { Packed* P; int col0; };   // P->w (and w16) = rows [0, P->n) x columns [col0, col0 + P->k) of the tensor
struct WeightSpec {
    enum Kind { LINEAR,    // a Linear weight: one Packed panel per slice
                BIAS,      // -> P->bias, zero padded to P->npad
                VECTOR,    // LayerNorm gamma / beta -> *vec, unpadded
                TABLE };   // positional / rotary table -> *vec; shape[0] is free and becomes the handle's row count
    Kind kind;
    std::string key;
    std::vector<int64_t> shape;
    std::vector<WeightSlice> slices;   // LINEAR
    Packed* P = nullptr;               // BIAS
    float** vec = nullptr;             // VECTOR, TABLE
    bool rotary = false;               // TABLE: counted by rope_rows (else pe_rows)
    int group = 0;                     // place in the "missing weights" report (the table itself is in packed-image order)
};

// Workspace the handle acquires after gdx_prepare, each buffer on first use (ws_need) by the call that needs it, with the host-side
// facts about that memory.  gdx_prepare frees the pool and resets all of this with ONE assignment: a new field needs no reset line.
struct LateWorkspace {
    float* temb_table = nullptr; int temb_table_rows = 0;   // step tables (loops.hip: build_step_tables), regrown for a longer loop
    float* c2t_table = nullptr; bool c2t_valid = false;     // V2: W_coa * temb_table rows (valid while c2t_valid)
    bool tables_valid = false;        // temb_table (and c2t_table) hold the rows of tmap_host under the current weights
    int64_t* tmap_dev = nullptr; std::vector<int64_t> tmap_host;
    float *bpd_xt = nullptr, *bpd_z = nullptr, *bpd_part = nullptr;   // gdx_bpd_loop: x_t, Philox noise [B, J, T], chunk sums
    // gdx_parallel_loop (B = window x samples): the window's predictions [B, J, T], the sweep's errors [B] and chunk sums, the scales
    // repeated per slot [B], and the model timestep of every slot the loop can reach, [steps + window][samples] (what pl_ts_host holds)
    float *pl_x0 = nullptr, *pl_scale = nullptr; double *pl_err = nullptr, *pl_part = nullptr;
    int64_t* pl_ts = nullptr; size_t pl_ts_cap = 0;
    std::vector<int64_t> pl_ts_host;
    double* rs_part = nullptr; float* rs_factor = nullptr;   // guidance rescale: chunk sums [B][chunks][4] and factors [B]
    float* gd = nullptr;              // guidance refresh: the stored difference c - u [B, J, T]
    bool gd_valid = false;            // ... holds a refresh call's difference under the current conditioning
    float* lc_delta = nullptr;        // layer cache: the stored change [2B, T, d]
    void* lc_in = nullptr;            // ... and the residual stream after layer lc_keep - 1 [2B, T+1, d] in the stream's element
                                      // type, kept until the end of a full call
    bool lc_valid = false;            // ... lc_delta holds a full call's change under the current conditioning,
    int lc_mode = 0;                  // ... stored by a call of this forward mode (GDX_COND / GDX_UNCOND / GDX_CFG)
    float* rp_tab = nullptr; int rp_tab_rows = 0;   // resampling: the device image of the handle's rp_rows, regrown for a longer schedule
    bool rp_tab_valid = false;        // ... holds the rows of the most recent gdx_set_resample
};

// What a guided call runs, by (compose mode, PAG kind): its row groups, whether it composes three passes, and the group that
// holds the all-dropped rows U.  The one table behind gdx_model::groups / three_pass / u_group.
struct GuideLayout { int groups; bool three; int u_group; };
constexpr GuideLayout GUIDE_LAYOUT[5][3] = {
    //  GDX_PAG_OFF      GDX_PAG_ONLY     GDX_PAG_CFG
    {{2, false, 1}, {2, false, 2}, {3, true, 2}},    // GDX_GUIDE_JOINT      (F, U)   | (F, P) + U | (F, P, U)
    {{2, false, 2}, {2, false, 2}, {2, false, 2}},   // GDX_GUIDE_TEXT       (F, S) + U
    {{2, false, 2}, {2, false, 2}, {2, false, 2}},   // GDX_GUIDE_SEED       (F, X) + U
    {{3, true, 2}, {3, true, 2}, {3, true, 2}},      // GDX_GUIDE_SEED_TEXT  (F, S, U)
    {{3, true, 2}, {3, true, 2}, {3, true, 2}},      // GDX_GUIDE_TEXT_SEED  (F, X, U)
};

}  // namespace gdx

struct gdx_model {
    gdx_config_t cfg;
    int d, J, ff, L, H;
    bool f16 = false;                 // reduced-precision mode (GDX_DTYPE_F16 or _BF16): 16-bit MFMA operands, fp32 accumulate
    bool bf16 = false;                // ... with bf16 elements (the gdx::b16 kernels)
    bool stream32 = false;            // 16-bit modes: the residual stream (x + sublayer(x), LayerNorm in / out) stays fp32 and
                                      // only the GEMM / attention operands are 16-bit copies (default for bf16, see add_norm)
    std::vector<gdx::WeightSpec> weights;   // describe_weights; points into this handle
    std::set<std::string> have;
    std::vector<std::string> required;
    std::vector<void*> allocs;        // weight allocations
    std::vector<void*> ws_allocs;     // workspace allocations
    gdx::Packed time0, time2, seed, in_x, in_mfcc, proj_pose, proj_audio, proj_coa, outp;
    gdx::Packed text;                 // cfg.text_dim > 0: embed_text [text_dim][clip_dim]; `seed` then has d - text_dim rows
    std::vector<gdx::Layer> layers;
    float* pe = nullptr; int pe_rows = 0;
    float *rope_cos = nullptr, *rope_sin = nullptr; int rope_rows = 0;
    // workspace (sized for G*B samples so that CFG runs as one batch of G row groups: 2, or 3 in a 3-pass compose mode)
    int B = 0, T = 0, S = 0;
    int G = 2;                        // row groups the workspace is prepared for (groups())
    long rows_alloc = 0;              // rows of the [G*B*S + pad] token buffers
    bool cond_set = false;
    int64_t guide_lo = INT64_MIN, guide_hi = INT64_MAX;   // gdx_set_guidance_interval: model timesteps that get guidance
    float guide_phi = 0.f;            // gdx_set_guidance_rescale: 0 = off
    int guide_compose = GDX_GUIDE_JOINT;   // gdx_set_guidance_compose: which passes a guided call contrasts (gdx.h)
    int guide_every = 1;              // gdx_set_guidance_refresh: the unconditional pass runs on every guide_every-th guided call
    int lc_every = 1, lc_keep = 0;    // gdx_set_layer_cache: every lc_every-th denoiser call of a loop is full; the calls between
                                      // run lc_keep layers and add the stored change of the deeper ones (1 = off)
    int rp_jump = 1, rp_repeats = 1, rp_steps = 0;   // gdx_set_resample: repeats = 1 is off; rp_steps = the schedule's length
    std::vector<float> rp_rows;       // ... host [rp_steps][2]: row l = (a, b) of the forward hop from level l to level l + rp_jump
    int64_t forward_samples = 0;     // gdx_forward_samples: samples pushed through forward_core since gdx_create
    int64_t forward_layer_samples = 0;   // gdx_forward_layer_samples: samples x encoder layers launched
    gdx::Act xa, xb, qkv, ctx, tmp, ffb;   // [rows_alloc] token rows: residual stream (xa, xb), sublayer operands and outputs
    gdx::Act xt, xc;                       // token-major pose in / compacted last layer, [2B*T + pad] rows
    gdx::Act emb, xseq;                    // V2 front end: InputProcess output, proj_pose output
    float* addend = nullptr;
    float *seed_cat = nullptr, *temb_in = nullptr, *temb_h = nullptr, *temb = nullptr, *coa = nullptr, *c2 = nullptr;
    float* x0 = nullptr;              // [G*B, J, T]
    float* x0t = nullptr;             // token-major x0
    int ldo = 0;                      // row stride of x0t = J rounded up to 64
    float* c2_seed = nullptr;         // V2: W_coa * seed_cat rows [3B, d]
    // guidance compose: the passes of a guided call are row groups F, then M (a 3-pass mode's middle pass, or the contrast of modes
    // 1 and 2), then U; JOINT has no M and keeps U in group 1
    // perturbed-attention guidance (gdx_set_attention_guidance) takes the place of M under JOINT: (F, P) with U kept in group 2 for
    // GDX_UNCOND, or (F, P, U); under another compose mode a guided call is refused (pag_conflict), and the mode's own layout stands
    int pag_kind = GDX_PAG_OFF;       // gdx_set_attention_guidance
    uint64_t pag_mask = 0;            // ... bit l: encoder layer l gives the rows of group P identity attention
    bool pag() const { return pag_kind != GDX_PAG_OFF && guide_compose == GDX_GUIDE_JOINT; }
    const gdx::GuideLayout& layout() const { return gdx::GUIDE_LAYOUT[guide_compose][pag_kind]; }
    bool three_pass() const { return layout().three; }
    int groups() const { return layout().groups; }
    int u_group() const { return layout().u_group; }   // where GDX_UNCOND finds the all-dropped rows
    // graph replay of launch-bound loops (gdx_sample_loop)
    bool graph_replay = false;        // gdx_set_graph_replay
    int* gstate = nullptr;            // device {schedule index, executed-step number}
    hipStream_t gstream = nullptr;    // capture needs a non-default stream (PyTorch's current stream is usually stream 0)
    hipEvent_t gev_in = nullptr, gev_out = nullptr;
    hipGraph_t ggraph = nullptr;
    hipGraphExec_t gexec = nullptr;
    bool prof = false;                // in-situ FFN-1 GEMM timing (gdx_profile_begin / gdx_profile_end)
    std::vector<hipEvent_t> prof_ev;  // pairs, recorded around each FFN-1 launch while prof is on
    size_t prof_used = 0;
    bool keep_taps = false;
    std::vector<float*> taps;         // [L+1] x [2B*S*d] when keep_taps
    bool guards = false;              // gdx_set_guards: every workspace allocation carries a canary zone behind it
    std::vector<std::pair<unsigned char*, size_t>> guard_zones;
    gdx::LateWorkspace late;
};

namespace gdx {
// weights.hip: fills h->weights, the dimensions of every Packed they name and h->required from h->cfg (gdx_create)
void describe_weights(gdx_model* h);

// handle.hip
// A workspace buffer of the handle, zero-filled on s, the stream of the call that asks, which orders the fill ahead of that call's
// first store; under gdx_set_guards with its canary zone behind it.  The only function that adds to h->ws_allocs.
int ws_alloc(gdx_model* h, void** p, size_t bytes, hipStream_t s);
// ... on first use: nothing to do once *p is set (the fields of h->late)
template <class T> int ws_need(gdx_model* h, T** p, size_t bytes, hipStream_t s) {
    return *p ? 0 : ws_alloc(h, (void**)p, bytes, s);
}
int check_ready(gdx_model* h, const char* who);                   // handle, gdx_prepare and a conditioning, or the refusal
int check_mode(const char* who, int mode, const float* scale);
// the refusal of a guided call of `who` under perturbed-attention guidance on a handle whose compose mode is not GDX_GUIDE_JOINT
int pag_conflict(const gdx_model* h, const char* who, int mode);
// the refusal of a loop `who` whose history does not survive a forward hop, while resampling is on (gdx_set_resample)
int refuse_resampling(const gdx_model* h, const char* who);

// forward.hip
struct ForwardOpts {
    const int* state = nullptr;   // graph replay: the row index of temb / c2t is read from device memory
    bool tm = false;              // token-major: the pose operand is in h->xt, the prediction stays in h->x0t
    int lc = LC_OFF;              // the call's part in the layer cache (gdx_call_plan.h)
};
int forward_core(gdx_model* h, const float* x, const float* temb, int tstride, const float* c2t, int mode, float* x0_out,
                 hipStream_t s, const ForwardOpts& o = {});
int time_embed(gdx_model* h, const int64_t* idx, int M, float* gathered, float* hidden, float* out, hipStream_t s);
// g != nullptr: the guided prediction is already formed (compose_x0) and u / scale are not read
int rescale_x0(gdx_model* h, const float* c, const float* u, const float* scale, const int64_t* t, float* out, hipStream_t s,
               const float* g = nullptr);
// a guided 3-pass call's prediction from the three thirds (F, M, U) of h->x0 and scale [2][B] (gdx.h gdx_set_guidance_compose),
// rescaled under the handle's phi > 0; guided where t == nullptr or lo <= t[b] <= hi, else F.  out may be the F third.
int compose_x0(gdx_model* h, const float* scale, const int64_t* t, float* out, hipStream_t s);
}  // namespace gdx
