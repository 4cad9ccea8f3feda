// Internal launcher declarations shared by the libgdx.so translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gdx.h"

// The reduced-precision mode exists for two 16-bit element types: fp16 (GDX_DTYPE_F16) and bf16 (GDX_DTYPE_BF16).  The kernel
// files whose kernels read or write half elements (the Makefile's HALF_SRCS: exactly the files that mention half_t) are compiled
// twice; the second time with -DGDX_BF16, which makes `half_t` = __bf16 and puts everything they define into namespace gdx::b16
// instead of the inline namespace gdx::h16 (so the fp16 / fp32 build keeps its plain gdx:: names).  A file of fp32-only kernels
// is compiled once, into plain gdx::.  Across translation units a half buffer is always passed as `_Float16*` -- an opaque
// 16-bit element pointer; only the kernels know which of the two formats the bits are.
#ifdef GDX_BF16
#define GDX_HNS_BEGIN namespace b16 {
#define GDX_HNS_NAME b16          // for calls between functions of the half API (an unqualified call would also find the
#else                             // gdx:: instance through the argument's namespace)
#define GDX_HNS_BEGIN inline namespace h16 {
#define GDX_HNS_NAME h16
#endif
#define GDX_HNS_END }

namespace gdx {

#ifdef GDX_BF16
typedef __bf16 half_t;
#else
typedef _Float16 half_t;
#endif

// Rows every token-major workspace buffer carries beyond its last logical row (include/gdx.h): the persistent GEMM
// (gemm2.hip) reads and stores WHOLE tiles, the attention kernels read whole K/V tiles.  Must be >= the tallest tile.
constexpr int ROW_PAD = GDX_ROW_PAD;

// ---- GEMM (gemm.hip) ---------------------------------------------------------------------
// C = A * W^T (+ epilogue).  W is a packed weight [Npad][ldw], K-contiguous, zero padded to
// multiples of 128 rows / 32 columns, so the weight operand never needs a bounds check.
// Instantiated (gemm.hip GDX_GEMM_INSTANCES): OUT_ROWS under each Epi and OUT_TOKROWS under EPI_RES.  A[m][k] = A[m*lda + k].
enum OutMode { OUT_ROWS = 0,      // C[m*ldc + n]
               OUT_TOKROWS = 1 };  // C[(m + m/T + 1)*ldc + n]   (frames into [B, T+1, d], token 0 skipped)
enum Epi { EPI_BIAS = 0,      // + bias[n]
           EPI_GELU = 1,      // gelu_erf(. + bias[n])
           EPI_RES = 2,       // + bias[n] + R[row_out*ldr + n]
           EPI_RES_VEC = 3 }; // + R[row_out*ldr + n] + V[(m/T)*ldv + n]

struct GemmParams {
    const float* A; int lda;
    const float* W; int ldw;
    const float* bias;
    const float* R; int ldr;
    const float* V; int ldv;
    float* C; int ldc;
    int M, N, K;   // K: multiple of 32
    int T;         // frames per sample, for the row maps
};

// Which kernel a launch takes depends on the problem and the environment only.  What a test or bench entry point (testapi.hip)
// wants beyond that travels in an optional control argument of the launchers; the forwards pass none.
// What an fp32 GEMM launch ran, filled in where the launch is decided (launch_gemm / launch_cfg): file 1 = gemm2.hip,
// 2 = gemm.hip; for gemm2.hip the tile shape (mb, nbw, bk), its LDS ring depth and whether it was the RESP instantiation
struct GemmLaunched { int file, mb, nbw, bk, nst, resp; };
struct GemmCtl {
    int file = 0;                          // 0 = the dispatch of gemm(), 1 = gemm2.hip or an error, 2 = gemm.hip
    int mb = 0, nbw = 0, bk = 0;           // gemm2.hip tile to force (wins over GDX_GEMM_TILE); 0 = none
    unsigned long long* stamps = nullptr;  // 512-byte device buffer for the in-kernel stamps of gemm2.hip (GDX_GEMM_DEBUG)
    GemmLaunched ran = {0, 0, 0, 0, 0, 0}; // out
};

hipError_t gemm_init();   // raises the dynamic-LDS limit of every instantiation
hipError_t launch_gemm(int omode, int epi, const GemmParams& p, hipStream_t s, GemmCtl* ctl = nullptr);

// persistent wave-specialised variant (gemm2.hip)
bool gemm2_supported(int omode, int epi, const GemmParams& p);
hipError_t launch_gemm2(int omode, int epi, const GemmParams& p, hipStream_t s, GemmCtl* ctl = nullptr);

// fp16-input / fp32-accumulate persistent GEMM of the reduced-precision mode (gemmh.hip):
//   C[row_out][n] = act( sum_k A[m][k] W[n][k] + bias[n] + R[row_out][n] + V[m / T][n] ),  row_out = rowmap ? m + m/T + 1 : m
// What a launch_gemmh ran: the tile of the first launch (mb == 16: the eight-wave kernel), the rows of the row cut's main part
// (0: no cut) and the tile of the tail launch
struct GemmHLaunched { int mb, nbw, main_rows, tail_mb, tail_nbw; };
struct GemmHCtl {
    int mb = -1, nbw = -1;                 // tile to force; (0, 0) = the cost model with its row cut, GDX_GEMMH_TILE ignored;
                                           // negative = no say (GDX_GEMMH_TILE, else the cost model)
    unsigned long long* stamps = nullptr;  // 512-byte device buffer for the in-kernel stamps (GDX_GEMM_DEBUG)
    GemmHLaunched ran = {0, 0, 0, 0, 0};   // out
};

struct GemmHParams {
    const _Float16* A; int lda;      // [M][K] halves, K % 64 == 0
    const _Float16* W; int ldw;      // packed weight, rows padded to a multiple of 256
    int a_bytes, w_bytes;            // exact extents for the buffer descriptors (reads past them return 0)
    const float* bias;               // [N] or nullptr
    const float* R; int ldr;         // fp32 per-output-row term or nullptr
    const float* V; int ldv;         // fp32 per-sample vector or nullptr
    float* C32; int ldc32;           // fp32 output or nullptr
    _Float16* C16; int ldc16;        // fp16 output or nullptr
    int M, N, K, T;
    int rowmap, gelu;
};
// ---- attention (attention.hip) -----------------------------------------------------------
// qkv [B*S][3d] (q | k | v, heads contiguous inside each), ctx [B*S][d]
hipError_t launch_attention(const float* qkv, float* ctx, int B, int S, int H, int d, hipStream_t s);
// the encoder head widths with a self-attention kernel in every compute mode (attention.hip, attentionh.hip)
inline bool head_dim_supported(int hd) { return hd == 32 || hd == 64 || hd == 96 || hd == 128 || hd == 192 || hd == 256; }
#define GDX_HEAD_DIMS "32, 64, 96, 128, 192 or 256"
// identity attention (perturbed-attention guidance): ctx [rows][d] = the V third of qkv [rows][3d], a bit copy of elem_bytes (2 or
// 4) wide elements in 16-byte units; d * elem_bytes % 16 == 0 and both pointers 16-byte aligned
hipError_t launch_attention_identity(int elem_bytes, const void* qkv, void* ctx, long rows, int d, hipStream_t s);

// eight-wave single-pass variant with the last query block shared out over four waves (attention3.hip); needs 64
// readable rows past the last sample
bool attention3_supported(int S, int H, int d);
// grid > 0: the persistent variant on that many workgroups (default: chosen from the item count); launched (optional, 3
// entries) receives what ran: 3 (item-resident) or 5 (persistent), the grid, the (sample, head) item count
hipError_t launch_attention3(const float* qkv, float* ctx, int B, int S, int H, int d, hipStream_t s, int grid = 0,
                             int* launched = nullptr);

// ---- fp32-only boundary kernels (boundary.hip) ----------------------------------------------
hipError_t launch_transpose_in(const float* x, float* xt, int B, int Bsrc, int J, int T, int ldx, hipStream_t s);
hipError_t launch_transpose_out(const float* yt, float* y, int B, int J, int T, int ldy, hipStream_t s);
// out[m][n] = act(sum_k A[m*lda+k] * W[n*ldw+k] + bias[n]);  act: 0 none, 1 SiLU.  K arbitrary.
hipError_t launch_small_linear(const float* A, int lda, const float* W, int ldw, const float* bias, float* out, int ldo,
                               int M, int N, int K, int act, hipStream_t s);
// out[m][:] = table[idx[m]][:]   (timestep -> sinusoidal row gather)
hipError_t launch_gather_rows(const float* table, const int64_t* idx, float* out, int M, int d, int max_rows, hipStream_t s);
// out[(b*rps + t + off)*d + n] = sum_c mfcc[((b%Bsrc)*C + c)*T + t] * W[n*ldw + c] + bias[n] (+ pe[(t+1)*d + n] if pe)
hipError_t launch_mfcc_project(const float* mfcc, const float* W, int ldw, const float* bias, const float* pe, float* out,
                               int B, int Bsrc, int C, int T, int d, int rps, int off, hipStream_t s);
// layer cache (gdx_layer_delta.h), fp32 stream and operand: op 0 delta = outc - in rows (b, t+1), op 1 outc = in rows + delta
hipError_t launch_layer_delta(int op, const float* in, float* outc, float* delta, int B, int T, int d, hipStream_t s);

// ---- MFCC front end pieces (mfcc.hip); the two transforms in between run on the persistent GEMM (mfcc.hip: gdx_mfcc) ----
hipError_t launch_mfcc_frames(const float* x, long n, float* frames, int numframes, int frame_len, int frame_step, int ldf,
                              float preemph, hipStream_t s);
hipError_t launch_mfcc_power(const float* spec, int lds, int im_off, float* pw, int ldp, float* energy, int numframes,
                             int nbins, int nfft, hipStream_t s);
hipError_t launch_mfcc_cepstrum(const float* mel, int ldm, const float* energy, const float* dct, const float* lift,
                                const float* mean, const float* stdv, float* out, int numframes, int nfilt, int numcep,
                                hipStream_t s);

// true when launch_local_attention (frontend.hip) takes the fp32 MFMA kernel (else the scalar one)
inline bool local_attention_mfma_supported(int d, int heads, int window) {
    const int e = d / heads;
    return (e == 32 || e == 64 || e == 128) && window >= 1 && window <= 16 && d % 4 == 0;
}

// ---- everything below exists once per half type (see the top of this file): gdx::X is the fp16 / fp32 build, gdx::b16::X
//      the bf16 build of the same source (gemmh.hip, attentionh.hip, norm.hip, frontend.hip, boundaryh.hip).  Only launchers
//      whose kernels read or write half_t belong here; a launcher of fp32-only kernels is declared once, above.
#define GDX_HALF_API                                                                                                        \
    bool gemmh_supported(const GemmHParams& p);                                                                             \
    hipError_t launch_gemmh(const GemmHParams& p, hipStream_t s, GemmHCtl* ctl = nullptr);                                  \
    /* reduced-precision attention (attentionh.hip): qkv / ctx in halves, head_dim 32/64/96/128/192/256, any S; qkv_rows = readable rows */ \
    bool attentionh_supported(int S, int H, int d);                                                                         \
    /* true where the 8 x 2 and persistent kernels (2, 3) are instantiated: head_dim 64/128/256 */                          \
    bool attentionh_multiblock(int hd);                                                                                     \
    hipError_t launch_attentionh(const _Float16* qkv, _Float16* ctx, int B, int S, int H, int d, long qkv_rows, hipStream_t s); \
    /* the same dispatch with a forced kernel (0 = the forward's choice, 1 = h8, 2 = h8q, 3 = h8p), the persistent grid      \
       (0 = its default), a report of what ran (launched: kernel, grid, work items) and a 512-byte device buffer for the     \
       in-kernel stamps of h8p (GDX_GEMM_DEBUG); used by gdx_attention_half and gdx_bench_attention.  Inside: ah_plan gives   \
       the (chunks, items, grid) of the kernel choice for the launch and for the report, one head-width ladder reaches the  \
       one launcher template launch_ah<KERNEL, HD> */                                                                       \
    hipError_t launch_attentionh_kernel(const _Float16* qkv, _Float16* ctx, int B, int S, int H, int d, long qkv_rows,     \
                                        int kernel, int grid, int* launched, hipStream_t s,                                \
                                        unsigned long long* stamps = nullptr);                                              \
    /* norm.hip: out = LayerNorm(x + res) (res may be nullptr); compact_S > 0: rows are [B, S] tokens and token 0 of every  \
       sample is dropped from the output ([B, S-1, d]); out (fp32) and out16 (half copy) are each optional */               \
    hipError_t launch_layernorm(const float* x, const float* res, const float* gamma, const float* beta, float* out,        \
                                _Float16* out16, int rows, int d, int compact_S, hipStream_t s);                            \
    /* half-mode LayerNorm: out16 = LN(x + res) with half x / res (res may be nullptr), fp32 statistics; out32 optional */  \
    hipError_t launch_layernorm_f16(const _Float16* x, const _Float16* res, const float* gamma, const float* beta,          \
                                    _Float16* out16, float* out32, int rows, int d, int compact_S, hipStream_t s);          \
    /* boundaryh.hip: launch_transpose_in with a half operand as its output */                                              \
    hipError_t launch_transpose_in_f16(const float* x, _Float16* xt, int B, int Bsrc, int J, int T, int ldx, hipStream_t s); \
    /* token 0 of the encoder input: enc[b*S*d + n] = temb[(b%Bsrc)*tstride + n] + seed[b*d + n] (+ pe0[n]).                \
       c2 != nullptr (V2): c2[b*d+n] = c2t[(b%Bsrc)*tstride + n] + c2_seed[b*d+n] -- the coarse slice of project_to_lat     \
       applied to (temb + seed_emb), split into its timestep half (c2t = W_coa temb rows, same stride as temb) and its seed \
       half (per conditioning) instead of a [B,d] x [d,d] linear per step */                                                \
    hipError_t launch_token0(const float* temb, int tstride, const float* seed_emb, const float* pe0, float* enc,           \
                             _Float16* enc16, const float* c2t, const float* c2_seed, float* c2, const int* state, int B,   \
                             int Bsrc, int S, int d, hipStream_t s);                                                        \
    /* launch_layer_delta with a half operand outc; in: the half stream, or (in32) the fp32 one */                          \
    hipError_t launch_layer_delta_h(int op, bool in32, const void* in, _Float16* outc, float* delta, int B, int T, int d,   \
                                    hipStream_t s);                                                                         \
    /* dst[i] = (half) src[i] and back */                                                                                   \
    hipError_t launch_convert_f16(const float* src, _Float16* dst, int64_t n, hipStream_t s);                               \
    hipError_t launch_convert_f32(const _Float16* src, float* dst, int64_t n, hipStream_t s);                               \
    /* frontend.hip, V2 front end: RoPE -> causal local attention (window, look back one window) -> RoPE at pos+1, written  \
       into enc[b][t+1][:].   xseq [B*T][d];  cos/sin tables [>=T+1][e/2], e = d/heads. */                                  \
    hipError_t launch_local_attention(const float* xseq, const float* cosT, const float* sinT, float* enc, _Float16* enc16, \
                                      int B, int T, int d, int heads, int window, hipStream_t s);                           \
    /* half-mode V2 front end on the 16-bit MFMA (d / heads in {64, 128}); xseq in halves; enc32 optional (parity taps) */   \
    bool local_attention_f16_supported(int d, int heads, int window);                                                       \
    hipError_t launch_local_attention_f16(const _Float16* xseq, const float* cosT, const float* sinT, _Float16* enc16,      \
                                          float* enc32, int B, int T, int d, int heads, int window, hipStream_t s);

inline namespace h16 { GDX_HALF_API }
namespace b16 { GDX_HALF_API }

// ---- the pose-layout files (fp32 only, contraction off: gdx_pose_device.h) -----------------
// chunks of GDX_BPD_CHUNK elements per sample: the blocks per sample of every chunked sum (gdx_bpd_terms, gdx_cfg_rescale,
// gdx_window_sweep) and the unit their workspaces are sized in
inline long bpd_chunks(long per_sample) { return (per_sample + GDX_BPD_CHUNK - 1) / GDX_BPD_CHUNK; }

// sampler.hip.  Graph replay of the sampling loop: device-resident {schedule index, executed-step number}
hipError_t launch_set_state(int* st, int idx, int k, hipStream_t s);
hipError_t launch_advance_state(int* st, hipStream_t s);
// guidance.hip.  out = u + scale[b]*(c - u) where lo <= t[b] <= hi (the handle's guidance interval), else c
hipError_t launch_cfg_blend(const float* c, const float* u, const float* scale, const int64_t* t, int64_t lo, int64_t hi,
                            float* out, int B, int64_t per_sample, hipStream_t s);

// out = g1 + s1[b]*(f - m) with g1 = u + s0[b]*(m - u) where t == nullptr or lo <= t[b] <= hi, else f (gdx_set_guidance_compose's
// 3-pass rule); rule = COMPOSE_PAG: g1 = u + s0[b]*(f - u) instead (gdx_set_attention_guidance's GDX_PAG_CFG, m = the perturbed
// pass); grid.y = sample, so B <= 65535; out may alias f, m or u
enum ComposeRule { COMPOSE_CHAIN = 0, COMPOSE_PAG = 1 };
hipError_t launch_cfg_compose(const float* f, const float* m, const float* u, const float* s0, const float* s1, const int64_t* t,
                              int64_t lo, int64_t hi, float* out, int B, int64_t per_sample, hipStream_t s, int rule = COMPOSE_CHAIN);

// argument of update_tm_kernel (sampler.hip): one step of gdx_sample_loop's token-major fast path, filled by loops.hip
struct UpdateTmDev {
    int kind, B, J, T, ldx, ldo;
    const float* coef; int step_index;
    float* xt;              // [Beff*T][ldx] in / out
    const float* x0t;       // [Beff*T][ldo]
    const float* scale;     // [B] or nullptr: guidance on (Beff = 2B)
    int const_noise;
    uint64_t seed, sample_offset;
    uint32_t rng_step;
    int clip;
    float* out_pose;        // [B][J][T] or nullptr (last step)
    void* xt16;             // half modes: the input GEMM's 16-bit operand [Beff*T][ldx], written beside the fp32 state
    int half_dtype;         // GDX_DTYPE_F16 or GDX_DTYPE_BF16 (the element type of xt16)
    const float* noise;     // this step's slice of a noise tape, reference layout [B or 1][J][T], or nullptr (Philox)
    int mirror;             // an unguided step (scale == nullptr) of a guided loop: write the uncond half of xt / xt16 as well
};

// operands of gdx_ddim_reverse_step (gdx.h), under the field names every pose-layout step struct uses: what step_begin / step_src
// (gdx_pose_host.h) and step_args (loops.hip) read.  The public entry takes them as plain arguments and fills this.
struct DdimReverseStepArgs {
    int32_t batch, njoints, frames;
    const float* coef;
    const int64_t* t;
    int32_t step_index;
    const float *x, *x0_cond, *x0_uncond, *scale;
    const uint8_t* inpaint_mask;
    const float* inpaint_motion;
    int32_t clip_denoised;
    float *out, *pred_out, *eps_out;
};

}  // namespace gdx

// the loops' (loops.hip) private entries into the pose-layout files; each returns 0, or -1 with the error recorded
// sampler.hip.  The update of a captured step: schedule index / step number read from `state` (UpdateDev::state)
int gdx_sampler_update_state_(const gdx_update_args_t* a, const int* state, long noise_stride, void* stream);
// one step of the token-major fast path of gdx_sample_loop (update_tm_kernel); checks the layout arguments of `d`
int gdx_sampler_update_tm_(const gdx::UpdateTmDev& d, void* stream);
// gdx_ddim_reverse_step on its operands as a struct (gdx_ddim_reverse_loop builds them with step_args)
int gdx_ddim_reverse_step_(const gdx::DdimReverseStepArgs& a, void* stream);
// gdx_parallel_loop: the window's planes [W + 1][plane] slid down by `stride` planes, the tail filled with P_W (window_slide_kernel)
int gdx_window_slide_(float* planes, long plane, int W, int stride, void* stream);
// gdx_sample_loop under gdx_set_resample: one forward hop x <- a*x + b*z in place, (a, b) = row `row` of tab [rows][2], z = noise
// [batch][per_sample] or the Philox draw rng_step (renoise_kernel)
int gdx_renoise_(float* x, const float* tab, int row, int batch, long per_sample, const float* noise, uint64_t seed,
                 uint64_t sample_offset, uint32_t rng_step, void* stream);
// bound.hip.  gdx_bpd_loop: x_t and the stored Philox noise of one step (bpd_xt_kernel)
int gdx_bpd_xt_(const float* x0, const float* coef, int idx, int batch, long per_sample, uint64_t seed, uint64_t sample_offset,
                uint32_t step, float* z_out, float* xt_out, void* stream);
// guidance.hip.  gdx_cfg_rescale with the guided prediction g given instead of blended from (x0_uncond, scale), which may then be NULL
int gdx_cfg_rescale_(const gdx_cfg_rescale_args_t* a, const float* g, void* stream);
// records the text of gdx_last_error and returns -1 (handle.hip), for the files that do not include gdx_host.h
extern "C" int gdx_set_error_(const char* msg);
