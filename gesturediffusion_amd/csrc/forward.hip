// libgdx.so host side: the per-step kernel sequence of the denoiser (V1 = reference model/mdm_old.py:84-122, V2 =
// model/mdm.py:105-224; forward_core, once for the three compute modes on top of linear / attend / add_norm), the GEMM dispatch
// under it, and gdx_forward.  C ABI in include/gdx.h; the handle is in handle.hip, the loops that call forward_core in loops.hip.
#include "gdx_host.h"

#include <cstring>
#include <string>

using namespace gdx;

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

// Self-attention of samples b0 .. b0 + nb - 1 of the batch: qkv -> ctx on their rows.  Every attention kernel takes
// qkv [rows][3d] -> ctx [rows][d], so a sub-batch is a launch on offset pointers; the rows readable behind it shrink with the offset
static int attend(gdx_model* h, int b0, int nb, hipStream_t s) {
    const size_t r0 = (size_t)b0 * h->S, d = h->d;
    if (h->f16)
        HIPCHK(HFN(h->bf16, launch_attentionh, h->qkv.h + r0 * 3 * d, h->ctx.h + r0 * d, nb, h->S, h->H, h->d, h->rows_alloc - (long)r0, s));
    else if (attention3_supported(h->S, h->H, h->d))
        HIPCHK(launch_attention3(h->qkv.f + r0 * 3 * d, h->ctx.f + r0 * d, nb, h->S, h->H, h->d, s));
    else                                              // other head dims / more than 256 tokens: the general 32 x 32-block kernel
        HIPCHK(launch_attention(h->qkv.f + r0 * 3 * d, h->ctx.f + r0 * d, nb, h->S, h->H, h->d, s));
    return 0;
}

// Self-attention of a guided call's layer under perturbed-attention guidance (gdx.h gdx_set_attention_guidance), groups (F, P) or
// (F, P, U) of B samples: attention on the contiguous runs of unperturbed groups, the identity (ctx = V, a copy) on the rows of P
static int attend_perturbed(gdx_model* h, int Beff, hipStream_t s) {
    const int B = h->B;
    const size_t r0 = (size_t)B * h->S, d = h->d;
    if (attend(h, 0, B, s) || (Beff > 2 * B && attend(h, 2 * B, Beff - 2 * B, s))) return -1;
    if (h->f16) HIPCHK(launch_attention_identity(2, h->qkv.h + r0 * 3 * d, h->ctx.h + r0 * d, (long)r0, h->d, s));
    else HIPCHK(launch_attention_identity(4, h->qkv.f + r0 * 3 * d, h->ctx.f + r0 * d, (long)r0, h->d, s));
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
// lc (layer cache, gdx.h gdx_set_layer_cache; the loops' plan decides, gdx_call_plan.h): LC_FULL = today's forward, which also keeps
// the stream after layer lc_keep - 1 and stores the change of the deeper layers; LC_PARTIAL = layers 0 .. lc_keep - 1 only, the output
// GEMM's operand formed from their output plus the stored change.  LC_OFF issues exactly the launches of a handle without a cache.

// gdx_layer_delta on device buffers whose pairing is already one of the three: the fp32 instance, or the build of the 16-bit type
static int layer_delta(int op, int in_dtype, int out_dtype, int B, int T, int d, const void* in, void* outc, float* delta,
                       hipStream_t s) {
    if (out_dtype == GDX_DTYPE_F32) HIPCHK(launch_layer_delta(op, (const float*)in, (float*)outc, delta, B, T, d, s));
    else HIPCHK(HFN(out_dtype == GDX_DTYPE_BF16, launch_layer_delta_h, op, in_dtype == GDX_DTYPE_F32, in, (_Float16*)outc, delta, B, T, d, s));
    return 0;
}

int gdx::forward_core(gdx_model* h, const float* x, const float* temb, int tstride, const float* c2t, int mode, float* x0_out,
                      hipStream_t s, const ForwardOpts& o) {
    const auto [state, tm, lc] = o;
    const int B = h->B, T = h->T, S = h->S, d = h->d, J = h->J;
    const int Beff = mode == GDX_CFG ? h->groups() * B : B;      // guided: row groups F, U -- or F, M, U (gdx_set_guidance_compose)
    const int layers = lc == LC_PARTIAL ? h->lc_keep : h->L;     // encoder layers this call launches
    const uint64_t perturbed = mode == GDX_CFG && h->pag() ? h->pag_mask : 0;   // layers whose group P gets identity attention
    h->forward_samples += Beff;                                   // gdx_forward_samples (host side only)
    h->forward_layer_samples += (int64_t)Beff * layers;           // gdx_forward_layer_samples
    // layer cache: the residual stream is fp32 in the fp32 mode and under stream32, else the 16-bit type; the operand of the
    // output GEMM is fp32 in the fp32 mode only
    const bool res32 = !h->f16 || h->stream32;
    const int lc_in_dt = res32 ? GDX_DTYPE_F32 : h->cfg.compute_dtype, lc_out_dt = h->cfg.compute_dtype;
    const void* lc_stream = res32 ? (const void*)h->xa.f : (const void*)h->xa.h;
    void* lc_xc = h->f16 ? (void*)h->xc.h : (void*)h->xc.f;
    if (lc != LC_OFF) {
        if (lc == LC_PARTIAL && (!h->late.lc_valid || !h->late.lc_delta))
            return fail("forward_core: a partial call without a stored layer change");
        if (ws_need(h, &h->late.lc_delta, sizeof(float) * 2 * B * T * d, s) ||
            ws_need(h, &h->late.lc_in, 2 * (size_t)B * S * d * (res32 ? 4 : 2), s))
            return -1;
    }
    const size_t uncond_rows = (size_t)h->u_group() * B * d;     // GDX_UNCOND: the all-dropped rows U, wherever the mode keeps them
    const float* seed_emb = mode == GDX_UNCOND ? h->seed_cat + uncond_rows : h->seed_cat;
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
        const float* c2s = mode == GDX_UNCOND ? h->c2_seed + uncond_rows : h->c2_seed;
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
        if (linear(h, h->xa, ly.qkv, {.bias = ly.qkv.bias}, h->qkv, 3 * d, N, 3 * d, s)) return -1;
        if (perturbed >> l & 1 ? attend_perturbed(h, Beff, s) : attend(h, 0, Beff, s)) return -1;
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
            HIPCHK(hipMemcpyAsync(h->late.lc_in, lc_stream, (size_t)N * d * (res32 ? 4 : 2), hipMemcpyDeviceToDevice, s));
    }
    if (lc == LC_FULL) {                                          // change of layers lc_keep .. L-1 on the rows the output GEMM reads
        if (layer_delta(0, lc_in_dt, lc_out_dt, Beff, T, d, h->late.lc_in, lc_xc, h->late.lc_delta, s)) return -1;
        h->late.lc_valid = true; h->late.lc_mode = mode;
    }
    // partial call: the operand from this call's own shallow layers plus the stored change (a GDX_COND call under a stored
    // GDX_CFG reads the conditional rows, the first B)
    if (lc == LC_PARTIAL && layer_delta(1, lc_in_dt, lc_out_dt, Beff, T, d, lc_stream, lc_xc, h->late.lc_delta, s)) return -1;
    if (h->keep_taps) {                                           // tap L + 1: the output GEMM's operand, widened
        if (h->f16) HIPCHK(HFN(h->bf16, launch_convert_f32, h->xc.h, h->taps[h->L + 1], (int64_t)Beff * T * d, s));
        else HIPCHK(hipMemcpyAsync(h->taps[h->L + 1], h->xc.f, sizeof(float) * (size_t)Beff * T * d, hipMemcpyDeviceToDevice, s));
    }
    // OutputProcess (model/mdm.py:372-380): token-major fp32 GEMM, then the permute back to [B, J, 1, T]
    if (linear(h, h->xc, h->outp, {.bias = h->outp.bias}, Act{h->x0t, nullptr}, h->ldo, Beff * T, h->ldo, s)) return -1;
    if (!tm) HIPCHK(launch_transpose_out(h->x0t, x0_out, Beff, J, T, h->ldo, s));
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

// gdx_cfg_rescale on the handle's buffers: c, u -> out for the B samples of the workspace, guided where t == nullptr or
// lo <= t[b] <= hi.  The chunk sums and factors belong to the handle (first use allocates, gdx_prepare resets).
int gdx::rescale_x0(gdx_model* h, const float* c, const float* u, const float* scale, const int64_t* t, float* out, hipStream_t s,
                    const float* g) {
    const size_t chunks = bpd_chunks((long)h->J * h->T);
    if (ws_need(h, &h->late.rs_part, sizeof(double) * 4 * h->B * chunks, s) || ws_need(h, &h->late.rs_factor, sizeof(float) * h->B, s))
        return -1;
    gdx_cfg_rescale_args_t r;
    memset(&r, 0, sizeof(r));
    r.batch = h->B; r.njoints = h->J; r.frames = h->T;
    r.x0_cond = c; r.x0_uncond = u; r.scale = scale; r.phi = h->guide_phi;
    r.t = t; r.lo = h->guide_lo; r.hi = h->guide_hi;
    r.workspace = h->late.rs_part; r.factor = h->late.rs_factor; r.out = out;
    return gdx_cfg_rescale_(&r, g, (void*)s);
}

// With phi > 0 the composed prediction is formed in the M third, which nothing reads afterwards, and the rescale reads c = F beside it
int gdx::compose_x0(gdx_model* h, const float* scale, const int64_t* t, float* out, hipStream_t s) {
    const int64_t per = (int64_t)h->J * h->T;
    const size_t n = (size_t)h->B * per;
    float *F = h->x0, *M = F + n, *U = M + n;
    const bool rescale = h->guide_phi > 0.0f;
    HIPCHK(launch_cfg_compose(F, M, U, scale, scale + h->B, t, h->guide_lo, h->guide_hi, rescale ? M : out, h->B, per, s,
                              h->pag() ? COMPOSE_PAG : COMPOSE_CHAIN));
    return rescale ? rescale_x0(h, F, nullptr, nullptr, t, out, s, M) : 0;
}

// timestep embedding rows for idx[M] (model/mdm.py:296-310): pe gather -> Linear -> SiLU -> Linear.  The same
// row-independent kernel serves the per-sample rows of gdx_forward and the whole-loop table of gdx_sample_loop, so a
// timestep's embedding has the same bits on both sides of the seam (fused loop == step-wise protocol, bit for bit).
int gdx::time_embed(gdx_model* h, const int64_t* idx, int M, float* gathered, float* hidden, float* out, hipStream_t s) {
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
    if (check_mode("gdx_forward", mode, scale) || pag_conflict(h, "gdx_forward", mode)) return -1;
    const bool three = mode == GDX_CFG && h->three_pass();
    if (three && h->B > 65535) return fail("gdx_forward: batch exceeds 65535 (3-pass guidance)");
    hipStream_t s = (hipStream_t)stream;
    if (time_embed(h, timesteps, h->B, h->temb_in, h->temb_h, h->temb, s)) return -1;
    const float* c2t = nullptr;
    if (h->cfg.arch == GDX_ARCH_MDM) {       // W_coa * temb per sample (h->coa doubles as the [B, d] buffer for it)
        HIPCHK(launch_small_linear(h->temb, h->d, h->proj_coa.w, h->proj_coa.kpad, nullptr, h->coa, h->d, h->B, h->d, h->d, 0, s));
        c2t = h->coa;
    }
    if (mode != GDX_CFG) return forward_core(h, x, h->temb, h->d, c2t, mode, out, s);
    if (forward_core(h, x, h->temb, h->d, c2t, mode, h->x0, s)) return -1;
    if (three) return compose_x0(h, scale, timesteps, out, s);
    const int64_t per = (int64_t)h->J * h->T;
    // the timesteps are on the device: the double batch stays, the blend selects per sample (guided: blend, else c)
    if (h->guide_phi > 0.0f) return rescale_x0(h, h->x0, h->x0 + (size_t)h->B * per, scale, timesteps, out, s);
    HIPCHK(launch_cfg_blend(h->x0, h->x0 + (size_t)h->B * per, scale, timesteps, h->guide_lo, h->guide_hi, out, h->B, per, s));
    return 0;
}
