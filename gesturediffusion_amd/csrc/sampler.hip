// Fused reverse-process update over the pose tensor [B, J, 1, T] (HBM-bound, float4 streaming):
// classifier-free-guidance blend + inpainting blend + posterior mean / DDIM step + Gaussian noise
// (noise tape or in-kernel Philox4x32-10) in ONE pass, and the other step kernels on StepSrc (PLMS, DPM-Solver++, UniPC, DDIM
// inversion, the parallel-in-time window sweep), q_sample, randn and the generated chunk's de-normalisation.
//
// Replaces the 6-10 separate elementwise torch kernels and 6-10 host->device table copies per step of
// reference diffusion/gaussian_diffusion.py:307-311 (inpainting), :253-275 (posterior mean),
// :524-548 (p_sample), :748-782 (ddim_sample), :1595-1608 (_extract_into_tensor) and
// model/cfg_sampler.py:28.  Products and sums are rounded separately (__fmul_rn/__fadd_rn, never
// contracted into FMA) in the reference's operation order, so given the same x0 / x / noise the
// result is bit-identical to the torch expression.  Algorithmic bytes per element: read x, x0 (+ x0_u,
// + tape noise), write x_{t-1}  ->  12-20 B.
// Contraction is off in this file: see gdx_pose_device.h, which holds the generator, the group accessors and the shared formulas.
#include <algorithm>

#include "gdx_pose_device.h"
#include "gdx_pose_host.h"

namespace gdx {

// eps' of plms_sample (:1053-1066) from the newest eps and the history e1 (newest) .. e3:
//   kind 1: eps   2: (3 eps - e1)/2   3: (23 eps - 16 e1 + 5 e2)/12   4: (55 eps - 59 e1 + 37 e2 - 9 e3)/24
//   kind 5: (e1 + eps)/2, the improved-Euler corrector (:1052; e1 = the first forward's eps, eps = eps_2).  Operand order of
//           plms_step_kernel; plms_kernel used to write (e0 + e1), the same sum with the operands exchanged (same bits)
__device__ __forceinline__ float plms_combine(int kind, float eps, float e1, float e2, float e3) {
    if (kind == 1) return eps;
    float num, den = 2.0f;
    if (kind == 2) num = __fsub_rn(__fmul_rn(3.0f, eps), e1);
    else if (kind == 3) { num = __fadd_rn(__fsub_rn(__fmul_rn(23.0f, eps), __fmul_rn(16.0f, e1)), __fmul_rn(5.0f, e2)); den = 12.0f; }
    else if (kind == 4) {
        num = __fsub_rn(__fadd_rn(__fsub_rn(__fmul_rn(55.0f, eps), __fmul_rn(59.0f, e1)), __fmul_rn(37.0f, e2)), __fmul_rn(9.0f, e3));
        den = 24.0f;
    } else num = __fadd_rn(e1, eps);
    return __fdiv_rn(num, den);
}
// pred' = c0*x - c1*eps';  (pred'*c2 + c3*eps')*nz + keep*(1 - nz), nz = c[7] = (t != 0); keep = the step's pred_xstart (:1067-1078)
__device__ __forceinline__ float plms_tail(const float* c, float x, float ep, float keep) {
    const float pred = xstart_from_eps(c[0], c[1], x, ep);
    const float mean = ddim_mean(c[2], c[3], pred, ep);
    const float nz = c[7];
    return __fadd_rn(__fmul_rn(mean, nz), __fmul_rn(keep, __fsub_rn(1.0f, nz)));
}

// DPM-Solver++ multistep update in the data-prediction form (Lu et al. 2022, arXiv:2211.01095, Algorithm 2 and its third-order
// extension; gdx.h gdx_dpm_step): a*x + (w0*m0 [+ w1*m1 [+ w2*m2]]) with m0 this step's x0 prediction and m1 / m2 the two
// before it.  Every order is linear in the predictions, so the host collects the weights in fp64 and rounds them once; NH =
// history terms read, w = the row's columns of the launched order.
template <int NH>
__device__ __forceinline__ float dpm_multistep(float a, const float* w, float x, float m0, float m1, float m2) {
    float d = __fmul_rn(w[0], m0);
    if (NH >= 1) d = __fadd_rn(d, __fmul_rn(w[1], m1));
    if (NH >= 2) d = __fadd_rn(d, __fmul_rn(w[2], m2));
    return __fadd_rn(__fmul_rn(a, x), d);
}
// SDE-DPM-Solver++ (gdx.h gdx_dpm_sde_step): the multistep update with the row's noise scale s times a standard normal z added
// last, (a*x + D) + s*z.
template <int NH>
__device__ __forceinline__ float dpm_sde_multistep(float a, const float* w, float s, float x, float m0, float m1, float z) {
    return __fadd_rn(dpm_multistep<NH>(a, w, x, m0, m1, 0.f), __fmul_rn(s, z));
}

struct UpdateDev {
    StepSrc s;
    int kind, batch;
    const float* noise;
    int const_noise;
    uint64_t seed, sample_offset;
    uint32_t rng_step;
    // graph replay (gdx_sample_loop): when `state` is set the step-dependent values come from device memory, so one
    // captured step can be replayed for every step: state[0] = schedule index, state[1] = executed-step number k
    // (rng_step = k + 1, noise = noise + k * noise_stride)
    const int* state;
    long noise_stride;
    // cond_fn guidance (reference :418-494): gradient tensor and, for DDIM, the per-step sqrt(1 - alpha_bar) table
    const float* grad;
    const float* gcoef;
};

template <bool VEC>
__global__ __launch_bounds__(256) void update_kernel(const UpdateDev a) {
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= a.s.groups * a.batch) return;
    const Group g = group_of<VEC>(gid, a.s.groups, a.s.per_sample);
    const long idx = a.state ? a.state[0] : coef_row(a.s, g.b);
    const float* c = a.s.coef + idx * 8;
    const uint32_t rng_step = a.state ? (uint32_t)a.state[1] + 1u : a.rng_step;
    const float* noise = a.noise && a.state ? a.noise + (long)a.state[1] * a.noise_stride : a.noise;

    const f32x4 x = load4<VEC>(a.s.x, g.e0, g.nval);
    const f32x4 x0 = pred_xstart4<VEC>(a.s, g);
    const f32x4 z = noise ? load4<VEC>(noise, a.const_noise ? 4L * g.grp : g.e0, g.nval)
                          : philox_normal4(a.seed, a.const_noise ? 0ull : a.sample_offset + (uint64_t)g.b, rng_step, g.grp);
    const bool cond = a.grad != nullptr;
    const f32x4 grad = cond ? load4<VEC>(a.grad, g.e0, g.nval) : f32x4{0.f, 0.f, 0.f, 0.f};
    const float s1m = cond && a.kind != GDX_SAMPLER_P ? a.gcoef[idx] : 0.0f;
    f32x4 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = update_value(a.kind, c, x[i], x0[i], z[i], cond, grad[i], s1m);
    store4<VEC>(a.s.out, g.e0, g.nval, r);
    if (a.s.pred) store4<VEC>(a.s.pred, g.e0, g.nval, x0);
}

// ---------------------------------------------------------------------------------------------------------------
// The same update on a TOKEN-MAJOR loop state (gdx_sample_loop's fast path: in-kernel Philox noise, no inpainting, no
// dumps, T % 4 == 0).  Between two steps the pose tensor only ever feeds the input GEMM, which wants it token-major
// ([Beff*T][ldx], row = b*T + t), and the denoiser's output leaves the output GEMM token-major ([Beff*T][ldo]); kept in
// the reference's [B, J, 1, T] layout it is transposed twice per step for nothing.  Here the state IS the token-major
// operand: this kernel reads x_t and x0 (cond / uncond halves) token-major and writes x_{t-1} token-major in place
// (both halves under guidance: the same x feeds both passes), plus, on the last step, the sample in the reference
// layout.  A thread owns a 4 (frames) x 4 (channels) micro-tile: for channel j the four frames t0..t0+3 are exactly
// Philox group j*T/4 + t0/4 of the pose-layout numbering, so every element gets the very noise value -- and, through
// update_value(), the very arithmetic -- of update_kernel: the two paths are bit-identical.  (UpdateTmDev: gdx_internal.h)
// An unguided step of a guided loop (guidance interval) has no scale: x0 is the cond half alone (the denoiser ran B samples),
// and `mirror` makes it write the uncond half of the state all the same, for the guided step that follows.
__global__ __launch_bounds__(256) void update_tm_kernel(const UpdateTmDev a) {
    const int jq_n = (a.J + 3) / 4, tq_n = a.T / 4;
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (long)a.B * tq_n * jq_n) return;
    const int jq = gid % jq_n;
    const long bt = gid / jq_n;
    const int tq = bt % tq_n, b = bt / tq_n;
    const int j0 = 4 * jq, t0 = 4 * tq;
    const float* c = a.coef + (long)a.step_index * 8;
    const long row0 = (long)b * a.T + t0;                        // first of the tile's four token rows
    const long urow = (long)a.B * a.T;                           // offset of the uncond half (guidance)
    const bool both = a.scale || a.mirror;                       // the state's uncond half is written too
    f32x4 x[4], x0[4];                                           // [frame][channel]
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
        x[tt] = *reinterpret_cast<const f32x4*>(a.xt + (row0 + tt) * a.ldx + j0);
        x0[tt] = *reinterpret_cast<const f32x4*>(a.x0t + (row0 + tt) * a.ldo + j0);
    }
    if (a.scale) {
        const float sc = a.scale[b];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            const f32x4 u = *reinterpret_cast<const f32x4*>(a.x0t + (urow + row0 + tt) * a.ldo + j0);
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) x0[tt][jj] = cfg_blend(x0[tt][jj], u[jj], sc);
        }
    }
    if (a.clip) {
#pragma unroll
        for (int tt = 0; tt < 4; ++tt)
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) x0[tt][jj] = clamp1(x0[tt][jj]);
    }
    const uint64_t sample = a.const_noise ? 0ull : a.sample_offset + (uint64_t)b;
    f32x4 r[4];
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
        const int j = j0 + jj;
        if (j < a.J) {
            const f32x4 z = a.noise ? *reinterpret_cast<const f32x4*>(a.noise + ((long)(a.const_noise ? 0 : b) * a.J + j) * a.T + t0)
                                    : philox_normal4(a.seed, sample, a.rng_step, (uint32_t)(j * tq_n + tq));   // frames t0 .. t0+3 of channel j
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) r[tt][jj] = update_value(a.kind, c, x[tt][jj], x0[tt][jj], z[tt]);
        } else {
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) r[tt][jj] = 0.0f;                                   // K padding of the input GEMM's operand
        }
    }
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
        *reinterpret_cast<f32x4*>(a.xt + (row0 + tt) * a.ldx + j0) = r[tt];
        if (both) *reinterpret_cast<f32x4*>(a.xt + (urow + row0 + tt) * a.ldx + j0) = r[tt];
    }
    if (a.xt16) {                                                  // the same values rounded once, as transpose_in_f16 would
        typedef _Float16 h4 __attribute__((ext_vector_type(4)));
        typedef __bf16 b4 __attribute__((ext_vector_type(4)));
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            const long o0 = (row0 + tt) * a.ldx + j0, o1 = o0 + urow * a.ldx;
            if (a.half_dtype == GDX_DTYPE_BF16) {
                const b4 v = b4{(__bf16)r[tt][0], (__bf16)r[tt][1], (__bf16)r[tt][2], (__bf16)r[tt][3]};
                *reinterpret_cast<b4*>((__bf16*)a.xt16 + o0) = v;
                if (both) *reinterpret_cast<b4*>((__bf16*)a.xt16 + o1) = v;
            } else {
                const h4 v = h4{(_Float16)r[tt][0], (_Float16)r[tt][1], (_Float16)r[tt][2], (_Float16)r[tt][3]};
                *reinterpret_cast<h4*>((_Float16*)a.xt16 + o0) = v;
                if (both) *reinterpret_cast<h4*>((_Float16*)a.xt16 + o1) = v;
            }
        }
    }
    if (a.out_pose) {
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
            if (j0 + jj < a.J)
                *reinterpret_cast<f32x4*>(a.out_pose + ((long)b * a.J + j0 + jj) * a.T + t0) = f32x4{r[0][jj], r[1][jj], r[2][jj], r[3][jj]};
    }
}

__global__ void q_sample_kernel(const float* __restrict__ xs, const float* __restrict__ nz, const float* coef,
                                int idx, const int64_t* __restrict__ t, long per_sample, long n, float* __restrict__ out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long row = t ? (long)t[i / per_sample] : (long)idx;
    const float a = coef[row * 8 + 5], b = coef[row * 8 + 6];
    out[i] = q_sample_value(a, b, xs[i], nz[i]);
}

// PLMS pieces (reference gaussian_diffusion.py:995-1079), every product / sum rounded separately in torch's op order.
// coef row c = coef[t]: c[0] sqrt_recip_alphas_cumprod, c[1] sqrt_recipm1_alphas_cumprod, c[2] sqrt(alpha_bar_prev),
// c[3] sqrt(1 - alpha_bar_prev), c[7] (t != 0).
//   kind 0: eps_from_xstart                                                   (_predict_eps_from_xstart)
//   kind 6: ddim_mean(x0, e0)                                                 (improved-Euler predictor)
//   kind 7: cond_score_xstart with e0 = gradient, e1[t] = sqrt(1 - alpha_bar) (pred_xstart under condition_score)
//   kind 8: xstart_from_eps(x, x0)                                            (pred_xstart from an EPSILON / PREVIOUS_X output)
//   kind 1..5: plms_tail(plms_combine(kind, e0, e1, e2, e3)) with keep = x0
__global__ void plms_kernel(int kind, const float* __restrict__ coef, const int64_t* __restrict__ t, int step_index,
                            const float* __restrict__ x, const float* __restrict__ x0, const float* __restrict__ e0,
                            const float* __restrict__ e1, const float* __restrict__ e2, const float* __restrict__ e3,
                            float* __restrict__ out, long per_sample, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long idx = t ? (long)t[i / per_sample] : (long)step_index;
    const float* c = coef + idx * 8;
    if (kind == 0) out[i] = eps_from_xstart(c[0], c[1], x[i], x0[i]);
    else if (kind == 6) out[i] = ddim_mean(c[2], c[3], x0[i], e0[i]);
    else if (kind == 7) out[i] = cond_score_xstart(c[0], c[1], e1[idx], x[i], x0[i], e0[i]);   // e0 = cond_fn gradient, e1 = sqrt(1 - alpha_bar) table
    else if (kind == 8) out[i] = xstart_from_eps(c[0], c[1], x[i], x0[i]);   // x0 slot = eps; with the (1/coef1, coef2/coef1) rows, x = xprev, slot = x_t
    else {
        const float v1 = kind != 1 ? e1[i] : 0.f, v2 = kind == 3 || kind == 4 ? e2[i] : 0.f, v3 = kind == 4 ? e3[i] : 0.f;
        out[i] = plms_tail(c, x[i], plms_combine(kind, e0[i], v1, v2, v3), x0[i]);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// One whole PLMS step in one pass (gdx.h gdx_plms_step): update_kernel's pred_xstart (CFG blend -> inpainting -> clamp),
// plms_kernel kind 0 (eps) and plms_kernel kind 1..6 on the values still in registers, every statement and rounding as
// there, so the result has the bits of the three launches.  Grid (ceil(groups / 256), B): blockIdx.y is the sample, the
// kind a template argument.  Kind 5 forms eps_2 from the SECOND forward of a loop's first step (state x_eps, row idx_e)
// and combines it with the stored eps (e1) and the first forward's pred (pred_prev) under row idx.
struct PlmsStepDev {
    StepSrc s;
    const int64_t* t_eps;
    int step_index_eps;
    const float *x_eps, *e1, *e2, *e3, *pred_prev;
    float* eps_out;
};

template <int KIND, bool VEC>
__global__ __launch_bounds__(256) void plms_step_kernel(const PlmsStepDev a) {
    const long grp = (long)blockIdx.x * 256 + threadIdx.x;
    if (grp >= a.s.groups) return;
    const Group g = group_at<VEC>(blockIdx.y, grp, a.s.per_sample);
    const long e0 = g.e0;
    const int nval = g.nval;
    const long idx = coef_row(a.s, g.b);
    const long idx_e = KIND == 5 ? (a.t_eps ? a.t_eps[g.b] : a.step_index_eps) : idx;     // row of this launch's eps
    const float* c = a.s.coef + idx * 8;
    const float* ce = a.s.coef + idx_e * 8;

    const f32x4 x = load4<VEC>(a.s.x, e0, nval);
    const f32x4 x0 = pred_xstart4<VEC>(a.s, g);
    const f32x4 xe = KIND == 5 ? load4<VEC>(a.x_eps, e0, nval) : x;
    f32x4 eps;
#pragma unroll
    for (int i = 0; i < 4; ++i) eps[i] = eps_from_xstart(ce[0], ce[1], xe[i], x0[i]);
    f32x4 e1 = {0.f, 0.f, 0.f, 0.f}, e2 = e1, e3 = e1;
    if (KIND == 2 || KIND == 3 || KIND == 4 || KIND == 5) e1 = load4<VEC>(a.e1, e0, nval);
    if (KIND == 3 || KIND == 4) e2 = load4<VEC>(a.e2, e0, nval);
    if (KIND == 4) e3 = load4<VEC>(a.e3, e0, nval);
    const f32x4 keep = KIND == 5 ? load4<VEC>(a.pred_prev, e0, nval) : x0;                // the (1 - nz) term's pred_xstart
    f32x4 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (KIND == 6) r[i] = ddim_mean(c[2], c[3], x0[i], eps[i]);
        else r[i] = plms_tail(c, x[i], plms_combine(KIND, eps[i], e1[i], e2[i], e3[i]), keep[i]);
    }
    if (a.eps_out) store4<VEC>(a.eps_out, e0, nval, eps);
    if (a.s.pred) store4<VEC>(a.s.pred, e0, nval, x0);
    store4<VEC>(a.s.out, e0, nval, r);
}

// ---------------------------------------------------------------------------------------------------------------
// One DPM-Solver++ multistep step in one pass (gdx.h gdx_dpm_step, gdx_dpm_sde_step): update_kernel's pred_xstart (CFG blend ->
// inpainting -> clamp) as m0, then dpm_multistep over it and NH older predictions, or (NOISE: SDE-DPM-Solver++)
// dpm_sde_multistep with the noise scale in column 7 and z from the tape or from philox_normal4 keyed like update_kernel
// (sample_offset + b, rng_step, group).  Grid (ceil(groups / 256), B): blockIdx.y is the sample, NH a template argument.  The
// row's weights of order NH + 1 start at column 1 + NH*(NH + 1)/2: (a, w1_0, w2_0, w2_1, w3_0, w3_1, w3_2, 0 or s).
// Memory-bound: per element 2 + NH reads (3 + NH under guidance, + mask and motion under inpainting, + one under a tape; one
// Philox draw per group without) and two writes.
struct DpmStepDev {
    StepSrc s;
    const float *m1, *m2;
    const float* noise;     // NOISE only, like seed, sample_offset and rng_step
    uint64_t seed, sample_offset;
    uint32_t rng_step;
};

template <int NH, bool NOISE, bool VEC>
__global__ __launch_bounds__(256) void dpm_step_kernel(const DpmStepDev a) {
    const long grp = (long)blockIdx.x * 256 + threadIdx.x;
    if (grp >= a.s.groups) return;
    const Group g = group_at<VEC>(blockIdx.y, grp, a.s.per_sample);
    const long e0 = g.e0;
    const int nval = g.nval;
    const float* c = a.s.coef + coef_row(a.s, g.b) * 8;
    const float* w = c + 1 + NH * (NH + 1) / 2;

    const f32x4 x = load4<VEC>(a.s.x, e0, nval);
    const f32x4 m0 = pred_xstart4<VEC>(a.s, g);
    f32x4 m1 = {0.f, 0.f, 0.f, 0.f}, m2 = m1, z = m1;
    if (NH >= 1) m1 = load4<VEC>(a.m1, e0, nval);
    if (NH >= 2) m2 = load4<VEC>(a.m2, e0, nval);
    if (NOISE) z = a.noise ? load4<VEC>(a.noise, e0, nval) : philox_normal4(a.seed, a.sample_offset + (uint64_t)g.b, a.rng_step, g.grp);
    f32x4 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (NOISE) r[i] = dpm_sde_multistep<NH>(c[0], w, c[7], x[i], m0[i], m1[i], z[i]);
        else r[i] = dpm_multistep<NH>(c[0], w, x[i], m0[i], m1[i], m2[i]);
    }
    if (a.s.pred) store4<VEC>(a.s.pred, e0, nval, m0);
    store4<VEC>(a.s.out, e0, nval, r);
}

// ---------------------------------------------------------------------------------------------------------------
// One UniPC step in one pass (gdx.h gdx_unipc_step): dpm_step_kernel's m0, then the corrector of order NC over m0 (= m_new) and
// the NC predictions before it on the base state x -- unipc_correct, weights from row idx + 1 of both tables; NC = 0: xc = x --
// and the predictor of order NP from xc, which is dpm_multistep<NP - 1> on the row's order-NP columns.  Grid (ceil(groups / 256),
// B): blockIdx.y is the sample, NC and NP template arguments.  Memory-bound, one pass, no LDS: per element 2 + max(NC, NP - 1)
// reads (one more under guidance, + mask and motion under inpainting) and three writes (xc, x_p, m0).
template <int NC>
__device__ __forceinline__ float unipc_correct(float ab, const float* c, float x, float mn, float h0, float h1, float h2) {
    float d = __fmul_rn(c[0], mn);
    d = __fadd_rn(d, __fmul_rn(c[1], h0));
    if (NC >= 2) d = __fadd_rn(d, __fmul_rn(c[2], h1));
    if (NC >= 3) d = __fadd_rn(d, __fmul_rn(c[3], h2));
    return __fadd_rn(__fmul_rn(ab, x), d);
}

struct UnipcStepDev {
    StepSrc s;              // x: the corrector's base state (NC = 0: the state itself); out: x_p; pred: m0
    const float* coef_c;
    const float *h0, *h1, *h2;
    float* base_out;
};

template <int NC, int NP, bool VEC>
__global__ __launch_bounds__(256) void unipc_step_kernel(const UnipcStepDev a) {
    constexpr int NHIST = NC > NP - 1 ? NC : NP - 1;               // history slots read
    const long grp = (long)blockIdx.x * 256 + threadIdx.x;
    if (grp >= a.s.groups) return;
    const Group g = group_at<VEC>(blockIdx.y, grp, a.s.per_sample);
    const long e0 = g.e0;
    const int nval = g.nval;
    const long idx = coef_row(a.s, g.b);
    const float* c = a.s.coef + idx * 8;
    const float* w = c + 1 + (NP - 1) * NP / 2;

    const f32x4 x = load4<VEC>(a.s.x, e0, nval);
    const f32x4 m0 = pred_xstart4<VEC>(a.s, g);
    f32x4 h0 = {0.f, 0.f, 0.f, 0.f}, h1 = h0, h2 = h0;
    if (NHIST >= 1) h0 = load4<VEC>(a.h0, e0, nval);
    if (NHIST >= 2) h1 = load4<VEC>(a.h1, e0, nval);
    if (NHIST >= 3) h2 = load4<VEC>(a.h2, e0, nval);
    f32x4 xc = x, r;
    if (NC > 0) {
        const float ab = a.s.coef[(idx + 1) * 8];
        const float* cc = a.coef_c + (idx + 1) * 16 + 4 * (NC - 1);
#pragma unroll
        for (int i = 0; i < 4; ++i) xc[i] = unipc_correct<NC>(ab, cc, x[i], m0[i], h0[i], h1[i], h2[i]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = dpm_multistep<NP - 1>(c[0], w, xc[i], m0[i], h0[i], h1[i]);
    if (a.s.pred) store4<VEC>(a.s.pred, e0, nval, m0);
    store4<VEC>(a.base_out, e0, nval, xc);
    store4<VEC>(a.s.out, e0, nval, r);
}

// ---------------------------------------------------------------------------------------------------------------
// One DDIM reverse-ODE (inversion) step in one pass (gdx.h gdx_ddim_reverse_step; reference :841-877): update_kernel's pred_xstart
// (CFG blend -> inpainting -> clamp) as m0, eps_from_xstart on the row's c0 / c1 and ddim_mean on its reverse columns c2 / c3 =
// sqrt(abar_next), sqrt(1 - abar_next).  No noise operand and no Philox draw: update_kernel with these rows and a zero tensor adds
// 0*0 to the same mean.  Grid (ceil(groups / 256), B): blockIdx.y is the sample.  Memory-bound, one pass, no LDS, one 128-bit
// access per stream and thread: per element 2 reads (3 under guidance, + mask and motion under inpainting) and 1..3 writes.
struct DdimReverseDev {
    StepSrc s;
    float* eps_out;
};

template <bool VEC>
__global__ __launch_bounds__(256) void ddim_reverse_step_kernel(const DdimReverseDev a) {
    const long grp = (long)blockIdx.x * 256 + threadIdx.x;
    if (grp >= a.s.groups) return;
    const Group g = group_at<VEC>(blockIdx.y, grp, a.s.per_sample);
    const float* c = a.s.coef + coef_row(a.s, g.b) * 8;

    const f32x4 x = load4<VEC>(a.s.x, g.e0, g.nval);
    const f32x4 m0 = pred_xstart4<VEC>(a.s, g);
    f32x4 eps, r;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        eps[i] = eps_from_xstart(c[0], c[1], x[i], m0[i]);
        r[i] = ddim_mean(c[2], c[3], m0[i], eps[i]);
    }
    if (a.eps_out) store4<VEC>(a.eps_out, g.e0, g.nval, eps);
    if (a.s.pred) store4<VEC>(a.s.pred, g.e0, g.nval, m0);
    store4<VEC>(a.s.out, g.e0, g.nval, r);
}

// De-normalisation + position / rotation split of a generated chunk (reference sample/generate.py:132-146 with
// data_loaders/gesture/data/dataset.py:118-119): feature 6j+c is rotation component c of joint j, 6j+3+c its position.
//   pos[b][j][c][t] = x[b][6j+3+c][t] * std[6j+3+c] + mean[6j+3+c],  rot[b][j][c][t] likewise with feature 6j+c.
// The reference multiplies the fp32 sample by fp64 statistics and rounds once at the end (.float()); so does this.
__global__ void postprocess_kernel(const float* __restrict__ x, const double* __restrict__ mean,
                                   const double* __restrict__ stdv, float* __restrict__ pos, float* __restrict__ rot,
                                   int nj, int T, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int t = i % T;
    const long r = i / T;                  // b * 6nj + f
    const int f = r % (6 * nj);
    const long b = r / (6 * nj);
    const int j = f / 6, c = f % 6;
    const float v = (float)__dadd_rn(__dmul_rn((double)x[i], stdv[f]), mean[f]);
    float* dst = c < 3 ? rot : pos;
    dst[((b * nj + j) * 3 + (c % 3)) * T + t] = v;
}

__global__ void randn_kernel(float* __restrict__ out, int batch, long per_sample, long groups, uint64_t seed,
                             uint64_t sample_offset, uint32_t step) {
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= groups * batch) return;
    const Group g = group_of<false>(gid, groups, per_sample);
    store4<false>(out, g.e0, g.nval, philox_normal4(seed, sample_offset + (uint64_t)g.b, step, g.grp));
}

// The forward hop of a resampled loop (gdx.h gdx_set_resample; gdx_sample_loop) in ONE pass, in place: x <- a*x + b*z with (a, b)
// row `row` of the handle's table and z this hop's tape slice or philox_normal4 keyed like update_kernel (sample_offset + b,
// rng_step, group), through q_sample_value: the bits of gdx_randn followed by gdx_q_sample on a row holding (c[5], c[6]) = (a, b).
// The whole tensor, an inpainted region included.  Memory-bound: per element one read and one write (+ one read under a tape).
// Not fused into the update in front of it: one forward hop comes per `jump` denoiser calls.
struct RenoiseDev {
    float* x;
    const float* tab;       // [rows][2]
    int row, batch;
    long per_sample, groups;
    const float* noise;     // nullptr (Philox) or [B][per_sample]
    uint64_t seed, sample_offset;
    uint32_t rng_step;
};

template <bool VEC>
__global__ __launch_bounds__(256) void renoise_kernel(const RenoiseDev a) {
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= a.groups * a.batch) return;
    const Group g = group_of<VEC>(gid, a.groups, a.per_sample);
    const float ca = a.tab[2L * a.row], cb = a.tab[2L * a.row + 1];
    const f32x4 x = load4<VEC>(a.x, g.e0, g.nval);
    const f32x4 z = a.noise ? load4<VEC>(a.noise, g.e0, g.nval)
                            : philox_normal4(a.seed, a.sample_offset + (uint64_t)g.b, a.rng_step, g.grp);
    f32x4 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = q_sample_value(ca, cb, x[i], z[i]);
    store4<VEC>(a.x, g.e0, g.nval, r);
}

// ---------------------------------------------------------------------------------------------------------------
// Parallel-in-time sampling (gdx.h gdx_window_sweep): the sequential update chain over a window of planes P_0 .. P_n with the
// denoiser's predictions M_0 .. M_{n-1} held fixed, in ONE launch.  A thread owns one group of four elements and walks the slots
// with the running state v in registers: v' = step(v, M_j) through pred_xstart4 / update_value / philox_normal4 -- the statements
// update_kernel runs, hence n successive gdx_sampler_update launches bit for bit --, the squared change of P_{j+1} in fp64, the
// store, v = v'.  Streaming: 2n planes read (M_j, old P_{j+1}; + tape noise, + mask and motion), n written.  The slot's squared
// differences are reduced across the wave inside the slot loop (one double per thread live at a time, not n) and meet in LDS
// once, behind the loop; the order is fixed, no atomics: thread -> wave -> block (= one chunk of GDX_BPD_CHUNK elements: 1024
// threads, one group each) -> part[(slot*B + b)*chunks + chunk], and window_err_kernel adds a (slot, sample)'s chunks in chunk
// order and divides by J*T.  Grid (chunks, B).
// The window kernels stay in update_kernel's file.  Compiled in a file of their own, window_sweep_kernel comes out with another
// instruction order (same register counts); with update_kernel in the translation unit -- the one caller that hands update_value
// a run-time `cond`, so its defaults are not folded into it before it is inlined -- the stream is unchanged
// (profiles/sampler_split_isa_compare.txt).
struct WindowSweepDev {
    StepSrc s;              // coef, step_index (slot 0's), mask / motion / clip, the geometry; x, x0c, out, pred are not read
    int kind, batch, n_slots, chunks;
    float* planes;          // [n_slots + 1][B][per_sample]
    const float* x0;        // [n_slots][B][per_sample]
    const float* noise;     // nullptr (Philox) or [n_slots][B][per_sample]
    long plane;             // B * per_sample
    uint64_t seed, sample_offset;
    uint32_t rng_step;      // slot 0's Philox draw
    double* part;
};
constexpr int WINDOW_MAX_SLOTS = 64;
static_assert(BPD_GROUPS == 1024, "window_sweep_kernel: one block of 1024 threads is one chunk");

template <bool VEC>
__global__ __launch_bounds__(1024) void window_sweep_kernel(const WindowSweepDev a) {
    __shared__ double red[BPD_GROUPS / 64][WINDOW_MAX_SLOTS];
    const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
    const long grp = (long)chunk * BPD_GROUPS + tid;
    const bool live = grp < a.s.groups;                            // a dead thread still takes part in the wave's reduction
    const Group g = group_at<VEC>(b, live ? grp : 0, a.s.per_sample);
    StepSrc s = a.s;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (live) v = load4<VEC>(a.planes, g.e0, g.nval);
    for (int j = 0; j < a.n_slots; ++j) {
        double d2 = 0.0;
        if (live) {
            const float* c = a.s.coef + (long)(a.s.step_index - j) * 8;
            s.x0c = a.x0 + (long)j * a.plane;
            const f32x4 x0 = pred_xstart4<VEC>(s, g);
            const f32x4 z = a.noise ? load4<VEC>(a.noise + (long)j * a.plane, g.e0, g.nval)
                                    : philox_normal4(a.seed, a.sample_offset + (uint64_t)b, a.rng_step + (uint32_t)j, g.grp);
            float* next = a.planes + (long)(j + 1) * a.plane;
            const f32x4 old = load4<VEC>(next, g.e0, g.nval);
            f32x4 r;
#pragma unroll
            for (int i = 0; i < 4; ++i) r[i] = update_value(a.kind, c, v[i], x0[i], z[i]);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (i < g.nval) {
                    const double d = __dsub_rn((double)r[i], (double)old[i]);
                    d2 = __dadd_rn(d2, __dmul_rn(d, d));
                }
            }
            store4<VEC>(next, g.e0, g.nval, r);
            v = r;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) d2 = __dadd_rn(d2, __shfl_down(d2, off, 64));
        if ((tid & 63) == 0) red[tid >> 6][j] = d2;
    }
    __syncthreads();
    if (tid < a.n_slots) {
        double t = red[0][tid];
#pragma unroll
        for (int w = 1; w < BPD_GROUPS / 64; ++w) t = __dadd_rn(t, red[w][tid]);
        a.part[((long)tid * a.batch + b) * a.chunks + chunk] = t;
    }
}

// err[i] = (the chunk sums of (slot, sample) pair i, in chunk order) / (J*T); one thread per pair
__global__ void window_err_kernel(const double* __restrict__ part, int chunks, long per_sample, int count, double* __restrict__ err) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    double t = 0.0;
    for (int ch = 0; ch < chunks; ++ch) t = __dadd_rn(t, part[(long)i * chunks + ch]);
    err[i] = __ddiv_rn(t, (double)per_sample);
}

// The window's slide by `stride` planes (gdx_parallel_loop): P_j <- P_{min(j + stride, W)} for j = 0 .. W-1 in ascending order, so
// the planes that fall off the end become copies of P_W.  A thread owns one element (V = f32x4: four) of every plane: what it
// reads at j + stride it has not yet written.  `count`: elements of type V per plane.
template <typename V>
__global__ __launch_bounds__(256) void window_slide_kernel(V* planes, long count, int W, int stride) {
    const long step = (long)gridDim.x * 256;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < count; e += step)
        for (int j = 0; j < W; ++j) planes[(long)j * count + e] = planes[(long)min(j + stride, W) * count + e];
}

__global__ void set_state_kernel(int* st, int idx, int k) { st[0] = idx; st[1] = k; }
__global__ void advance_state_kernel(int* st) { st[0] -= 1; st[1] += 1; }

hipError_t launch_set_state(int* st, int idx, int k, hipStream_t s) {
    hipLaunchKernelGGL(set_state_kernel, dim3(1), dim3(1), 0, s, st, idx, k);
    return hipGetLastError();
}
hipError_t launch_advance_state(int* st, hipStream_t s) {
    hipLaunchKernelGGL(advance_state_kernel, dim3(1), dim3(1), 0, s, st);
    return hipGetLastError();
}
}  // namespace gdx

static int sampler_update_impl(const gdx_update_args_t* a, const int* state, long noise_stride, void* stream);

// internal (loops.hip, gdx_sample_loop): one step of the token-major fast path (update_tm_kernel)
int gdx_sampler_update_tm_(const gdx::UpdateTmDev& d, void* stream) {
    using namespace gdx;
    const int jpad = (d.J + 3) / 4 * 4;
    if (!d.coef || !d.xt || !d.x0t || d.T % 4 || d.ldx % 4 || d.ldo % 4 || d.ldx < jpad || d.ldo < jpad)
        return gdx_set_error_("gdx_sampler_update_tm_: bad argument");
    if (d.noise && ((uintptr_t)d.noise & 15)) return gdx_set_error_("gdx_sampler_update_tm_: noise tape not 16-byte aligned");
    const long total = (long)d.B * (d.T / 4) * (jpad / 4);
    if (total == 0) return 0;
    hipLaunchKernelGGL(update_tm_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, d);
    return launch_status("gdx_sampler_update_tm_: launch failed");
}

extern "C" int gdx_sampler_update(const gdx_update_args_t* a, void* stream) {
    return sampler_update_impl(a, nullptr, 0, stream);
}

// internal: the update of a captured step (see UpdateDev::state)
int gdx_sampler_update_state_(const gdx_update_args_t* a, const int* state, long noise_stride, void* stream) {
    return sampler_update_impl(a, state, noise_stride, stream);
}

static int sampler_update_impl(const gdx_update_args_t* a, const int* state, long noise_stride, void* stream) {
    using namespace gdx;
    if (!a || !a->coef || !a->x || !a->x0_cond || !a->out) return gdx_set_error_("gdx_sampler_update: null argument");
    if (a->x0_uncond && !a->scale) return gdx_set_error_("gdx_sampler_update: CFG needs scale");
    if (a->inpaint_mask && !a->inpaint_motion) return gdx_set_error_("gdx_sampler_update: mask without motion");
    UpdateDev d;
    d.s = step_src(a, a->pred_xstart);
    d.kind = a->kind; d.batch = a->batch;
    d.noise = a->noise; d.const_noise = a->const_noise;
    d.seed = a->philox_seed; d.sample_offset = a->sample_offset; d.rng_step = a->rng_step;
    d.state = state; d.noise_stride = noise_stride;
    d.grad = a->cond_grad; d.gcoef = a->cond_coef;
    if (d.grad && a->kind != GDX_SAMPLER_P && !d.gcoef) return gdx_set_error_("gdx_sampler_update: cond_grad needs cond_coef for DDIM");
    const long total = d.s.groups * d.batch;
    if (total == 0) return 0;
    launch_vec(vec_ok(d.s, d.noise, d.grad), update_kernel<true>, update_kernel<false>, dim3((total + 255) / 256), dim3(256),
               (hipStream_t)stream, d);
    return launch_status("gdx_sampler_update: launch failed");
}

extern "C" int gdx_q_sample(const float* x_start, const float* noise, const float* coef, int32_t idx, int64_t count,
                            float* out, void* stream) {
    if (!x_start || !noise || !coef || !out) return gdx_set_error_("gdx_q_sample: null argument");
    if (count == 0) return 0;
    hipLaunchKernelGGL(gdx::q_sample_kernel, dim3((count + 255) / 256), dim3(256), 0, (hipStream_t)stream, x_start,
                       noise, coef, idx, (const int64_t*)nullptr, (long)count, (long)count, out);
    return launch_status("gdx_q_sample: launch failed");
}

extern "C" int gdx_q_sample_t(const float* x_start, const float* noise, const float* coef, const int64_t* t,
                              int32_t batch, int64_t per_sample, float* out, void* stream) {
    if (!x_start || !noise || !coef || !t || !out) return gdx_set_error_("gdx_q_sample_t: null argument");
    const long count = (long)batch * per_sample;
    if (count <= 0) return 0;
    hipLaunchKernelGGL(gdx::q_sample_kernel, dim3((count + 255) / 256), dim3(256), 0, (hipStream_t)stream, x_start,
                       noise, coef, 0, t, (long)per_sample, count, out);
    return launch_status("gdx_q_sample_t: launch failed");
}

extern "C" int gdx_plms_update(const gdx_plms_args_t* a, void* stream) {
    if (!a || !a->coef || !a->out) return gdx_set_error_("gdx_plms_update: null argument");
    if (a->kind < 0 || a->kind > 8) return gdx_set_error_("gdx_plms_update: bad kind");
    const int k = a->kind;
    const bool need_x = k != 6, need_x0 = true, need_e0 = k != 0 && k != 8, need_e1 = k == 2 || k == 3 || k == 4 || k == 5 || k == 7,
               need_e2 = k == 3 || k == 4, need_e3 = k == 4;
    if ((need_x && !a->x) || (need_x0 && !a->pred_xstart) || (need_e0 && !a->eps[0]) || (need_e1 && !a->eps[1]) ||
        (need_e2 && !a->eps[2]) || (need_e3 && !a->eps[3]))
        return gdx_set_error_("gdx_plms_update: missing operand for this kind");
    const long total = (long)a->batch * a->per_sample;
    if (total <= 0) return 0;
    hipLaunchKernelGGL(gdx::plms_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, k, a->coef, a->t,
                       a->step_index, a->x, a->pred_xstart, a->eps[0], a->eps[1], a->eps[2], a->eps[3], a->out,
                       (long)a->per_sample, total);
    return launch_status("gdx_plms_update: launch failed");
}

static void launch_plms_step(int kind, bool vec, dim3 grid, hipStream_t s, const gdx::PlmsStepDev& d) {
    using namespace gdx;
    const dim3 block(256);
    switch (kind) {
        case 1: launch_vec(vec, plms_step_kernel<1, true>, plms_step_kernel<1, false>, grid, block, s, d); break;
        case 2: launch_vec(vec, plms_step_kernel<2, true>, plms_step_kernel<2, false>, grid, block, s, d); break;
        case 3: launch_vec(vec, plms_step_kernel<3, true>, plms_step_kernel<3, false>, grid, block, s, d); break;
        case 4: launch_vec(vec, plms_step_kernel<4, true>, plms_step_kernel<4, false>, grid, block, s, d); break;
        case 5: launch_vec(vec, plms_step_kernel<5, true>, plms_step_kernel<5, false>, grid, block, s, d); break;
        default: launch_vec(vec, plms_step_kernel<6, true>, plms_step_kernel<6, false>, grid, block, s, d); break;
    }
}

extern "C" int gdx_plms_step(const gdx_plms_step_args_t* a, void* stream) {
    using namespace gdx;
    PlmsStepDev d;
    dim3 grid;
    int older = 0;                                                  // history slots this kind reads
    const int rc = step_begin(
        "gdx_plms_step", a, &gdx_plms_step_args_t::pred_xstart, [&] { return a->kind < 1 || a->kind > 6 ? "bad kind" : nullptr; },
        [&]() -> const char* {
            const int k = a->kind;
            older = k <= 4 ? k - 1 : (k == 5 ? 1 : 0);
            for (int i = 0; i < older; ++i)
                if (!a->eps_hist[i]) return "missing history for this kind";
            if (k != 5 && !a->eps_out) return "missing history for this kind";
            if (k == 5 && (!a->x_eps || !a->pred_prev)) return "kind 5 needs x_eps and pred_prev";
            return nullptr;
        },
        d.s, grid);
    if (rc) return rc < 0 ? -1 : 0;
    const int k = a->kind;
    d.t_eps = a->t_eps; d.step_index_eps = a->step_index_eps;
    d.x_eps = k == 5 ? a->x_eps : nullptr; d.pred_prev = k == 5 ? a->pred_prev : nullptr;
    d.e1 = older > 0 ? a->eps_hist[0] : nullptr; d.e2 = older > 1 ? a->eps_hist[1] : nullptr;
    d.e3 = older > 2 ? a->eps_hist[2] : nullptr; d.eps_out = a->eps_out;
    launch_plms_step(k, vec_ok(d.s, d.x_eps, d.e1, d.e2, d.e3, d.pred_prev, d.eps_out), grid, (hipStream_t)stream, d);
    return launch_status("gdx_plms_step: launch failed");
}

template <bool NOISE>
static void launch_dpm_step(int nh, bool vec, dim3 grid, hipStream_t s, const gdx::DpmStepDev& d) {
    using namespace gdx;
    const dim3 block(256);
    if (nh == 0) launch_vec(vec, dpm_step_kernel<0, NOISE, true>, dpm_step_kernel<0, NOISE, false>, grid, block, s, d);
    else if (NOISE || nh == 1) launch_vec(vec, dpm_step_kernel<1, NOISE, true>, dpm_step_kernel<1, NOISE, false>, grid, block, s, d);
    else launch_vec(vec, dpm_step_kernel<2, false, true>, dpm_step_kernel<2, false, false>, grid, block, s, d);
}

// gdx_dpm_step (NOISE = false: orders 1..3) and gdx_dpm_sde_step (NOISE = true: orders 1..2, the noise fields)
template <bool NOISE, typename A>
static int dpm_step_impl(const char* who, const A* a, void* stream) {
    using namespace gdx;
    DpmStepDev d = {};
    dim3 grid;
    const int rc = step_begin(
        who, a, &A::pred_out,
        [&] { return a->order >= 1 && a->order <= (NOISE ? 2 : 3) ? nullptr : (NOISE ? "order must be 1 or 2" : "order must be 1, 2 or 3"); },
        [&]() -> const char* {
            for (int i = 0; i < a->order - 1; ++i) {                // history slots this order reads
                if (!a->hist[i]) return "missing history for this order";
                if (a->pred_out && a->pred_out == a->hist[i]) return "pred_out aliases a history slot it reads";
            }
            return nullptr;
        },
        d.s, grid);
    if (rc) return rc < 0 ? -1 : 0;
    const int nh = a->order - 1;
    d.m1 = nh > 0 ? a->hist[0] : nullptr;
    if constexpr (NOISE) {
        d.noise = a->noise; d.seed = a->philox_seed; d.sample_offset = a->sample_offset; d.rng_step = a->rng_step;
    } else {
        d.m2 = nh > 1 ? a->hist[1] : nullptr;
    }
    launch_dpm_step<NOISE>(nh, vec_ok(d.s, d.m1, d.m2, d.noise), grid, (hipStream_t)stream, d);
    return hipGetLastError() == hipSuccess ? 0 : refuse(who, "launch failed");
}
extern "C" int gdx_dpm_step(const gdx_dpm_step_args_t* a, void* stream) { return dpm_step_impl<false>("gdx_dpm_step", a, stream); }
extern "C" int gdx_dpm_sde_step(const gdx_dpm_sde_step_args_t* a, void* stream) {
    return dpm_step_impl<true>("gdx_dpm_sde_step", a, stream);
}

// The (corr_order, pred_order) pairs the order rule of gdx_unipc_loop reaches (gdx.h), the only instantiations
static bool unipc_pair_ok(int nc, int np) {
    return np == 1 ? nc <= 1 : (np == 2 ? nc >= 1 : nc >= 2);
}

static void launch_unipc_step(int nc, int np, bool vec, dim3 grid, hipStream_t s, const gdx::UnipcStepDev& d) {
    using namespace gdx;
    const dim3 block(256);
    switch (nc * 4 + np) {
        case 0 * 4 + 1: launch_vec(vec, unipc_step_kernel<0, 1, true>, unipc_step_kernel<0, 1, false>, grid, block, s, d); break;
        case 1 * 4 + 1: launch_vec(vec, unipc_step_kernel<1, 1, true>, unipc_step_kernel<1, 1, false>, grid, block, s, d); break;
        case 1 * 4 + 2: launch_vec(vec, unipc_step_kernel<1, 2, true>, unipc_step_kernel<1, 2, false>, grid, block, s, d); break;
        case 2 * 4 + 2: launch_vec(vec, unipc_step_kernel<2, 2, true>, unipc_step_kernel<2, 2, false>, grid, block, s, d); break;
        case 3 * 4 + 2: launch_vec(vec, unipc_step_kernel<3, 2, true>, unipc_step_kernel<3, 2, false>, grid, block, s, d); break;
        case 2 * 4 + 3: launch_vec(vec, unipc_step_kernel<2, 3, true>, unipc_step_kernel<2, 3, false>, grid, block, s, d); break;
        default: launch_vec(vec, unipc_step_kernel<3, 3, true>, unipc_step_kernel<3, 3, false>, grid, block, s, d); break;
    }
}

extern "C" int gdx_unipc_step(const gdx_unipc_step_args_t* a, void* stream) {
    using namespace gdx;
    const char* who = "gdx_unipc_step";
    UnipcStepDev d = {};
    dim3 grid;
    int nh = 0;                                                     // history slots this pair reads
    const int rc = step_begin(
        who, a, &gdx_unipc_step_args_t::pred_out,
        [&]() -> const char* {
            if (!a->base_out) return "null argument";
            if (a->corr_order < 0 || a->corr_order > 3) return "corr_order must be 0, 1, 2 or 3";
            if (a->pred_order < 1 || a->pred_order > 3) return "pred_order must be 1, 2 or 3";
            if (!unipc_pair_ok(a->corr_order, a->pred_order)) return "no such (corr_order, pred_order) pair in the order rule";
            if (a->corr_order > 0 && !a->coef_c) return "corr_order > 0 needs coef_c";
            return a->base_out == a->out ? "base_out aliases out" : nullptr;
        },
        [&]() -> const char* {
            nh = std::max(a->corr_order, a->pred_order - 1);
            for (int i = 0; i < nh; ++i) {
                if (!a->hist[i]) return "missing history for these orders";
                if (a->pred_out && a->pred_out == a->hist[i]) return "pred_out aliases a history slot it reads";
            }
            return nullptr;
        },
        d.s, grid);
    if (rc) return rc < 0 ? -1 : 0;
    d.coef_c = a->coef_c; d.base_out = a->base_out;
    d.h0 = nh > 0 ? a->hist[0] : nullptr; d.h1 = nh > 1 ? a->hist[1] : nullptr; d.h2 = nh > 2 ? a->hist[2] : nullptr;
    launch_unipc_step(a->corr_order, a->pred_order, vec_ok(d.s, d.h0, d.h1, d.h2, d.base_out), grid, (hipStream_t)stream, d);
    return launch_status("gdx_unipc_step: launch failed");
}

extern "C" int gdx_ddim_reverse_step(int32_t batch, int32_t njoints, int32_t frames, const float* coef, const int64_t* t,
                                     int32_t step_index, const float* x, const float* x0_cond, const float* x0_uncond,
                                     const float* scale, const uint8_t* inpaint_mask, const float* inpaint_motion,
                                     int32_t clip_denoised, float* out, float* pred_out, float* eps_out, void* stream) {
    return gdx_ddim_reverse_step_(gdx::DdimReverseStepArgs{batch, njoints, frames, coef, t, step_index, x, x0_cond, x0_uncond, scale,
                                                           inpaint_mask, inpaint_motion, clip_denoised, out, pred_out, eps_out},
                                  stream);
}

int gdx_ddim_reverse_step_(const gdx::DdimReverseStepArgs& args, void* stream) {
    using namespace gdx;
    const DdimReverseStepArgs* a = &args;
    DdimReverseDev d = {};
    dim3 grid;
    const int rc = step_begin(
        "gdx_ddim_reverse_step", a, &DdimReverseStepArgs::pred_out, [] { return (const char*)nullptr; },
        [&]() -> const char* {
            if ((a->pred_out && (a->pred_out == a->eps_out || a->pred_out == a->out)) || (a->eps_out && a->eps_out == a->out))
                return "out, pred_out and eps_out must differ";
            return nullptr;
        },
        d.s, grid);
    if (rc) return rc < 0 ? -1 : 0;
    d.eps_out = a->eps_out;
    launch_vec(vec_ok(d.s, d.eps_out), ddim_reverse_step_kernel<true>, ddim_reverse_step_kernel<false>, grid, dim3(256),
               (hipStream_t)stream, d);
    return launch_status("gdx_ddim_reverse_step: launch failed");
}

extern "C" int gdx_window_sweep(int32_t kind, int32_t batch, int32_t njoints, int32_t frames, int32_t n_slots, const float* coef,
                                int32_t first_index, float* planes, const float* x0, const uint8_t* inpaint_mask,
                                const float* inpaint_motion, int32_t clip_denoised, const float* noise, uint64_t philox_seed,
                                uint64_t sample_offset, uint32_t rng_step, double* err, double* workspace, void* stream) {
    using namespace gdx;
    const char* who = "gdx_window_sweep";
    if (!coef || !planes || !x0 || !err || !workspace) return refuse(who, "null argument");
    if (kind != GDX_SAMPLER_P && kind != GDX_SAMPLER_DDIM) return refuse(who, "kind must be GDX_SAMPLER_P or GDX_SAMPLER_DDIM");
    if (batch < 0 || njoints < 0 || frames < 0 || batch > 65535) return refuse(who, "bad shape");
    if (n_slots < 1 || n_slots > WINDOW_MAX_SLOTS) return refuse(who, "n_slots must lie in 1 .. 64");
    if (first_index < n_slots - 1) return refuse(who, "the window runs below index 0 (first_index < n_slots - 1)");
    if (inpaint_mask && !inpaint_motion) return refuse(who, "mask without motion");
    if (((uintptr_t)err | (uintptr_t)workspace) & 7) return refuse(who, "err and workspace must be 8-byte aligned");
    WindowSweepDev d = {};
    StepSrc& s = d.s;
    s.per_sample = (long)njoints * frames;
    s.groups = (s.per_sample + 3) / 4;
    if (batch == 0 || s.per_sample == 0) return 0;
    s.coef = coef; s.step_index = first_index;
    s.mask = inpaint_mask; s.motion = inpaint_motion; s.clip = clip_denoised;
    d.kind = kind; d.batch = batch; d.n_slots = n_slots;
    d.chunks = (int)bpd_chunks(s.per_sample);
    d.planes = planes; d.x0 = x0; d.noise = noise; d.plane = (long)batch * s.per_sample;
    d.seed = philox_seed; d.sample_offset = sample_offset; d.rng_step = rng_step;
    d.part = workspace;
    hipStream_t st = (hipStream_t)stream;
    // per_sample % 4 == 0 keeps every plane / slot / tape slice as aligned as its base
    launch_vec(vec_ok(s.per_sample, (const float*)planes, x0, noise, inpaint_mask, inpaint_motion), window_sweep_kernel<true>,
               window_sweep_kernel<false>, dim3(d.chunks, batch), dim3(BPD_GROUPS), st, d);
    if (launch_status("gdx_window_sweep: launch failed")) return -1;
    const int pairs = n_slots * batch;
    hipLaunchKernelGGL(window_err_kernel, dim3((pairs + 63) / 64), dim3(64), 0, st, d.part, d.chunks, s.per_sample, pairs, err);
    return launch_status("gdx_window_sweep: launch failed");
}

// internal (loops.hip, gdx_parallel_loop): planes [W + 1][plane] slid down by `stride` planes (window_slide_kernel)
int gdx_window_slide_(float* planes, long plane, int W, int stride, void* stream) {
    using namespace gdx;
    if (plane == 0 || stride <= 0) return 0;
    const bool vec = plane % 4 == 0 && group_aligned(planes);
    const long count = vec ? plane / 4 : plane;
    const dim3 grid((unsigned)std::min(2048L, (count + 255) / 256)), block(256);
    if (vec) hipLaunchKernelGGL(window_slide_kernel<f32x4>, grid, block, 0, (hipStream_t)stream, (f32x4*)planes, count, W, stride);
    else hipLaunchKernelGGL(window_slide_kernel<float>, grid, block, 0, (hipStream_t)stream, planes, count, W, stride);
    return launch_status("gdx_parallel_loop: slide launch failed");
}

// internal (loops.hip, gdx_sample_loop under gdx_set_resample): one forward hop on the state x [batch][per_sample], in place
int gdx_renoise_(float* x, const float* tab, int row, int batch, long per_sample, const float* noise, uint64_t seed,
                 uint64_t sample_offset, uint32_t rng_step, void* stream) {
    using namespace gdx;
    RenoiseDev d;
    d.x = x; d.tab = tab; d.row = row; d.batch = batch;
    d.per_sample = per_sample; d.groups = (per_sample + 3) / 4;
    d.noise = noise; d.seed = seed; d.sample_offset = sample_offset; d.rng_step = rng_step;
    const long total = d.groups * batch;
    if (total == 0) return 0;
    launch_vec(vec_ok(per_sample, (const float*)x, noise), renoise_kernel<true>, renoise_kernel<false>, dim3((total + 255) / 256),
               dim3(256), (hipStream_t)stream, d);
    return launch_status("gdx_sample_loop: forward hop launch failed");
}

extern "C" int gdx_postprocess(const float* x, const double* mean, const double* stdv, float* pos, float* rot,
                               int32_t batch, int32_t n_joints, int32_t frames, void* stream) {
    if (!x || !mean || !stdv || !pos || !rot) return gdx_set_error_("gdx_postprocess: null argument");
    const long total = (long)batch * n_joints * 6 * frames;
    if (total <= 0) return 0;
    hipLaunchKernelGGL(gdx::postprocess_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, x, mean,
                       stdv, pos, rot, n_joints, frames, total);
    return launch_status("gdx_postprocess: launch failed");
}

extern "C" int gdx_randn(float* out, int32_t batch, int64_t per_sample, uint64_t philox_seed, uint64_t sample_offset,
                         uint32_t rng_step, void* stream) {
    if (!out) return gdx_set_error_("gdx_randn: null argument");
    const long groups = (per_sample + 3) / 4;
    const long total = groups * batch;
    if (total == 0) return 0;
    hipLaunchKernelGGL(gdx::randn_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, out, batch,
                       (long)per_sample, groups, philox_seed, sample_offset, rng_step);
    return launch_status("gdx_randn: launch failed");
}
