// Fused reverse-process update over the pose tensor [B, J, 1, T] (HBM-bound, float4 streaming):
// classifier-free-guidance blend + inpainting blend + posterior mean / DDIM step + Gaussian noise
// (noise tape or in-kernel Philox4x32-10) in ONE pass.
//
// Replaces the 6-10 separate elementwise torch kernels and 6-10 host->device table copies per step of
// reference diffusion/gaussian_diffusion.py:307-311 (inpainting), :253-275 (posterior mean),
// :524-548 (p_sample), :748-782 (ddim_sample), :1595-1608 (_extract_into_tensor) and
// model/cfg_sampler.py:28.  Products and sums are rounded separately (__fmul_rn/__fadd_rn, never
// contracted into FMA) in the reference's operation order, so given the same x0 / x / noise the
// result is bit-identical to the torch expression.  Algorithmic bytes per element: read x, x0 (+ x0_u,
// + tape noise), write x_{t-1}  ->  12-20 B.
// NOTE: HIP's __fmul_rn/__fadd_rn are plain * and + and hipcc defaults to -ffp-contract=fast, so this
// file is compiled with -ffp-contract=off (Makefile) AND carries the pragma below: bit-exactness against
// the torch expression depends on no mul+add pair being fused.
#include <algorithm>
#include <string>

#include "gdx_internal.h"
#include "gdx_device.h"
#include "../../include/gdx.h"

#pragma clang fp contract(off)

namespace gdx {


struct Philox {
    static constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
    __device__ static void run(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
        for (int r = 0; r < 10; ++r) {
            const uint32_t hi0 = __umulhi(M0, c[0]), lo0 = M0 * c[0];
            const uint32_t hi1 = __umulhi(M1, c[2]), lo1 = M1 * c[2];
            const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
            c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
            k0 += W0; k1 += W1;
        }
    }
};

// 4 standard normals for element group `grp` of sample `sample` at draw `step` (Box-Muller on
// 24-bit uniforms; oracle/philox.py restates this bit for bit up to libm rounding).
__device__ __forceinline__ f32x4 philox_normal4(uint64_t seed, uint64_t sample, uint32_t step, uint32_t grp) {
    uint32_t c[4] = {grp, step, (uint32_t)sample, (uint32_t)(sample >> 32)};
    Philox::run(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const float inv24 = 1.0f / 16777216.0f;
    const float u0 = (float)((c[0] >> 8) + 1u) * inv24, u1 = (float)(c[1] >> 8) * inv24;
    const float u2 = (float)((c[2] >> 8) + 1u) * inv24, u3 = (float)(c[3] >> 8) * inv24;
    const float r0 = sqrtf(-2.0f * logf(u0)), r1 = sqrtf(-2.0f * logf(u2));
    const float a0 = 6.28318530717958647692f * u1, a1 = 6.28318530717958647692f * u3;
    f32x4 z;
    z[0] = r0 * cosf(a0); z[1] = r0 * sinf(a0); z[2] = r1 * cosf(a1); z[3] = r1 * sinf(a1);
    return z;
}

// ---------------------------------------------------------------------------------------------------------------
// Device helpers.  Every formula whose bits are pinned to the reference's torch expression is written ONCE, here, and every
// kernel below calls it: two kernels agree bit for bit because they run the same statements, not because two copies were
// kept in step.  Each product / sum / quotient is its own __fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn in torch's op order;
// the helpers must stay in this translation unit (contraction off, see the top of the file).

// A group = four consecutive elements of one sample in the pose layout [B][J*T]; the last group of a sample holds `nval` < 4
// elements when J*T % 4 != 0 (VEC = false).  `grp` is also the Philox group number.
struct Group {
    int b;
    uint32_t grp;
    long e0;                // flat index of the group's first element
    int nval;
};
template <bool VEC>
__device__ __forceinline__ Group group_at(int b, long grp, long per_sample) {          // 2-D grids: blockIdx.y = sample
    return Group{b, (uint32_t)grp, (long)b * per_sample + 4L * grp, VEC ? 4 : (int)min(4L, per_sample - 4L * grp)};
}
template <bool VEC>
__device__ __forceinline__ Group group_of(long gid, long groups, long per_sample) {    // 1-D grids: gid = b * groups + grp
    const int b = gid / groups;
    return group_at<VEC>(b, gid - (long)b * groups, per_sample);
}

template <bool VEC>
__device__ __forceinline__ f32x4 load4(const float* p, long e0, int nval) {
    if (VEC) return *reinterpret_cast<const f32x4*>(p + e0);
    f32x4 v;
    for (int i = 0; i < 4; ++i) v[i] = i < nval ? p[e0 + i] : 0.f;
    return v;
}
template <bool VEC>
__device__ __forceinline__ void store4(float* p, long e0, int nval, const f32x4 v) {
    if (VEC) *reinterpret_cast<f32x4*>(p + e0) = v;
    else for (int i = 0; i < nval; ++i) p[e0 + i] = v[i];
}
// the group's four mask bytes, byte i in bits 8i .. 8i+7 (an element is masked when its byte is non-zero)
template <bool VEC>
__device__ __forceinline__ uint32_t mask4(const uint8_t* p, long e0, int nval) {
    if (VEC) return *reinterpret_cast<const uint32_t*>(p + e0);
    uint32_t m = 0;
    for (int i = 0; i < nval; ++i) m |= (uint32_t)p[e0 + i] << (8 * i);
    return m;
}

// classifier-free guidance (model/cfg_sampler.py:28): u + sc * (c - u)
__device__ __forceinline__ float cfg_blend(float c, float u, float sc) { return __fadd_rn(u, __fmul_rn(sc, __fsub_rn(c, u))); }
// torch.clamp(v, -1, 1): a NaN stays a NaN
__device__ __forceinline__ float clamp1(float v) { return v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v); }

// What every pose-layout step kernel is given besides its own operands: the group geometry, the coefficient row selection,
// the state x, the x0 operands of pred_xstart4, and the outputs (x_{t-1}, and pred = the x0 it formed, or nullptr).
struct StepSrc {
    long per_sample;        // J*T
    long groups;            // ceil(per_sample/4)
    const float* coef;
    const int64_t* t;
    int step_index;
    const float *x, *x0c, *x0u, *scale;
    const uint8_t* mask;
    const float* motion;
    int clip;               // clip_denoised: x0 clamped to [-1, 1] after the CFG / inpainting blends (reference :349-355)
    float *out, *pred;
};
// the coefficient row of sample b
__device__ __forceinline__ long coef_row(const StepSrc& s, int b) { return s.t ? s.t[b] : s.step_index; }

// pred_xstart of p_mean_variance for group g: CFG blend (x0u set) -> inpainting (:307-311) -> clip_denoised (:349-355)
// (the guidance scale scale[b] is read only under guidance)
template <bool VEC>
__device__ __forceinline__ f32x4 pred_xstart4(const StepSrc& s, const Group& g) {
    f32x4 x0 = load4<VEC>(s.x0c, g.e0, g.nval);
    if (s.x0u) {
        const f32x4 u = load4<VEC>(s.x0u, g.e0, g.nval);
        const float sc = s.scale[g.b];
#pragma unroll
        for (int i = 0; i < 4; ++i) x0[i] = cfg_blend(x0[i], u[i], sc);
    }
    if (s.mask) {
        const uint32_t m = mask4<VEC>(s.mask, g.e0, g.nval);
        const f32x4 mo = load4<VEC>(s.motion, g.e0, g.nval);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if ((m >> (8 * i)) & 0xffu) x0[i] = mo[i];
    }
    if (s.clip) {
#pragma unroll
        for (int i = 0; i < 4; ++i) x0[i] = clamp1(x0[i]);
    }
    return x0;
}

// _predict_eps_from_xstart (:407-411): (c0*x - x0) / c1, with c0 = sqrt_recip_alphas_cumprod, c1 = sqrt_recipm1_alphas_cumprod
__device__ __forceinline__ float eps_from_xstart(float c0, float c1, float x, float x0) {
    return __fdiv_rn(__fsub_rn(__fmul_rn(c0, x), x0), c1);
}
// _predict_xstart_from_eps (:390-396): c0*x - c1*eps
__device__ __forceinline__ float xstart_from_eps(float c0, float c1, float x, float eps) {
    return __fsub_rn(__fmul_rn(c0, x), __fmul_rn(c1, eps));
}
// pred_xstart under condition_score (:452-472): eps - sqrt(1 - alpha_bar) * gradient, and x0 back from it
__device__ __forceinline__ float cond_score_xstart(float c0, float c1, float s1m, float x, float x0, float grad) {
    return xstart_from_eps(c0, c1, x, __fsub_rn(eps_from_xstart(c0, c1, x, x0), __fmul_rn(s1m, grad)));
}
// a*x0 + b*x: the posterior mean (:253-275) with (a, b) = posterior_mean_coef1/2
__device__ __forceinline__ float posterior_mean(float a, float b, float x0, float x) { return __fadd_rn(__fmul_rn(a, x0), __fmul_rn(b, x)); }
// x0*a + b*eps: the DDIM / improved-Euler mean (:766-770, :1046) with (a, b) = sqrt(alpha_bar_prev), sqrt(1 - alpha_bar_prev [- sigma^2])
__device__ __forceinline__ float ddim_mean(float a, float b, float x0, float eps) { return __fadd_rn(__fmul_rn(x0, a), __fmul_rn(b, eps)); }
// q_sample (:233-251): sa*x + s1m*z
__device__ __forceinline__ float q_sample_value(float sa, float s1m, float x, float z) { return __fadd_rn(__fmul_rn(sa, x), __fmul_rn(s1m, z)); }

// The ancestral (p_sample :524-548) / DDIM (:748-782) step of one element, c = the step's coefficient row.  cond: cond_fn
// guidance with gradient `grad` -- condition_mean (mean + variance * gradient, c[3] = posterior variance) for the ancestral
// step, condition_score (s1m = sqrt(1 - alpha_bar)) for DDIM.
__device__ __forceinline__ float update_value(int kind, const float* c, float x, float x0, float z, bool cond = false,
                                              float grad = 0.f, float s1m = 0.f) {
    if (kind == GDX_SAMPLER_P) {
        float mean = posterior_mean(c[0], c[1], x0, x);
        if (cond) mean = __fadd_rn(mean, __fmul_rn(c[3], grad));
        return __fadd_rn(mean, __fmul_rn(c[2], z));
    }
    if (cond) x0 = cond_score_xstart(c[0], c[1], s1m, x, x0, grad);
    const float mean = ddim_mean(c[2], c[3], x0, eps_from_xstart(c[0], c[1], x, x0));
    return __fadd_rn(mean, __fmul_rn(c[4], z));
}

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

// masked_l2 (reference gaussian_diffusion.py:201-213): out[b] = sum_{j,t} (a - b)^2 * mask[b,t] / (J * sum_t mask[b,t]).
// One block per sample, fp32 partial sums per thread, tree reduce in LDS (the summation order differs from torch's).
__global__ __launch_bounds__(256) void masked_l2_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                        const uint8_t* __restrict__ mask, float* __restrict__ out, int J,
                                                        int T) {
    __shared__ float ssum[256];
    __shared__ float scnt[256];
    const int bidx = blockIdx.x, tid = threadIdx.x;
    const long base = (long)bidx * J * T;
    float s = 0.0f, c = 0.0f;
    for (long i = tid; i < (long)J * T; i += 256) {
        const int t = i % T;
        const float m = mask[(long)bidx * T + t] ? 1.0f : 0.0f;
        const float d = a[base + i] - b[base + i];
        s += d * d * m;
    }
    for (int t = tid; t < T; t += 256) c += mask[(long)bidx * T + t] ? 1.0f : 0.0f;
    ssum[tid] = s;
    scnt[tid] = c;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            ssum[tid] += ssum[tid + o];
            scnt[tid] += scnt[tid + o];
        }
        __syncthreads();
    }
    if (tid == 0) out[bidx] = ssum[0] / (scnt[0] * (float)J);
}

__global__ void randn_kernel(float* __restrict__ out, int batch, long per_sample, long groups, uint64_t seed,
                             uint64_t sample_offset, uint32_t step) {
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= groups * batch) return;
    const Group g = group_of<false>(gid, groups, per_sample);
    store4<false>(out, g.e0, g.nval, philox_normal4(seed, sample_offset + (uint64_t)g.b, step, g.grp));
}

// classifier-free guidance blend (model/cfg_sampler.py:28), op order as the reference.  Guidance interval
// (gdx_set_guidance_interval): a sample whose timestep t[b] lies outside [lo, hi] takes the conditional output c itself
__global__ void cfg_blend_kernel(const float* __restrict__ c, const float* __restrict__ u,
                                 const float* __restrict__ scale, const int64_t* __restrict__ t, int64_t lo, int64_t hi,
                                 float* __restrict__ out, long per_sample, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long b = i / per_sample;
    const int64_t tb = t[b];
    out[i] = lo <= tb && tb <= hi ? cfg_blend(c[i], u[i], scale[b]) : c[i];
}

// Per-condition guidance, 3-pass rule (gdx.h gdx_set_guidance_compose): g = g1 + s1*(f - m) with g1 = u + s0*(m - u), every
// difference, product and sum rounded on its own.  A sample is composed when t == NULL or lo <= t[b] <= hi (cfg_blend_kernel's
// rule), else it is f.  Grid (ceil(groups / 256), B) like cfg_rescale_apply_kernel; out may alias f, m or u (no __restrict__: a
// thread reads its group of every operand before it writes it, and no other thread touches that group).
struct CfgComposeDev {
    long per_sample, groups;
    const float *f, *m, *u, *s0, *s1;
    const int64_t* t;
    int64_t lo, hi;
    float* out;
};
__device__ __forceinline__ float cfg_compose(float f, float m, float u, float s0, float s1) {
    return __fadd_rn(cfg_blend(m, u, s0), __fmul_rn(s1, __fsub_rn(f, m)));
}
template <bool VEC>
__global__ __launch_bounds__(256) void cfg_compose_kernel(const CfgComposeDev a) {
    const long grp = (long)blockIdx.x * 256 + threadIdx.x;
    if (grp >= a.groups) return;
    const Group g = group_at<VEC>(blockIdx.y, grp, a.per_sample);
    f32x4 x0 = load4<VEC>(a.f, g.e0, g.nval);
    bool guided = true;
    if (a.t) {
        const int64_t tb = a.t[g.b];
        guided = a.lo <= tb && tb <= a.hi;
    }
    if (guided) {
        const f32x4 m = load4<VEC>(a.m, g.e0, g.nval), u = load4<VEC>(a.u, g.e0, g.nval);
        const float s0 = a.s0[g.b], s1 = a.s1[g.b];
#pragma unroll
        for (int i = 0; i < 4; ++i) x0[i] = cfg_compose(x0[i], m[i], u[i], s0, s1);
    }
    store4<VEC>(a.out, g.e0, g.nval, x0);
}

// ---------------------------------------------------------------------------------------------------------------
// Variational bound (reference gaussian_diffusion.py:1192-1225, 1519-1592, diffusion/losses.py:12-77; gdx.h gdx_bpd_terms).
// bpd_xt_kernel forms x_t = sa*x0 + s1m*z with in-kernel Philox noise and STORES z next to it: the terms kernel reads the
// same z back (4 B/element written and read once) instead of running Philox + Box-Muller a second time per element.
template <bool VEC>
__global__ __launch_bounds__(256) void bpd_xt_kernel(const float* __restrict__ x0, const float* __restrict__ coef, int idx,
                                                     int batch, long per_sample, long groups, uint64_t seed,
                                                     uint64_t sample_offset, uint32_t step, float* __restrict__ z_out,
                                                     float* __restrict__ xt_out) {
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= groups * batch) return;
    const Group g = group_of<VEC>(gid, groups, per_sample);
    const float sa = coef[(long)idx * 8 + 5], s1m = coef[(long)idx * 8 + 6];
    const f32x4 z = philox_normal4(seed, sample_offset + (uint64_t)g.b, step, g.grp);
    const f32x4 x = load4<VEC>(x0, g.e0, g.nval);
    f32x4 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = q_sample_value(sa, s1m, x[i], z[i]);
    store4<VEC>(z_out, g.e0, g.nval, z);
    store4<VEC>(xt_out, g.e0, g.nval, r);
}

struct BpdDev {
    StepSrc s;              // x = x_t; out unused
    int chunks;
    const float *x0, *z, *mean;
    int prior;
    float prior_lv;
    float* part;
};

// approx_standard_normal_cdf (losses.py:42-47); th.pow(x, 3) is x*x*x
__device__ __forceinline__ float bpd_cdf(float x) {
    const float x3 = __fmul_rn(__fmul_rn(x, x), x);
    const float u = __fmul_rn(0.7978845608028654f, __fadd_rn(x, __fmul_rn(0.044715f, x3)));
    return __fmul_rn(0.5f, __fadd_rn(1.0f, tanhf(u)));
}

constexpr int BPD_GROUPS = GDX_BPD_CHUNK / 4;      // float4 groups per block: 256 threads x 4 groups

// One block = one GDX_BPD_CHUNK-element slice of one sample (grid (chunks, B)): per-thread partial sums of the three
// quantities in element order, wave64 shuffle reduction, the four waves through LDS, then ONE ordinary store of the
// block's three sums to part[(b*chunks + chunk)*4 ..]; bpd_finish_kernel adds a sample's chunks in sequence.  The
// summation order is a function of J*T alone, so a sample's numbers do not depend on the batch around it.
template <bool VEC>
__global__ __launch_bounds__(256) void bpd_terms_kernel(const BpdDev a) {
    __shared__ float red[4][3];
    const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
    const long idx = coef_row(a.s, b);
    const float* c = a.s.coef + idx * 8;
    const float pm1 = c[0], pm2 = c[1], lv1 = c[2], lv2 = c[3], sra = c[4], sa = c[5], srm1 = c[7];
    // the per-step scalars of normal_kl / the decoder term, in torch's op order on the expanded fp32 tables
    const float klc = a.prior ? __fadd_rn(__fsub_rn(-1.0f, a.prior_lv), expf(a.prior_lv))
                              : __fadd_rn(__fsub_rn(__fadd_rn(-1.0f, lv2), lv1), expf(__fsub_rn(lv1, lv2)));
    const float e2 = expf(-lv2);
    const float inv_std = expf(-__fmul_rn(0.5f, lv2));
    const float bin = (float)(1.0 / 255.0);
    const bool first = idx == 0;
    float s_vb = 0.0f, s_x = 0.0f, s_e = 0.0f;
    for (int it = 0; it < BPD_GROUPS / 256; ++it) {
        const long grp = (long)chunk * BPD_GROUPS + it * 256 + tid;
        if (grp >= a.s.groups) break;
        const Group g = group_at<VEC>(b, grp, a.s.per_sample);
        const long e0 = g.e0;
        const int nval = g.nval;
        const f32x4 x0 = load4<VEC>(a.x0, e0, nval);
        if (a.prior) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float m = __fmul_rn(sa, x0[i]);
                if (i < nval) s_vb = __fadd_rn(s_vb, __fmul_rn(0.5f, __fadd_rn(klc, __fmul_rn(m, m))));
            }
            continue;
        }
        const f32x4 xt = load4<VEC>(a.s.x, e0, nval);
        const f32x4 p = pred_xstart4<VEC>(a.s, g);
        const f32x4 z = a.z ? load4<VEC>(a.z, e0, nval) : f32x4{0.f, 0.f, 0.f, 0.f};
        f32x4 mm;
        if (a.mean) {
            mm = load4<VEC>(a.mean, e0, nval);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) mm[i] = posterior_mean(pm1, pm2, p[i], xt[i]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float v;
            if (first) {            // discretized_gaussian_log_likelihood (losses.py:50-77), block-uniform branch
                const float cx = __fsub_rn(x0[i], mm[i]);
                const float cp = bpd_cdf(__fmul_rn(inv_std, __fadd_rn(cx, bin)));
                const float cm = bpd_cdf(__fmul_rn(inv_std, __fsub_rn(cx, bin)));
                const float lp = x0[i] < -0.999f ? logf(fmaxf(cp, 1e-12f))
                               : (x0[i] > 0.999f ? logf(fmaxf(__fsub_rn(1.0f, cm), 1e-12f))
                                                 : logf(fmaxf(__fsub_rn(cp, cm), 1e-12f)));
                v = -lp;
            } else {                // normal_kl (losses.py:33-39)
                const float mt = posterior_mean(pm1, pm2, x0[i], xt[i]);
                const float dm = __fsub_rn(mt, mm[i]);
                v = __fmul_rn(0.5f, __fadd_rn(klc, __fmul_rn(__fmul_rn(dm, dm), e2)));
            }
            const float dx = __fsub_rn(p[i], x0[i]);
            const float eps = eps_from_xstart(sra, srm1, xt[i], p[i]);
            const float de = __fsub_rn(eps, z[i]);
            if (i < nval) {
                s_vb = __fadd_rn(s_vb, v);
                s_x = __fadd_rn(s_x, __fmul_rn(dx, dx));
                s_e = __fadd_rn(s_e, __fmul_rn(de, de));
            }
        }
        if (a.s.pred) store4<VEC>(a.s.pred, e0, nval, p);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s_vb = __fadd_rn(s_vb, __shfl_down(s_vb, off, 64));
        s_x = __fadd_rn(s_x, __shfl_down(s_x, off, 64));
        s_e = __fadd_rn(s_e, __shfl_down(s_e, off, 64));
    }
    if ((tid & 63) == 0) { red[tid >> 6][0] = s_vb; red[tid >> 6][1] = s_x; red[tid >> 6][2] = s_e; }
    __syncthreads();
    if (tid < 3) {
        const float s = __fadd_rn(__fadd_rn(__fadd_rn(red[0][tid], red[1][tid]), red[2][tid]), red[3][tid]);
        a.part[((long)b * a.chunks + chunk) * 4 + tid] = s;
    }
}

// out[b*ld + col] = (sum of the sample's chunk sums, in chunk order) / (J*T)  [ / ln 2 for the bound ]: mean_flat(.) / np.log(2.0)
__global__ void bpd_finish_kernel(const float* __restrict__ part, int chunks, long per_sample, int batch, float* vb,
                                  float* xs, float* mse, int ld, int col) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= batch * 3) return;
    const int b = i / 3, q = i % 3;
    float* out = q == 0 ? vb : (q == 1 ? xs : mse);
    if (!out) return;
    float s = 0.0f;
    for (int ch = 0; ch < chunks; ++ch) s = __fadd_rn(s, part[((long)b * chunks + ch) * 4 + q]);
    float m = __fdiv_rn(s, (float)per_sample);
    if (q == 0) m = __fdiv_rn(m, 0.6931471805599453f);
    out[(long)b * ld + col] = m;
}

// ---------------------------------------------------------------------------------------------------------------
// Guidance rescale (Lin et al. 2023, arXiv:2305.08891 section 3.4; gdx.h gdx_cfg_rescale): the guided output g = cfg_blend(c, u, s)
// of a sample scaled by f = phi * std(c)/std(g) + (1 - phi).  Three launches: per-chunk sums of c, c^2, g, g^2 in fp64 (an fp32
// value widens exactly and its square is exact in fp64, so only the additions round), the sample's factor, the streaming pass.
// A sample is guided when t == NULL or lo <= t[b] <= hi; an unguided one keeps c and gets the factor 1.
struct CfgRescaleDev {
    long per_sample, groups;
    int chunks, batch;
    const float *c, *u, *scale;
    const float* g;                  // the guided prediction already formed (gdx_cfg_rescale_), or nullptr: cfg_blend(c, u, scale)
    const int64_t* t;
    int64_t lo, hi;
    double phi;
    double* part;
    float *factor, *out;
};
__device__ __forceinline__ bool rescale_guided(const CfgRescaleDev& a, int b) {
    if (!a.t) return true;
    const int64_t tb = a.t[b];
    return a.lo <= tb && tb <= a.hi;
}
// the guided prediction of a guided sample's group whose conditional output is c
template <bool VEC>
__device__ __forceinline__ f32x4 rescale_g4(const CfgRescaleDev& a, const f32x4 c, int b, long e0, int nval) {
    if (a.g) return load4<VEC>(a.g, e0, nval);
    const f32x4 u = load4<VEC>(a.u, e0, nval);
    const float sc = a.scale[b];
    f32x4 g;
#pragma unroll
    for (int i = 0; i < 4; ++i) g[i] = cfg_blend(c[i], u[i], sc);
    return g;
}

// bpd_terms_kernel's decomposition and summation order (grid (chunks, B), thread -> wave -> block -> one ordinary store of the
// block's four sums to part[(b*chunks + chunk)*4 ..]): a function of J*T alone, no atomics.
template <bool VEC>
__global__ __launch_bounds__(256) void cfg_rescale_stats_kernel(const CfgRescaleDev a) {
    __shared__ double red[4][4];
    const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
    if (!rescale_guided(a, b)) return;                             // block-uniform
    const long base = (long)b * a.per_sample;
    double s[4] = {0.0, 0.0, 0.0, 0.0};                            // sum c, sum c^2, sum g, sum g^2
    for (int it = 0; it < BPD_GROUPS / 256; ++it) {
        const long grp = (long)chunk * BPD_GROUPS + it * 256 + tid;
        if (grp >= a.groups) break;
        const long e0 = base + 4L * grp;
        const int nval = VEC ? 4 : (int)min(4L, a.per_sample - 4L * grp);
        const f32x4 c = load4<VEC>(a.c, e0, nval);
        const f32x4 g = rescale_g4<VEC>(a, c, b, e0, nval);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i < nval) {
                const double dc = (double)c[i], dg = (double)g[i];
                s[0] = __dadd_rn(s[0], dc);
                s[1] = __dadd_rn(s[1], __dmul_rn(dc, dc));
                s[2] = __dadd_rn(s[2], dg);
                s[3] = __dadd_rn(s[3], __dmul_rn(dg, dg));
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int q = 0; q < 4; ++q) s[q] = __dadd_rn(s[q], __shfl_down(s[q], off, 64));
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) red[tid >> 6][q] = s[q];
    }
    __syncthreads();
    if (tid < 4)
        a.part[((long)b * a.chunks + chunk) * 4 + tid] =
            __dadd_rn(__dadd_rn(__dadd_rn(red[0][tid], red[1][tid]), red[2][tid]), red[3][tid]);
}

// One thread per sample: the chunk sums in chunk order, then f = (float)(phi * sqrt(SS_c / SS_g) + (1 - phi)) with
// SS = max(Q - S^2/N, 0), all in fp64 and rounded once.  SS_g == 0 (a constant guided output) gives 1; a NaN or infinity in the
// sample makes SS NaN, which passes both comparisons and reaches f.
__global__ void cfg_rescale_factor_kernel(const CfgRescaleDev a) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.batch) return;
    if (!rescale_guided(a, b)) { a.factor[b] = 1.0f; return; }
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int ch = 0; ch < a.chunks; ++ch) {
#pragma unroll
        for (int q = 0; q < 4; ++q) s[q] = __dadd_rn(s[q], a.part[((long)b * a.chunks + ch) * 4 + q]);
    }
    const double n = (double)a.per_sample;
    double ss_c = __dsub_rn(s[1], __ddiv_rn(__dmul_rn(s[0], s[0]), n));
    double ss_g = __dsub_rn(s[3], __ddiv_rn(__dmul_rn(s[2], s[2]), n));
    if (ss_c < 0.0) ss_c = 0.0;
    if (ss_g < 0.0) ss_g = 0.0;
    const double r = ss_g == 0.0 ? 1.0 : __dsqrt_rn(__ddiv_rn(ss_c, ss_g));
    a.factor[b] = (float)__dadd_rn(__dmul_rn(a.phi, r), __dsub_rn(1.0, a.phi));
}

// out = guided ? g * f : c, grid (ceil(groups / 256), B) like dpm_step_kernel; out may alias c (a thread reads its group first)
template <bool VEC>
__global__ __launch_bounds__(256) void cfg_rescale_apply_kernel(const CfgRescaleDev a) {
    const long grp = (long)blockIdx.x * 256 + threadIdx.x;
    if (grp >= a.groups) return;
    const Group g = group_at<VEC>(blockIdx.y, grp, a.per_sample);
    f32x4 x0 = load4<VEC>(a.c, g.e0, g.nval);
    if (rescale_guided(a, g.b)) {
        const f32x4 gp = rescale_g4<VEC>(a, x0, g.b, g.e0, g.nval);
        const float f = a.factor[g.b];
#pragma unroll
        for (int i = 0; i < 4; ++i) x0[i] = __fmul_rn(gp[i], f);
    }
    store4<VEC>(a.out, g.e0, g.nval, x0);
}

// Guidance refresh (gdx.h gdx_cfg_delta): out = fl32(a - b) over `count` elements, the one pass behind both uses -- storing the
// guidance difference d = c - u on a refresh call and forming u' = c - d on a reuse call.  A thread handles groups of four
// consecutive elements, grid-strided; VEC: count % 4 == 0 and every pointer 16-byte aligned, else the scalar form, whose last
// group holds count % 4 elements.  out may alias b (no __restrict__: a thread reads its group before it writes it, and no other
// thread touches that group).
template <bool VEC>
__global__ __launch_bounds__(256) void cfg_delta_kernel(const float* a, const float* b, float* out, long count, long groups) {
    const long stride = (long)gridDim.x * 256;
    for (long grp = (long)blockIdx.x * 256 + threadIdx.x; grp < groups; grp += stride) {
        const long e0 = 4L * grp;
        const int nval = VEC ? 4 : (int)min(4L, count - e0);
        const f32x4 x = load4<VEC>(a, e0, nval), y = load4<VEC>(b, e0, nval);
        f32x4 r;
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i] = __fsub_rn(x[i], y[i]);
        store4<VEC>(out, e0, nval, r);
    }
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

hipError_t launch_cfg_blend(const float* c, const float* u, const float* scale, const int64_t* t, int64_t lo, int64_t hi,
                            float* out, int B, int64_t per_sample, hipStream_t s) {
    const long total = (long)B * per_sample;
    hipLaunchKernelGGL(cfg_blend_kernel, dim3((total + 255) / 256), dim3(256), 0, s, c, u, scale, t, lo, hi, out,
                       (long)per_sample, total);
    return hipGetLastError();
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

// 0, or -1 with `msg` ("<entry>: launch failed") recorded, from the status of the launch just made
static int launch_status(const char* msg) { return hipGetLastError() == hipSuccess ? 0 : gdx_set_error_(msg); }

// May a pose-layout kernel take its VEC = true instantiation: whole groups only, and every operand it reads or writes by
// group (nullptr = absent) aligned for the group access -- 16 bytes for floats, 4 for mask bytes.
static inline bool group_aligned(const float* p) { return !((uintptr_t)p & 15); }
static inline bool group_aligned(const uint8_t* p) { return !((uintptr_t)p & 3); }
template <typename... P>
static bool vec_ok(long per_sample, const P*... p) { return per_sample % 4 == 0 && (group_aligned(p) && ...); }
// ... of a kernel over a StepSrc: its operands and whatever else (`more`) the kernel reads or writes by group
template <typename... P>
static bool vec_ok(const gdx::StepSrc& s, const P*... more) {
    return vec_ok(s.per_sample, s.x, s.x0c, s.x0u, s.mask, s.motion, s.out, s.pred, more...);
}

hipError_t gdx::launch_cfg_compose(const float* f, const float* m, const float* u, const float* s0, const float* s1, const int64_t* t,
                                   int64_t lo, int64_t hi, float* out, int B, int64_t per_sample, hipStream_t s) {
    CfgComposeDev d{(long)per_sample, (long)(per_sample + 3) / 4, f, m, u, s0, s1, t, lo, hi, out};
    if (B <= 0 || per_sample <= 0) return hipSuccess;
    const dim3 grid((unsigned)((d.groups + 255) / 256), (unsigned)B), block(256);
    if (vec_ok(d.per_sample, f, m, u, out)) hipLaunchKernelGGL(cfg_compose_kernel<true>, grid, block, 0, s, d);
    else hipLaunchKernelGGL(cfg_compose_kernel<false>, grid, block, 0, s, d);
    return hipGetLastError();
}

static int refuse(const char* who, const char* what) { return gdx_set_error_((std::string(who) + ": " + what).c_str()); }

// The kernels' StepSrc from an entry's argument struct (every step struct names these fields alike); pred: where x0 goes
template <typename A>
static gdx::StepSrc step_src(const A* a, float* pred) {
    gdx::StepSrc s;
    s.per_sample = (long)a->njoints * a->frames;
    s.groups = (s.per_sample + 3) / 4;
    s.coef = a->coef; s.t = a->t; s.step_index = a->step_index;
    s.x = a->x; s.x0c = a->x0_cond; s.x0u = a->x0_uncond; s.scale = a->scale;
    s.mask = a->inpaint_mask; s.motion = a->inpaint_motion; s.clip = a->clip_denoised;
    s.out = a->out; s.pred = pred;
    return s;
}

// What gdx_plms_step, gdx_dpm_step, gdx_dpm_sde_step and gdx_unipc_step (`who`) share in front of their launch: the refusals in their order
// -- null argument, the entry's own kind / order check, shape, CFG, mask, the entry's history check (both return the
// refusal's text or nullptr) --, then the StepSrc and the (ceil(groups / 256), B) grid.  -1: refused, 1: nothing to do, 0: launch.
template <typename A, typename Entry, typename Hist>
static int step_begin(const char* who, const A* a, float* A::*pred, Entry entry_check, Hist hist_check, gdx::StepSrc& s, dim3& grid) {
    if (!a || !a->coef || !a->x || !a->x0_cond || !a->out) return refuse(who, "null argument");
    if (const char* m = entry_check()) return refuse(who, m);
    if (a->batch < 0 || a->njoints < 0 || a->frames < 0 || a->batch > 65535) return refuse(who, "bad shape");
    if (a->x0_uncond && !a->scale) return refuse(who, "CFG needs scale");
    if (a->inpaint_mask && !a->inpaint_motion) return refuse(who, "mask without motion");
    if (const char* m = hist_check()) return refuse(who, m);
    s = step_src(a, a->*pred);
    if (a->batch == 0 || s.per_sample == 0) return 1;
    grid = dim3((unsigned)((s.groups + 255) / 256), (unsigned)a->batch);
    return 0;
}

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
    const dim3 grid((total + 255) / 256), block(256);
    if (vec_ok(d.s, d.noise, d.grad))
        hipLaunchKernelGGL(update_kernel<true>, grid, block, 0, (hipStream_t)stream, d);
    else
        hipLaunchKernelGGL(update_kernel<false>, grid, block, 0, (hipStream_t)stream, d);
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

extern "C" int gdx_masked_l2(const float* a, const float* b, const uint8_t* mask, float* out, int32_t batch,
                             int32_t njoints, int32_t frames, void* stream) {
    if (!a || !b || !mask || !out) return gdx_set_error_("gdx_masked_l2: null argument");
    if (batch <= 0 || njoints <= 0 || frames <= 0) return 0;
    hipLaunchKernelGGL(gdx::masked_l2_kernel, dim3(batch), dim3(256), 0, (hipStream_t)stream, a, b, mask, out, njoints,
                       frames);
    return launch_status("gdx_masked_l2: launch failed");
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

template <bool VEC>
static void launch_plms_step(int kind, dim3 grid, hipStream_t s, const gdx::PlmsStepDev& d) {
    using namespace gdx;
    const dim3 block(256);
    switch (kind) {
        case 1: hipLaunchKernelGGL((plms_step_kernel<1, VEC>), grid, block, 0, s, d); break;
        case 2: hipLaunchKernelGGL((plms_step_kernel<2, VEC>), grid, block, 0, s, d); break;
        case 3: hipLaunchKernelGGL((plms_step_kernel<3, VEC>), grid, block, 0, s, d); break;
        case 4: hipLaunchKernelGGL((plms_step_kernel<4, VEC>), grid, block, 0, s, d); break;
        case 5: hipLaunchKernelGGL((plms_step_kernel<5, VEC>), grid, block, 0, s, d); break;
        default: hipLaunchKernelGGL((plms_step_kernel<6, VEC>), grid, block, 0, s, d); break;
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
    if (vec_ok(d.s, d.x_eps, d.e1, d.e2, d.e3, d.pred_prev, d.eps_out)) launch_plms_step<true>(k, grid, (hipStream_t)stream, d);
    else launch_plms_step<false>(k, grid, (hipStream_t)stream, d);
    return launch_status("gdx_plms_step: launch failed");
}

template <bool NOISE, bool VEC>
static void launch_dpm_step(int nh, dim3 grid, hipStream_t s, const gdx::DpmStepDev& d) {
    using namespace gdx;
    const dim3 block(256);
    if (nh == 0) hipLaunchKernelGGL((dpm_step_kernel<0, NOISE, VEC>), grid, block, 0, s, d);
    else if (NOISE || nh == 1) hipLaunchKernelGGL((dpm_step_kernel<1, NOISE, VEC>), grid, block, 0, s, d);
    else hipLaunchKernelGGL((dpm_step_kernel<2, false, VEC>), grid, block, 0, s, d);
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
    if (vec_ok(d.s, d.m1, d.m2, d.noise)) launch_dpm_step<NOISE, true>(nh, grid, (hipStream_t)stream, d);
    else launch_dpm_step<NOISE, false>(nh, grid, (hipStream_t)stream, d);
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

template <bool VEC>
static void launch_unipc_step(int nc, int np, dim3 grid, hipStream_t s, const gdx::UnipcStepDev& d) {
    using namespace gdx;
    const dim3 block(256);
    switch (nc * 4 + np) {
        case 0 * 4 + 1: hipLaunchKernelGGL((unipc_step_kernel<0, 1, VEC>), grid, block, 0, s, d); break;
        case 1 * 4 + 1: hipLaunchKernelGGL((unipc_step_kernel<1, 1, VEC>), grid, block, 0, s, d); break;
        case 1 * 4 + 2: hipLaunchKernelGGL((unipc_step_kernel<1, 2, VEC>), grid, block, 0, s, d); break;
        case 2 * 4 + 2: hipLaunchKernelGGL((unipc_step_kernel<2, 2, VEC>), grid, block, 0, s, d); break;
        case 3 * 4 + 2: hipLaunchKernelGGL((unipc_step_kernel<3, 2, VEC>), grid, block, 0, s, d); break;
        case 2 * 4 + 3: hipLaunchKernelGGL((unipc_step_kernel<2, 3, VEC>), grid, block, 0, s, d); break;
        default: hipLaunchKernelGGL((unipc_step_kernel<3, 3, VEC>), grid, block, 0, s, d); break;
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
    if (vec_ok(d.s, d.h0, d.h1, d.h2, d.base_out)) launch_unipc_step<true>(a->corr_order, a->pred_order, grid, (hipStream_t)stream, d);
    else launch_unipc_step<false>(a->corr_order, a->pred_order, grid, (hipStream_t)stream, d);
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
    const dim3 block(256);
    if (vec_ok(d.s, d.eps_out)) hipLaunchKernelGGL(ddim_reverse_step_kernel<true>, grid, block, 0, (hipStream_t)stream, d);
    else hipLaunchKernelGGL(ddim_reverse_step_kernel<false>, grid, block, 0, (hipStream_t)stream, d);
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
    d.chunks = (int)((s.per_sample + GDX_BPD_CHUNK - 1) / GDX_BPD_CHUNK);
    d.planes = planes; d.x0 = x0; d.noise = noise; d.plane = (long)batch * s.per_sample;
    d.seed = philox_seed; d.sample_offset = sample_offset; d.rng_step = rng_step;
    d.part = workspace;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(d.chunks, batch), block(BPD_GROUPS);
    // per_sample % 4 == 0 keeps every plane / slot / tape slice as aligned as its base
    if (vec_ok(s.per_sample, (const float*)planes, x0, noise, inpaint_mask, inpaint_motion))
        hipLaunchKernelGGL(window_sweep_kernel<true>, grid, block, 0, st, d);
    else
        hipLaunchKernelGGL(window_sweep_kernel<false>, grid, block, 0, st, d);
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

extern "C" int gdx_bpd_terms(const gdx_bpd_args_t* a, void* stream) {
    using namespace gdx;
    if (!a) return gdx_set_error_("gdx_bpd_terms: null argument");
    if (!a->coef || !a->x_start || !a->workspace) return gdx_set_error_("gdx_bpd_terms: null argument");
    if (a->batch < 0 || a->njoints < 0 || a->frames < 0 || a->batch > 65535) return gdx_set_error_("gdx_bpd_terms: bad shape");
    if (a->prior) {
        if (!a->vb) return gdx_set_error_("gdx_bpd_terms: the prior term needs vb");
    } else {
        if (!a->x_t || !a->x0_cond) return gdx_set_error_("gdx_bpd_terms: null argument");
        if (a->x0_uncond && !a->scale) return gdx_set_error_("gdx_bpd_terms: CFG needs scale");
        if (a->inpaint_mask && !a->inpaint_motion) return gdx_set_error_("gdx_bpd_terms: mask without motion");
        if (a->mse && !a->noise) return gdx_set_error_("gdx_bpd_terms: mse needs noise");
    }
    if (a->ld <= 0 || a->col < 0 || a->col >= a->ld) return gdx_set_error_("gdx_bpd_terms: bad output column");
    BpdDev d;
    StepSrc& s = d.s;
    s.per_sample = (long)a->njoints * a->frames;
    s.groups = (s.per_sample + 3) / 4;
    d.chunks = (int)((s.per_sample + GDX_BPD_CHUNK - 1) / GDX_BPD_CHUNK);
    if (a->batch == 0 || s.per_sample == 0) return 0;
    s.coef = a->coef; s.t = a->t; s.step_index = a->step_index;
    s.x = a->x_t; s.x0c = a->x0_cond; s.x0u = a->x0_uncond; s.scale = a->scale;
    s.mask = a->inpaint_mask; s.motion = a->inpaint_motion; s.clip = a->clip_denoised;
    s.out = nullptr; s.pred = a->prior ? nullptr : a->pred_xstart;
    d.x0 = a->x_start; d.z = a->noise; d.mean = a->model_mean;
    d.prior = a->prior; d.prior_lv = a->prior_log_variance; d.part = a->workspace;
    // mask / motion are read by group through pred_xstart4 like everywhere else: a mask not 4-byte aligned or a motion tensor
    // not 16-byte aligned selects the scalar instantiation, which gives the same bits
    const dim3 grid(d.chunks, a->batch), block(256);
    if (vec_ok(s, d.x0, d.z, d.mean)) hipLaunchKernelGGL(bpd_terms_kernel<true>, grid, block, 0, (hipStream_t)stream, d);
    else hipLaunchKernelGGL(bpd_terms_kernel<false>, grid, block, 0, (hipStream_t)stream, d);
    if (launch_status("gdx_bpd_terms: launch failed")) return -1;
    hipLaunchKernelGGL(bpd_finish_kernel, dim3((a->batch * 3 + 63) / 64), dim3(64), 0, (hipStream_t)stream, d.part, d.chunks,
                       s.per_sample, a->batch, a->vb, a->prior ? nullptr : a->xstart_mse, a->prior ? nullptr : a->mse, a->ld,
                       a->col);
    return launch_status("gdx_bpd_terms: launch failed");
}

extern "C" int gdx_cfg_rescale(const gdx_cfg_rescale_args_t* a, void* stream) { return gdx_cfg_rescale_(a, nullptr, stream); }

int gdx_cfg_rescale_(const gdx_cfg_rescale_args_t* a, const float* g, void* stream) {
    using namespace gdx;
    if (!a) return gdx_set_error_("gdx_cfg_rescale: null argument");
    if (!a->x0_cond || (!g && (!a->x0_uncond || !a->scale)) || !a->workspace || !a->factor || !a->out)
        return gdx_set_error_("gdx_cfg_rescale: null argument");
    if (a->batch <= 0 || a->njoints <= 0 || a->frames <= 0 || a->batch > 65535) return gdx_set_error_("gdx_cfg_rescale: bad shape");
    if (!(a->phi >= 0.0f && a->phi <= 1.0f)) return gdx_set_error_("gdx_cfg_rescale: phi must lie in [0, 1]");
    if ((uintptr_t)a->workspace & 7) return gdx_set_error_("gdx_cfg_rescale: workspace not 8-byte aligned");
    CfgRescaleDev d;
    d.per_sample = (long)a->njoints * a->frames;
    d.groups = (d.per_sample + 3) / 4;
    d.chunks = (int)((d.per_sample + GDX_BPD_CHUNK - 1) / GDX_BPD_CHUNK);
    d.batch = a->batch;
    d.c = a->x0_cond; d.u = a->x0_uncond; d.scale = a->scale; d.g = g;
    d.t = a->t; d.lo = a->lo; d.hi = a->hi;
    d.phi = (double)a->phi;
    d.part = a->workspace; d.factor = a->factor; d.out = a->out;
    hipStream_t s = (hipStream_t)stream;
    const dim3 block(256);
    if (vec_ok(d.per_sample, d.c, d.u, d.g)) hipLaunchKernelGGL(cfg_rescale_stats_kernel<true>, dim3(d.chunks, a->batch), block, 0, s, d);
    else hipLaunchKernelGGL(cfg_rescale_stats_kernel<false>, dim3(d.chunks, a->batch), block, 0, s, d);
    if (launch_status("gdx_cfg_rescale: launch failed")) return -1;
    hipLaunchKernelGGL(cfg_rescale_factor_kernel, dim3((a->batch + 63) / 64), dim3(64), 0, s, d);
    if (launch_status("gdx_cfg_rescale: launch failed")) return -1;
    const dim3 grid((unsigned)((d.groups + 255) / 256), (unsigned)a->batch);
    if (vec_ok(d.per_sample, d.c, d.u, d.g, d.out)) hipLaunchKernelGGL(cfg_rescale_apply_kernel<true>, grid, block, 0, s, d);
    else hipLaunchKernelGGL(cfg_rescale_apply_kernel<false>, grid, block, 0, s, d);
    return launch_status("gdx_cfg_rescale: launch failed");
}

extern "C" int gdx_cfg_delta(const gdx_cfg_delta_args_t* a, void* stream) {
    using namespace gdx;
    if (!a) return gdx_set_error_("gdx_cfg_delta: null argument");
    if (!a->a || !a->b || !a->out) return gdx_set_error_("gdx_cfg_delta: null argument");
    if (a->count <= 0) return gdx_set_error_("gdx_cfg_delta: count must be positive");
    const long count = (long)a->count, groups = (count + 3) / 4;
    // memory-bound: at most 2048 blocks, the rest grid-strided
    const dim3 grid((unsigned)std::min(2048L, (groups + 255) / 256)), block(256);
    if (vec_ok(count, a->a, a->b, a->out)) hipLaunchKernelGGL(cfg_delta_kernel<true>, grid, block, 0, (hipStream_t)stream, a->a, a->b, a->out, count, groups);
    else hipLaunchKernelGGL(cfg_delta_kernel<false>, grid, block, 0, (hipStream_t)stream, a->a, a->b, a->out, count, groups);
    return launch_status("gdx_cfg_delta: launch failed");
}

// internal (loops.hip, gdx_bpd_loop): x_t and the stored Philox noise of one step (bpd_xt_kernel)
int gdx_bpd_xt_(const float* x0, const float* coef, int idx, int batch, long per_sample, uint64_t seed, uint64_t sample_offset,
                uint32_t step, float* z_out, float* xt_out, void* stream) {
    using namespace gdx;
    const long groups = (per_sample + 3) / 4, total = groups * batch;
    if (total == 0) return 0;
    const dim3 grid((total + 255) / 256), block(256);
    if (vec_ok(per_sample, x0, z_out, xt_out))
        hipLaunchKernelGGL(bpd_xt_kernel<true>, grid, block, 0, (hipStream_t)stream, x0, coef, idx, batch, per_sample, groups, seed,
                           sample_offset, step, z_out, xt_out);
    else
        hipLaunchKernelGGL(bpd_xt_kernel<false>, grid, block, 0, (hipStream_t)stream, x0, coef, idx, batch, per_sample, groups,
                           seed, sample_offset, step, z_out, xt_out);
    return launch_status("gdx_bpd_loop: x_t launch failed");
}
