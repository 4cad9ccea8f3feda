// Device side of the pose-layout kernels (sampler.hip, guidance.hip, bound.hip): the in-kernel noise generator, the
// group accessors and every bit-pinned formula that more than one of those files uses.
//
// CONTRACTION OFF.  Products and sums are rounded separately (__fmul_rn/__fadd_rn, never contracted into FMA) in the reference's
// operation order, so given the same operands a result is bit-identical to the torch expression.  HIP's __fmul_rn/__fadd_rn are
// plain * and + and hipcc defaults to -ffp-contract=fast, so bit-exactness depends on no mul+add pair being fused anywhere in a
// file that uses these helpers.  One rule says so twice: the pragma below covers the rest of every translation unit that includes
// this header, and the Makefile compiles exactly the including files (EXACT_SRCS) with -ffp-contract=off;
// tests/test_host_logic.py holds the two lists together.  A kernel with a bit-pinned formula belongs in a file that includes this
// header, and nowhere else.
#pragma once
#pragma clang fp contract(off)

#include "gdx_internal.h"
#include "gdx_device.h"
#include "../../include/gdx.h"

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
// kernel calls it: two kernels agree bit for bit because they run the same statements, not because two copies were kept in
// step.  Each product / sum / quotient is its own __fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn in torch's op order.  A helper
// that one kernel family alone uses stays next to that family, in a file that includes this header.

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

// float4 groups per GDX_BPD_CHUNK-element chunk, the unit of every per-sample sum (bound.hip, guidance.hip: 256 threads x 4
// groups; window_sweep_kernel: 1024 threads, one group each)
constexpr int BPD_GROUPS = GDX_BPD_CHUNK / 4;

}  // namespace gdx
