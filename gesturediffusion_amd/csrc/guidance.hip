// The guidance arithmetic on the pose layout [B][J*T], outside the step kernels: the classifier-free blend of two forwards, the
// per-condition 3-pass composition, the guidance rescale and the guidance-refresh difference.  Every product, sum and difference
// is rounded on its own in the reference's order; contraction is off in this file (gdx_pose_device.h).
#include <algorithm>

#include "gdx_pose_device.h"
#include "gdx_pose_host.h"

namespace gdx {

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
// Perturbed-attention guidance stacked on classifier-free guidance (gdx.h gdx_set_attention_guidance, GDX_PAG_CFG), m = the
// perturbed pass P: g = (u + s0*(f - u)) + s1*(f - m), rounded like the rule above
__device__ __forceinline__ float cfg_compose_pag(float f, float m, float u, float s0, float s1) {
    return __fadd_rn(cfg_blend(f, u, s0), __fmul_rn(s1, __fsub_rn(f, m)));
}
template <bool VEC, int RULE>
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
        for (int i = 0; i < 4; ++i)
            x0[i] = RULE == COMPOSE_PAG ? cfg_compose_pag(x0[i], m[i], u[i], s0, s1) : cfg_compose(x0[i], m[i], u[i], s0, s1);
    }
    store4<VEC>(a.out, g.e0, g.nval, x0);
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

// bpd_terms_kernel's (bound.hip) decomposition and summation order (grid (chunks, B), thread -> wave -> block -> one ordinary store
// of the block's four sums to part[(b*chunks + chunk)*4 ..]): a function of J*T alone, no atomics.
template <bool VEC>
__global__ __launch_bounds__(256) void cfg_rescale_stats_kernel(const CfgRescaleDev a) {
    __shared__ double red[4][4];
    const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
    if (!rescale_guided(a, b)) return;                             // block-uniform
    double s[4] = {0.0, 0.0, 0.0, 0.0};                            // sum c, sum c^2, sum g, sum g^2
    for (int it = 0; it < BPD_GROUPS / 256; ++it) {
        const long grp = (long)chunk * BPD_GROUPS + it * 256 + tid;
        if (grp >= a.groups) break;
        const Group gr = group_at<VEC>(b, grp, a.per_sample);
        const long e0 = gr.e0;
        const int nval = gr.nval;
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

hipError_t launch_cfg_blend(const float* c, const float* u, const float* scale, const int64_t* t, int64_t lo, int64_t hi,
                            float* out, int B, int64_t per_sample, hipStream_t s) {
    const long total = (long)B * per_sample;
    hipLaunchKernelGGL(cfg_blend_kernel, dim3((total + 255) / 256), dim3(256), 0, s, c, u, scale, t, lo, hi, out,
                       (long)per_sample, total);
    return hipGetLastError();
}

hipError_t launch_cfg_compose(const float* f, const float* m, const float* u, const float* s0, const float* s1, const int64_t* t,
                              int64_t lo, int64_t hi, float* out, int B, int64_t per_sample, hipStream_t s, int rule) {
    CfgComposeDev d{(long)per_sample, (long)(per_sample + 3) / 4, f, m, u, s0, s1, t, lo, hi, out};
    if (B <= 0 || per_sample <= 0) return hipSuccess;
    const dim3 grid((unsigned)((d.groups + 255) / 256), (unsigned)B);
    const bool vec = vec_ok(d.per_sample, f, m, u, out);
    if (rule == COMPOSE_PAG)
        launch_vec(vec, cfg_compose_kernel<true, COMPOSE_PAG>, cfg_compose_kernel<false, COMPOSE_PAG>, grid, dim3(256), s, d);
    else
        launch_vec(vec, cfg_compose_kernel<true, COMPOSE_CHAIN>, cfg_compose_kernel<false, COMPOSE_CHAIN>, grid, dim3(256), s, d);
    return hipGetLastError();
}
}  // namespace gdx

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
    d.chunks = (int)bpd_chunks(d.per_sample);
    d.batch = a->batch;
    d.c = a->x0_cond; d.u = a->x0_uncond; d.scale = a->scale; d.g = g;
    d.t = a->t; d.lo = a->lo; d.hi = a->hi;
    d.phi = (double)a->phi;
    d.part = a->workspace; d.factor = a->factor; d.out = a->out;
    hipStream_t s = (hipStream_t)stream;
    const dim3 block(256);
    launch_vec(vec_ok(d.per_sample, d.c, d.u, d.g), cfg_rescale_stats_kernel<true>, cfg_rescale_stats_kernel<false>,
               dim3(d.chunks, a->batch), block, s, d);
    if (launch_status("gdx_cfg_rescale: launch failed")) return -1;
    hipLaunchKernelGGL(cfg_rescale_factor_kernel, dim3((a->batch + 63) / 64), dim3(64), 0, s, d);
    if (launch_status("gdx_cfg_rescale: launch failed")) return -1;
    const dim3 grid((unsigned)((d.groups + 255) / 256), (unsigned)a->batch);
    launch_vec(vec_ok(d.per_sample, d.c, d.u, d.g, d.out), cfg_rescale_apply_kernel<true>, cfg_rescale_apply_kernel<false>, grid,
               block, s, d);
    return launch_status("gdx_cfg_rescale: launch failed");
}

extern "C" int gdx_cfg_delta(const gdx_cfg_delta_args_t* a, void* stream) {
    using namespace gdx;
    if (!a) return gdx_set_error_("gdx_cfg_delta: null argument");
    if (!a->a || !a->b || !a->out) return gdx_set_error_("gdx_cfg_delta: null argument");
    if (a->count <= 0) return gdx_set_error_("gdx_cfg_delta: count must be positive");
    const long count = (long)a->count, groups = (count + 3) / 4;
    // memory-bound: at most 2048 blocks, the rest grid-strided
    const dim3 grid((unsigned)std::min(2048L, (groups + 255) / 256));
    launch_vec(vec_ok(count, a->a, a->b, a->out), cfg_delta_kernel<true>, cfg_delta_kernel<false>, grid, dim3(256),
               (hipStream_t)stream, a->a, a->b, a->out, count, groups);
    return launch_status("gdx_cfg_delta: launch failed");
}
