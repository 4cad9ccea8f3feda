// The variational bound's per-step terms on the pose layout (gdx.h gdx_bpd_terms; gdx_bpd_loop's x_t kernel) and the masked L2 of
// the training loss.  Contraction is off in this file (gdx_pose_device.h): the bound's terms are pinned to the reference's torch
// expressions, and masked_l2_kernel's s += d * d * m would round differently as an FMA.
#include "gdx_pose_device.h"
#include "gdx_pose_host.h"

namespace gdx {

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
}  // namespace gdx

extern "C" int gdx_masked_l2(const float* a, const float* b, const uint8_t* mask, float* out, int32_t batch,
                             int32_t njoints, int32_t frames, void* stream) {
    if (!a || !b || !mask || !out) return gdx_set_error_("gdx_masked_l2: null argument");
    if (batch <= 0 || njoints <= 0 || frames <= 0) return 0;
    hipLaunchKernelGGL(gdx::masked_l2_kernel, dim3(batch), dim3(256), 0, (hipStream_t)stream, a, b, mask, out, njoints,
                       frames);
    return launch_status("gdx_masked_l2: launch failed");
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
    d.chunks = (int)bpd_chunks(s.per_sample);
    if (a->batch == 0 || s.per_sample == 0) return 0;
    s.coef = a->coef; s.t = a->t; s.step_index = a->step_index;
    s.x = a->x_t; s.x0c = a->x0_cond; s.x0u = a->x0_uncond; s.scale = a->scale;
    s.mask = a->inpaint_mask; s.motion = a->inpaint_motion; s.clip = a->clip_denoised;
    s.out = nullptr; s.pred = a->prior ? nullptr : a->pred_xstart;
    d.x0 = a->x_start; d.z = a->noise; d.mean = a->model_mean;
    d.prior = a->prior; d.prior_lv = a->prior_log_variance; d.part = a->workspace;
    // mask / motion are read by group through pred_xstart4 like everywhere else: a mask not 4-byte aligned or a motion tensor
    // not 16-byte aligned selects the scalar instantiation, which gives the same bits
    launch_vec(vec_ok(s, d.x0, d.z, d.mean), bpd_terms_kernel<true>, bpd_terms_kernel<false>, dim3(d.chunks, a->batch), dim3(256),
               (hipStream_t)stream, d);
    if (launch_status("gdx_bpd_terms: launch failed")) return -1;
    hipLaunchKernelGGL(bpd_finish_kernel, dim3((a->batch * 3 + 63) / 64), dim3(64), 0, (hipStream_t)stream, d.part, d.chunks,
                       s.per_sample, a->batch, a->vb, a->prior ? nullptr : a->xstart_mse, a->prior ? nullptr : a->mse, a->ld,
                       a->col);
    return launch_status("gdx_bpd_terms: launch failed");
}

// internal (loops.hip, gdx_bpd_loop): x_t and the stored Philox noise of one step (bpd_xt_kernel)
int gdx_bpd_xt_(const float* x0, const float* coef, int idx, int batch, long per_sample, uint64_t seed, uint64_t sample_offset,
                uint32_t step, float* z_out, float* xt_out, void* stream) {
    using namespace gdx;
    const long groups = (per_sample + 3) / 4, total = groups * batch;
    if (total == 0) return 0;
    launch_vec(vec_ok(per_sample, x0, z_out, xt_out), bpd_xt_kernel<true>, bpd_xt_kernel<false>, dim3((total + 255) / 256), dim3(256),
               (hipStream_t)stream, x0, coef, idx, batch, per_sample, groups, seed, sample_offset, step, z_out, xt_out);
    return launch_status("gdx_bpd_loop: x_t launch failed");
}
