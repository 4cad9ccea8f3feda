// LayerNorm over the last dim (post-norm encoder: model/mdm.py:90-96 -> norm1/norm2, eps 1e-5, biased variance) with the
// residual add fused in: out = LN(x + res).  One wave per row, four rows per block, two-pass mean / variance, wave shuffles
// for the reduce.  Four kernels -- fp32 or 16-bit input, row in registers (vector loads) or re-read (any d) -- that share the
// token-0 compaction, the variance pass and the affine expression below; each keeps its own loads with its own first-pass
// summation order, and its own stores.  The helpers are cut where the compiler's output stays what it was with every kernel
// written out (tools/isa_compare.py): the bounds check and `orow = row` stay in the kernels, and layernorm_h_gen_kernel, whose
// schedule moves with either, spells out the compaction and the affine expression.
#include "gdx_internal.h"
#include "gdx_device.h"

namespace gdx {
GDX_HNS_BEGIN

// compact_S > 0 drops token 0 of every sample, [B, S, d] -> [B, S-1, d]: the output row of input row `row`; false: token 0
__device__ __forceinline__ bool ln_compact(int row, int compact_S, long& orow) {
    const int b = row / compact_S;
    if (row - b * compact_S == 0) return false;
    orow = row - b - 1;
    return true;
}

// Second pass: an element's squared deviation ...
__device__ __forceinline__ float ln_sq(float x, float mean) {
    const float c = x - mean;
    return c * c;
}
// ... and 1 / sqrt(biased variance + eps) from the lanes' sums of them
__device__ __forceinline__ float ln_rstd(float q, int d) { return 1.0f / sqrtf(wave_sum(q) / (float)d + 1e-5f); }

__device__ __forceinline__ float ln_affine(float v, float mean, float rstd, float g, float b) {
    return (v - mean) * rstd * g + b;
}

// fp32 in, fp32 and / or 16-bit out (each optional).  HBM-bound: 3 * rows * d * 4 bytes.
template <int VPL>   // float4 per lane: d = 256 * VPL
__global__ __launch_bounds__(256) void layernorm_vec_kernel(const float* __restrict__ x, const float* __restrict__ res,
                                                             const float* __restrict__ g,
                                                             const float* __restrict__ bta, float* __restrict__ out,
                                                             half_t* __restrict__ out16, int rows, int d,
                                                             int compact_S) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);   // one wave per row
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    long orow = row;
    if (compact_S > 0 && !ln_compact(row, compact_S, orow)) return;
    const f32x4* xp = reinterpret_cast<const f32x4*>(x + (long)row * d);
    const f32x4* rp = reinterpret_cast<const f32x4*>(res + (long)row * d);
    f32x4 v[VPL];
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        v[i] = xp[lane + 64 * i];
        if (res) v[i] += rp[lane + 64 * i];
        s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
    }
    const float mean = wave_sum(s) / (float)d;
    float q = 0.0f;
#pragma unroll
    for (int i = 0; i < VPL; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) q += ln_sq(v[i][e], mean);
    const float rstd = ln_rstd(q, d);
    f32x4* op = reinterpret_cast<f32x4*>(out + orow * d);
    f16x4* hp = reinterpret_cast<f16x4*>(out16 + orow * d);
    const f32x4* gp = reinterpret_cast<const f32x4*>(g);
    const f32x4* bp = reinterpret_cast<const f32x4*>(bta);
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        const f32x4 gg = gp[lane + 64 * i], bb = bp[lane + 64 * i];
        f32x4 r;
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = ln_affine(v[i][e], mean, rstd, gg[e], bb[e]);
        if (out) op[lane + 64 * i] = r;
        if (out16) hp[lane + 64 * i] = f16x4{(half_t)r[0], (half_t)r[1], (half_t)r[2], (half_t)r[3]};
    }
}

// generic d (multiple of 32, <= 2048): scalar lane-strided loads
__global__ __launch_bounds__(256) void layernorm_gen_kernel(const float* __restrict__ x, const float* __restrict__ res,
                                                             const float* __restrict__ g,
                                                             const float* __restrict__ bta, float* __restrict__ out,
                                                             half_t* __restrict__ out16, int rows, int d,
                                                             int compact_S) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);   // one wave per row
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    long orow = row;
    if (compact_S > 0 && !ln_compact(row, compact_S, orow)) return;
    const float* xp = x + (long)row * d;
    const float* rp = res + (long)row * d;
    float s = 0.0f;
    for (int e = lane; e < d; e += 64) s += res ? xp[e] + rp[e] : xp[e];
    const float mean = wave_sum(s) / (float)d;
    float q = 0.0f;
    for (int e = lane; e < d; e += 64) q += ln_sq(res ? xp[e] + rp[e] : xp[e], mean);
    const float rstd = ln_rstd(q, d);
    for (int e = lane; e < d; e += 64) {
        const float r = ln_affine(res ? xp[e] + rp[e] : xp[e], mean, rstd, g[e], bta[e]);
        if (out) out[orow * d + e] = r;
        if (out16) out16[orow * d + e] = (half_t)r;
    }
}

hipError_t launch_layernorm(const float* x, const float* res, const float* gamma, const float* beta, float* out,
                            _Float16* out16_, int rows, int d, int compact_S, hipStream_t s) {
    half_t* out16 = reinterpret_cast<half_t*>(out16_);
    const dim3 grid((rows + 3) / 4), block(256);
    if (d == 512)
        hipLaunchKernelGGL(layernorm_vec_kernel<2>, grid, block, 0, s, x, res, gamma, beta, out, out16, rows, d, compact_S);
    else if (d == 1024)
        hipLaunchKernelGGL(layernorm_vec_kernel<4>, grid, block, 0, s, x, res, gamma, beta, out, out16, rows, d, compact_S);
    else if (d == 256)
        hipLaunchKernelGGL(layernorm_vec_kernel<1>, grid, block, 0, s, x, res, gamma, beta, out, out16, rows, d, compact_S);
    else
        hipLaunchKernelGGL(layernorm_gen_kernel, grid, block, 0, s, x, res, gamma, beta, out, out16, rows, d, compact_S);
    return hipGetLastError();
}

// fp16-mode LayerNorm: x and the residual are fp16 (the whole activation stream of the fp16 mode is fp16), statistics
// and the affine transform are fp32, output fp16 (+ optional fp32 copy for the parity taps).  8 halves (16 B) per lane per
// load.  HBM-bound: 3 * rows * d * 2 bytes.
template <int NV>   // 16-byte loads per lane: d = 512 * NV
__global__ __launch_bounds__(256) void layernorm_h_vec_kernel(const half_t* __restrict__ x, const half_t* __restrict__ res,
                                                               const float* __restrict__ g, const float* __restrict__ bta,
                                                               half_t* __restrict__ out16, float* __restrict__ out32,
                                                               int rows, int d, int compact_S) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);   // one wave per row
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    long orow = row;
    if (compact_S > 0 && !ln_compact(row, compact_S, orow)) return;
    const f16x8* xp = reinterpret_cast<const f16x8*>(x + (long)row * d);
    const f16x8* rp = reinterpret_cast<const f16x8*>(res + (long)row * d);
    float v[NV][8];
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const f16x8 a = xp[lane + 64 * i];
        f16x8 r = f16x8{0, 0, 0, 0, 0, 0, 0, 0};
        if (res) r = rp[lane + 64 * i];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            v[i][e] = (float)a[e] + (float)r[e];
            s += v[i][e];
        }
    }
    const float mean = wave_sum(s) / (float)d;
    float q = 0.0f;
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int e = 0; e < 8; ++e) q += ln_sq(v[i][e], mean);
    const float rstd = ln_rstd(q, d);
    const f32x4* gp = reinterpret_cast<const f32x4*>(g);
    const f32x4* bp = reinterpret_cast<const f32x4*>(bta);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c4 = 2 * (lane + 64 * i);
        const f32x4 g0 = gp[c4], g1 = gp[c4 + 1], b0 = bp[c4], b1 = bp[c4 + 1];
        float r[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            r[e] = ln_affine(v[i][e], mean, rstd, g0[e], b0[e]);
            r[4 + e] = ln_affine(v[i][4 + e], mean, rstd, g1[e], b1[e]);
        }
        reinterpret_cast<f16x8*>(out16 + orow * d)[lane + 64 * i] =
            f16x8{(half_t)r[0], (half_t)r[1], (half_t)r[2], (half_t)r[3], (half_t)r[4], (half_t)r[5], (half_t)r[6], (half_t)r[7]};
        if (out32) {
            f32x4* op = reinterpret_cast<f32x4*>(out32 + orow * d);
            op[c4] = f32x4{r[0], r[1], r[2], r[3]};
            op[c4 + 1] = f32x4{r[4], r[5], r[6], r[7]};
        }
    }
}

__global__ __launch_bounds__(256) void layernorm_h_gen_kernel(const half_t* __restrict__ x, const half_t* __restrict__ res,
                                                               const float* __restrict__ g, const float* __restrict__ bta,
                                                               half_t* __restrict__ out16, float* __restrict__ out32,
                                                               int rows, int d, int compact_S) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);   // one wave per row
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    long orow = row;
    if (compact_S > 0) {                 // ln_compact, spelled out (see the top of the file)
        const int b = row / compact_S;
        if (row - b * compact_S == 0) return;
        orow = row - b - 1;
    }
    const half_t* xp = x + (long)row * d;
    const half_t* rp = res + (long)row * d;
    auto at = [&](int e) { return res ? (float)xp[e] + (float)rp[e] : (float)xp[e]; };
    float s = 0.0f;
    for (int e = lane; e < d; e += 64) s += at(e);
    const float mean = wave_sum(s) / (float)d;
    float q = 0.0f;
    for (int e = lane; e < d; e += 64) q += ln_sq(at(e), mean);
    const float rstd = ln_rstd(q, d);
    for (int e = lane; e < d; e += 64) {
        float r = (at(e) - mean) * rstd * g[e] + bta[e];   // ln_affine, spelled out
        // out16 is r rounded: without the barrier the compiler fuses the last multiply-add into the 16-bit conversion
        // (v_fma_mixlo_f16, one rounding from the exact value), which disagrees with out32 rounded on ~1e-4 of the elements
        asm volatile("" : "+v"(r));
        out16[orow * d + e] = (half_t)r;
        if (out32) out32[orow * d + e] = r;
    }
}

hipError_t launch_layernorm_f16(const _Float16* x_, const _Float16* res_, const float* gamma, const float* beta,
                                _Float16* out16_, float* out32, int rows, int d, int compact_S, hipStream_t s) {
    const half_t* x = reinterpret_cast<const half_t*>(x_);
    const half_t* res = reinterpret_cast<const half_t*>(res_);
    half_t* out16 = reinterpret_cast<half_t*>(out16_);
    const dim3 grid((rows + 3) / 4), block(256);
    if (d == 512)
        hipLaunchKernelGGL(layernorm_h_vec_kernel<1>, grid, block, 0, s, x, res, gamma, beta, out16, out32, rows, d, compact_S);
    else if (d == 1024)
        hipLaunchKernelGGL(layernorm_h_vec_kernel<2>, grid, block, 0, s, x, res, gamma, beta, out16, out32, rows, d, compact_S);
    else
        hipLaunchKernelGGL(layernorm_h_gen_kernel, grid, block, 0, s, x, res, gamma, beta, out16, out32, rows, d, compact_S);
    return hipGetLastError();
}

GDX_HNS_END
}  // namespace gdx
