// The boundary kernels of the denoiser step that write or read half_t: the conditioning token (fp32 + optional 16-bit copy),
// the pose-tensor -> token-major transpose into a 16-bit operand and the two converts.  Built once per 16-bit type; the
// fp32-only boundary kernels are in boundary.hip.
#include "gdx_internal.h"
#include "gdx_device.h"
#include "gdx_transpose.h"
#include "gdx_layer_delta.h"

namespace gdx {
GDX_HNS_BEGIN

hipError_t launch_transpose_in_f16(const float* x, _Float16* xt_, int B, int Bsrc, int J, int T, int ldx, hipStream_t s) {
    half_t* xt = reinterpret_cast<half_t*>(xt_);
    const dim3 grid((T + 31) / 32, (ldx + 31) / 32, B);
    hipLaunchKernelGGL(transpose_in_kernel<half_t>, grid, dim3(256), 0, s, x, xt, Bsrc, J, T, ldx);
    return hipGetLastError();
}

// conditioning token (model/mdm_old.py:94-111: emb_t + emb_seed, then + pe[0]; model/mdm.py:154-160,197)
__global__ void token0_kernel(const float* __restrict__ temb, int tstride, const float* __restrict__ seed_emb,
                              const float* __restrict__ pe0, float* __restrict__ enc, half_t* __restrict__ enc16,
                              const float* __restrict__ c2t, const float* __restrict__ c2_seed, float* __restrict__ c2,
                              const int* __restrict__ state, int B, int Bsrc, int S, int d) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * d) return;
    const int b = i / d, n = i % d;
    if (state) {                            // graph replay: temb / c2t are table bases, the row comes from device memory
        temb += (long)state[0] * d;
        if (c2t) c2t += (long)state[0] * d;
    }
    const long trow = (long)(b % Bsrc) * tstride + n;
    float v = temb[trow] + seed_emb[i];
    if (c2) c2[i] = c2t[trow] + c2_seed[i];       // coarse slice of project_to_lat: W_coa temb + W_coa seed_emb
    if (pe0) v += pe0[n];
    enc[(long)b * S * d + n] = v;
    if (enc16) enc16[(long)b * S * d + n] = (half_t)v;
}

hipError_t launch_token0(const float* temb, int tstride, const float* seed_emb, const float* pe0, float* enc,
                         _Float16* enc16_, const float* c2t, const float* c2_seed, float* c2, const int* state, int B,
                         int Bsrc, int S, int d, hipStream_t s) {
    half_t* enc16 = reinterpret_cast<half_t*>(enc16_);
    hipLaunchKernelGGL(token0_kernel, dim3((B * d + 255) / 256), dim3(256), 0, s, temb, tstride, seed_emb, pe0, enc,
                       enc16, c2t, c2_seed, c2, state, B, Bsrc, S, d);
    return hipGetLastError();
}

__global__ void convert_f16_kernel(const float* __restrict__ src, half_t* __restrict__ dst, int64_t n) {
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i + 3 < n) {
        const float4 v = *reinterpret_cast<const float4*>(src + i);
        typedef half_t h4 __attribute__((ext_vector_type(4)));
        *reinterpret_cast<h4*>(dst + i) = h4{(half_t)v.x, (half_t)v.y, (half_t)v.z, (half_t)v.w};
    } else {
        for (int64_t k = i; k < n; ++k) dst[k] = (half_t)src[k];
    }
}

__global__ void convert_f32_kernel(const half_t* __restrict__ src, float* __restrict__ dst, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = (float)src[i];
}

hipError_t launch_convert_f32(const _Float16* src_, float* dst, int64_t n, hipStream_t s) {
    const half_t* src = reinterpret_cast<const half_t*>(src_);
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(convert_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, dst, n);
    return hipGetLastError();
}

hipError_t launch_convert_f16(const float* src, _Float16* dst_, int64_t n, hipStream_t s) {
    half_t* dst = reinterpret_cast<half_t*>(dst_);
    if (n <= 0) return hipSuccess;
    const int64_t nth = (n + 3) / 4;
    hipLaunchKernelGGL(convert_f16_kernel, dim3((unsigned)((nth + 255) / 256)), dim3(256), 0, s, src, dst, n);
    return hipGetLastError();
}

// layer cache with a 16-bit operand (gdx_layer_delta.h): the residual stream in the build's half_t, or fp32 (in32: the bf16
// mode's fp32 stream)
hipError_t launch_layer_delta_h(int op, bool in32, const void* in, _Float16* outc_, float* delta, int B, int T, int d,
                                hipStream_t s) {
    half_t* outc = reinterpret_cast<half_t*>(outc_);
    if (in32) return launch_layer_delta_t<float, half_t>(op, static_cast<const float*>(in), outc, delta, B, T, d, s);
    return launch_layer_delta_t<half_t, half_t>(op, static_cast<const half_t*>(in), outc, delta, B, T, d, s);
}

GDX_HNS_END
}  // namespace gdx
