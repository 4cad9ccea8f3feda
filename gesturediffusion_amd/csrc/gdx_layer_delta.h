// The row-remapped delta pass of the layer cache (gdx.h, gdx_set_layer_cache / gdx_layer_delta), one definition for the fp32
// instance (boundary.hip) and the 16-bit ones (boundaryh.hip).  Row (b, t) of the compact side ([B, T, d]: the output GEMM's
// operand and the stored change) pairs with row (b, t + 1) of the [B, T+1, d] residual stream, token 0 skipped:
//   store: delta[b,t,j] = fl32(outc[b,t,j] - in[b,t+1,j])
//   apply: outc[b,t,j]  = (TO) fl32(in[b,t+1,j] + delta[b,t,j])
// 16-bit elements are widened to fp32 first.  HBM-bound streaming: a thread owns groups of eight consecutive columns (d % 32
// == 0 and 16-byte aligned bases make every access a whole 128-bit one; there is no scalar path), grid-strided.
#pragma once
#include <hip/hip_runtime.h>

namespace gdx {

template <typename T>
struct Octet {   // eight consecutive elements of a row as fp32
    typedef T v8 __attribute__((ext_vector_type(8)));
    static __device__ __forceinline__ void load(const T* p, float (&v)[8]) {
        const v8 x = *reinterpret_cast<const v8*>(p);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (float)x[i];
    }
    static __device__ __forceinline__ void store(T* p, const float (&v)[8]) {
        v8 x;
#pragma unroll
        for (int i = 0; i < 8; ++i) x[i] = (T)v[i];
        *reinterpret_cast<v8*>(p) = x;
    }
};
template <>
struct Octet<float> {
    typedef float v4 __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ void load(const float* p, float (&v)[8]) {
        const v4 a = *reinterpret_cast<const v4*>(p), b = *reinterpret_cast<const v4*>(p + 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) { v[i] = a[i]; v[4 + i] = b[i]; }
    }
    static __device__ __forceinline__ void store(float* p, const float (&v)[8]) {
        *reinterpret_cast<v4*>(p) = v4{v[0], v[1], v[2], v[3]};
        *reinterpret_cast<v4*>(p + 4) = v4{v[4], v[5], v[6], v[7]};
    }
};

// groups = B * T * d8 octets of the compact side, d8 = d / 8.  No __restrict__ claims beyond the read-only side: outc and delta
// are each read or written depending on APPLY.
template <typename TI, typename TO, bool APPLY>
__global__ __launch_bounds__(256) void layer_delta_kernel(const TI* __restrict__ in, TO* outc, float* delta, int T, int d8,
                                                          long groups) {
    const long stride = (long)gridDim.x * 256;
    for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < groups; g += stride) {
        const long row = g / d8, b = row / T;
        const long ie = ((row + b + 1) * d8 + (g - row * d8)) * 8, oe = g * 8;
        float x[8], y[8], r[8];
        Octet<TI>::load(in + ie, x);
        if (APPLY) {
            Octet<float>::load(delta + oe, y);
#pragma unroll
            for (int i = 0; i < 8; ++i) r[i] = __fadd_rn(x[i], y[i]);
            Octet<TO>::store(outc + oe, r);
        } else {
            Octet<TO>::load(outc + oe, y);
#pragma unroll
            for (int i = 0; i < 8; ++i) r[i] = __fsub_rn(y[i], x[i]);
            Octet<float>::store(delta + oe, r);
        }
    }
}

template <typename TI, typename TO>
hipError_t launch_layer_delta_t(int op, const TI* in, TO* outc, float* delta, int B, int T, int d, hipStream_t s) {
    const long groups = (long)B * T * (d / 8);
    if (groups <= 0) return hipSuccess;
    // memory-bound: at most 2048 blocks, the rest grid-strided
    const dim3 grid((unsigned)(groups + 255 < 2048L * 256 ? (groups + 255) / 256 : 2048)), block(256);
    if (op) hipLaunchKernelGGL((layer_delta_kernel<TI, TO, true>), grid, block, 0, s, in, outc, delta, T, d / 8, groups);
    else hipLaunchKernelGGL((layer_delta_kernel<TI, TO, false>), grid, block, 0, s, in, outc, delta, T, d / 8, groups);
    return hipGetLastError();
}

}  // namespace gdx
