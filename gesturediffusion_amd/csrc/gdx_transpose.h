// The pose-tensor -> token-major transpose in front of the input GEMM, one definition for the fp32 instance (boundary.hip)
// and the 16-bit ones (boundaryh.hip).  32x32 tiles through LDS, coalesced on both sides.
//   x [Bsrc, J, T]  -> xt [(b*T + t)*ldx + j], b < B (source sample b % Bsrc), columns j >= J zeroed
#pragma once
#include <hip/hip_runtime.h>

namespace gdx {

template <typename OutT>
__global__ __launch_bounds__(256) void transpose_in_kernel(const float* __restrict__ x, OutT* __restrict__ xt, int Bsrc,
                                                           int J, int T, int ldx) {
    __shared__ float tile[32][33];
    const int b = blockIdx.z, t0 = blockIdx.x * 32, j0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;           // 32 x 8
    const float* xb = x + (long)(b % Bsrc) * J * T;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int j = j0 + ty + 8 * r, t = t0 + tx;
        tile[ty + 8 * r][tx] = (j < J && t < T) ? xb[(long)j * T + t] : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int t = t0 + ty + 8 * r, j = j0 + tx;
        if (t < T && j < ldx) xt[((long)b * T + t) * ldx + j] = (OutT)tile[tx][ty + 8 * r];
    }
}

}  // namespace gdx
