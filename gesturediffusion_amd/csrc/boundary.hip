// fp32 kernels at the boundary of the denoiser step: the pose-tensor <-> token-major transposes, the small per-sample
// linears (timestep / seed embedding), the timestep row gather and the MFCC projection hoisted out of the loop.
// (Their 16-bit neighbours -- the conditioning token, the 16-bit transpose and the converts -- are in boundaryh.hip.)
#include "gdx_internal.h"
#include "gdx_device.h"
#include "gdx_transpose.h"
#include "gdx_layer_delta.h"

namespace gdx {

// ---------------------------------------------------------------------------------------------
// Pose-tensor <-> token-major transposes around the boundary GEMMs (model/mdm.py:350-356 InputProcess permute,
// :372-380 OutputProcess permute).  32x32 tiles through LDS, coalesced on both sides.  ~26 MB each way at
// config 2: a few microseconds, and they let both boundary linears run on the persistent GEMM.
//   in : gdx_transpose.h
//   out: yt [(b*T + t)*ldy + j] -> y [(b*J + j)*T + t]
__global__ __launch_bounds__(256) void transpose_out_kernel(const float* __restrict__ yt, float* __restrict__ y, int J,
                                                            int T, int ldy) {
    __shared__ float tile[32][33];
    const int b = blockIdx.z, t0 = blockIdx.x * 32, j0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int t = t0 + ty + 8 * r, j = j0 + tx;
        tile[ty + 8 * r][tx] = (t < T && j < J) ? yt[((long)b * T + t) * ldy + j] : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int j = j0 + ty + 8 * r, t = t0 + tx;
        if (j < J && t < T) y[((long)b * J + j) * T + t] = tile[tx][ty + 8 * r];
    }
}

hipError_t launch_transpose_in(const float* x, float* xt, int B, int Bsrc, int J, int T, int ldx, hipStream_t s) {
    const dim3 grid((T + 31) / 32, (ldx + 31) / 32, B);
    hipLaunchKernelGGL(transpose_in_kernel<float>, grid, dim3(256), 0, s, x, xt, Bsrc, J, T, ldx);
    return hipGetLastError();
}

hipError_t launch_transpose_out(const float* yt, float* y, int B, int J, int T, int ldy, hipStream_t s) {
    const dim3 grid((T + 31) / 32, (J + 31) / 32, B);
    hipLaunchKernelGGL(transpose_out_kernel, grid, dim3(256), 0, s, yt, y, J, T, ldy);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Small-M linear (timestep MLP model/mdm.py:296-310, seed-pose encoder :382-392, the per-sample
// coarse-vector slice of project_to_lat :154-169).  M is the batch (<= a few hundred rows): pure
// latency, one wave per output element, lane-strided coalesced K loop, shuffle reduce.
__global__ __launch_bounds__(256) void small_linear_kernel(const float* __restrict__ A, int lda,
                                                            const float* __restrict__ W, int ldw,
                                                            const float* __restrict__ bias, float* __restrict__ out,
                                                            int ldo, int M, int N, int K, int act) {
    const int n = blockIdx.x;
    const int m = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (m >= M) return;
    const float* a = A + (long)m * lda;
    const float* w = W + (long)n * ldw;
    float s = 0.0f;
    for (int k = lane; k < K; k += 64) s = fmaf(a[k], w[k], s);
    s = wave_sum(s);
    if (lane == 0) {
        if (bias) s += bias[n];
        if (act == 1) s = s / (1.0f + expf(-s));   // SiLU
        out[(long)m * ldo + n] = s;
    }
}

hipError_t launch_small_linear(const float* A, int lda, const float* W, int ldw, const float* bias, float* out,
                               int ldo, int M, int N, int K, int act, hipStream_t s) {
    const dim3 grid(N, (M + 3) / 4), block(256);
    hipLaunchKernelGGL(small_linear_kernel, grid, block, 0, s, A, lda, W, ldw, bias, out, ldo, M, N, K, act);
    return hipGetLastError();
}

__global__ void gather_rows_kernel(const float* __restrict__ table, const int64_t* __restrict__ idx,
                                   float* __restrict__ out, int M, int d, int max_rows) {
    const int m = blockIdx.x;
    long r = idx[m];
    r = r < 0 ? 0 : (r >= max_rows ? max_rows - 1 : r);
    for (int e = threadIdx.x; e < d; e += blockDim.x) out[(long)m * d + e] = table[r * d + e];
}

hipError_t launch_gather_rows(const float* table, const int64_t* idx, float* out, int M, int d, int max_rows,
                              hipStream_t s) {
    hipLaunchKernelGGL(gather_rows_kernel, dim3(M), dim3(256), 0, s, table, idx, out, M, d, max_rows);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Step-invariant MFCC slice of the input linear (V1: model/mdm_old.py:104-108 concatenates the 26
// MFCC channels onto the pose channels before InputProcess; V2: model/mdm.py:151-169 feeds them to
// project_to_lat).  Computed once per conditioning, not once per step:
//   out[b,t,n] = sum_c mfcc[b,c,t] * W[n][c] + bias[n] (+ pe[t+1][n])
// One thread owns output column n for a run of ROWS (sample, frame) rows: its C <= 32 weights W[n][0..C) sit in registers
// (read once, as one contiguous run per thread), a row's C MFCC values are wave-uniform (scalar loads) and the stores are
// coalesced along n.  (The first version recomputed everything per output element: every thread re-read its weight row
// with a 128-byte stride for each of its outputs -- 6.5 ms at config 5 against 0.2 ms for this one; same fmaf chain, c
// ascending, so the results are bit-identical.)
__global__ __launch_bounds__(256) void mfcc_project_kernel(const float* __restrict__ mfcc, const float* __restrict__ W,
                                                           int ldw, const float* __restrict__ bias,
                                                           const float* __restrict__ pe, float* __restrict__ out,
                                                           int B, int Bsrc, int C, int T, int d, int rps, int off, int rows_per_block) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    const long row0 = (long)blockIdx.y * rows_per_block;
    const long nrows = (long)B * T;
    if (n >= d) return;
    float w[32];
#pragma unroll
    for (int c = 0; c < 32; ++c) w[c] = c < C ? W[(long)n * ldw + c] : 0.0f;
    const float bn = bias[n];
    for (long bt = row0; bt < row0 + rows_per_block && bt < nrows; ++bt) {
        const int t = bt % T, b = bt / T;
        const float* m = mfcc + ((long)(b % Bsrc) * C) * T + t;
        float s = 0.0f;
#pragma unroll
        for (int c = 0; c < 32; ++c)
            if (c < C) s = fmaf(m[(long)c * T], w[c], s);
        s += bn;
        if (pe) s += pe[(long)(t + 1) * d + n];
        out[((long)b * rps + t + off) * d + n] = s;
    }
}

hipError_t launch_mfcc_project(const float* mfcc, const float* W, int ldw, const float* bias, const float* pe,
                               float* out, int B, int Bsrc, int C, int T, int d, int rps, int off, hipStream_t s) {
    if (C > 32) return hipErrorInvalidValue;                      // gdx_create caps mfcc_dim at 32
    const long nrows = (long)B * T;
    if (nrows <= 0) return hipSuccess;
    const int rpb = 64;
    hipLaunchKernelGGL(mfcc_project_kernel, dim3((d + 255) / 256, (unsigned)((nrows + rpb - 1) / rpb)), dim3(256), 0, s, mfcc, W,
                       ldw, bias, pe, out, B, Bsrc, C, T, d, rps, off, rpb);
    return hipGetLastError();
}

// layer cache, fp32 residual stream and fp32 operand (gdx_layer_delta.h)
hipError_t launch_layer_delta(int op, const float* in, float* outc, float* delta, int B, int T, int d, hipStream_t s) {
    return launch_layer_delta_t<float, float>(op, in, outc, delta, B, T, d, s);
}

}  // namespace gdx
