// The fused V2 front end (RoPE -> causal local attention -> RoPE at t+1), one wave per (sample, local head, window): the
// scalar fp32 kernel for any shape, the fp32-MFMA kernel, and the 16-bit-MFMA kernel of the half modes.
//
// The two MFMA kernels are twins in their work decode, their mask + softmax, the prefetch of the second rotary's table rows and
// the second rotary + stores; they differ in the fragment type, the layout of the parked key rows, the exponential and which
// output is optional.  The twin parts are NOT factored out: each of the four as a __forceinline__ helper changes the
// compiler's schedule of at least three of the five instantiations (the softmax one also the register counts, 68 -> 84 VGPRs
// for local_attention_h_kernel<64>).  A change to one of those parts goes into both kernels.
#include "gdx_internal.h"
#include "gdx_device.h"

namespace gdx {
GDX_HNS_BEGIN

// ---------------------------------------------------------------------------------------------
// V2 front end, one wave per (sample, local head, window):
//   rotary embedding (NeoX half-split, model/local_attention.py:43-62) of the <= 2*window rows it needs,
//   causal windowed attention with q = k = v (model/local_attention.py:92-172 as configured at
//   model/mdm.py:72-80: look back one window, scale e^-0.5, padded look-back keys masked),
//   second rotary at position t+1 (model/mdm.py:197-213; token 0 sits at position 0 where the
//   rotation is the identity), result written straight into the encoder input [B, T+1, d].
// All intermediates live in LDS; nothing but xseq is read and enc_in written.
__global__ __launch_bounds__(64) void local_attention_kernel(const float* __restrict__ xseq,
                                                             const float* __restrict__ cosT,
                                                             const float* __restrict__ sinT, float* __restrict__ enc,
                                                             half_t* __restrict__ enc16, int T, int d, int heads,
                                                             int window) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int e = d / heads, half = e >> 1;
    const int nwin = T / window;
    const int w = blockIdx.x % nwin;
    const int head = (blockIdx.x / nwin) % heads;
    const int b = blockIdx.x / (nwin * heads);
    const int lane = threadIdx.x;
    const int k0 = w == 0 ? 0 : (w - 1) * window;
    const int q0 = w * window;
    const int nkeys = q0 + window - k0;          // window or 2*window
    const int es = e + 1;                        // padded row stride
    float* xr = sm;                              // [nkeys][es]   rotated rows
    float* sc = xr + 2 * window * es;            // [window][2*window] scores / probabilities
    float* ob = sc + window * 2 * window;        // [window][es]  attention output

    const float* xb = xseq + ((long)b * T) * d + head * e;
    for (int i = lane; i < nkeys * e; i += 64) {
        const int r = i / e, c = i % e;
        const int pos = k0 + r;
        const float* row = xb + (long)pos * d;
        const float x = row[c];
        const float rot = c < half ? -row[c + half] : row[c - half];
        const int f = c < half ? c : c - half;
        xr[r * es + c] = x * cosT[pos * half + f] + rot * sinT[pos * half + f];
    }
    __syncthreads();
    const float scale = 1.0f / sqrtf((float)e);
    for (int p = lane; p < window * nkeys; p += 64) {
        const int qi = p / nkeys, kj = p % nkeys;
        const float* qr = xr + (q0 - k0 + qi) * es;
        const float* kr = xr + kj * es;
        float s = 0.0f;
        for (int c = 0; c < e; ++c) s = fmaf(qr[c], kr[c], s);
        s *= scale;
        if (k0 + kj > q0 + qi) s = -INFINITY;    // causal
        sc[qi * 2 * window + kj] = s;
    }
    __syncthreads();
    if (lane < window) {
        float* r = sc + lane * 2 * window;
        float mx = -INFINITY;
        for (int k = 0; k < nkeys; ++k) mx = fmaxf(mx, r[k]);
        float sum = 0.0f;
        for (int k = 0; k < nkeys; ++k) {
            r[k] = expf(r[k] - mx);
            sum += r[k];
        }
        const float inv = 1.0f / sum;
        for (int k = 0; k < nkeys; ++k) r[k] *= inv;
    }
    __syncthreads();
    for (int i = lane; i < window * e; i += 64) {
        const int qi = i / e, c = i % e;
        const float* pr = sc + qi * 2 * window;
        float s = 0.0f;
        for (int k = 0; k < nkeys; ++k) s = fmaf(pr[k], xr[k * es + c], s);
        ob[qi * es + c] = s;
    }
    __syncthreads();
    float* eb = enc + ((long)b * (T + 1)) * d + head * e;
    for (int i = lane; i < window * e; i += 64) {
        const int qi = i / e, c = i % e;
        const int pos = q0 + qi + 1;             // position in the [token | frames] sequence
        const float x = ob[qi * es + c];
        const float rot = c < half ? -ob[qi * es + c + half] : ob[qi * es + c - half];
        const int f = c < half ? c : c - half;
        const float v = x * cosT[pos * half + f] + rot * sinT[pos * half + f];
        eb[(long)pos * d + c] = v;
        if (enc16) enc16[((long)b * (T + 1) + pos) * d + head * e + c] = (half_t)v;
    }
}

// The same front end on the fp32 MFMA (v_mfma_f32_16x16x4_f32), one wave per (sample, local head, window), four waves per
// block -- the structure of local_attention_h_kernel below with fp32 fragments:
//   * a lane loads float4 pieces of "its" row (row l15 of a 16-row block, head-dim 16kk + 4lq .. +3), so both halves of a
//     rotary pair sit in the same lane; the rotated pieces are directly the fragments of S^T = K Q^T (k-slot lq of k-step
//     (kk, e) <-> head-dim 16kk + 4lq + e, the same map for both operands);
//   * the rotated key rows are parked in LDS (row stride E + 4 floats: the four k-slots of a V^T fragment read land 16
//     banks apart); the queries ARE key rows q0 - k0 .., read back from there;
//   * softmax on the accumulator layout (query on the lane axis, keys 4lq + r in the registers): register r of the
//     probability tile is the B operand of the PV k-step whose slot lq holds key 4lq + r -- no cross-lane movement;
//   * second rotary (position t + 1) on the O^T accumulators, in-lane; float4 stores into the encoder input.
// The scalar kernel above spends its time in ~1 000 four-byte LDS reads per lane (87 us at config 2's V2 shape).
template <int E>
__global__ __launch_bounds__(256) void local_attention_mfma_kernel(const float* __restrict__ xseq,
                                                                   const float* __restrict__ cosT,
                                                                   const float* __restrict__ sinT, float* __restrict__ enc,
                                                                   half_t* __restrict__ enc16, int nwork, int T, int d,
                                                                   int heads, int window) {
    constexpr int HALF = E / 2, NKK = E / 16, NNB = E / 16, RS = E + 4;
    __shared__ __attribute__((aligned(16))) float sm_all[4 * 32 * RS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l15 = lane & 15, lq = lane >> 4;
    int work = blockIdx.x * 4 + wave;
    const bool active = work < nwork;
    work = active ? work : nwork - 1;                 // surplus waves redo the last window and skip the stores
    float* sm = sm_all + wave * 32 * RS;
    const int nwin = T / window;
    const int w = work % nwin, head = (work / nwin) % heads, b = work / (nwin * heads);
    const int k0 = w == 0 ? 0 : (w - 1) * window;
    const int q0 = w * window;
    const int nkeys = q0 + window - k0;               // window or 2*window (<= 32)
    const float* xb = xseq + ((long)b * T) * d + head * E;

    auto load_rot = [&](int pos, f32x4 (&f)[NKK]) {   // rows past the sequence read row T-1 (masked below)
        const int pc = pos < T ? pos : T - 1;
        const float* row = xb + (long)pc * d + 4 * lq;
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk) f[kk] = *reinterpret_cast<const f32x4*>(row + 16 * kk);
#pragma unroll
        for (int kk = 0; kk < NKK / 2; ++kk) {
            const f32x4 c = *reinterpret_cast<const f32x4*>(cosT + (long)pc * HALF + 16 * kk + 4 * lq);
            const f32x4 sn = *reinterpret_cast<const f32x4*>(sinT + (long)pc * HALF + 16 * kk + 4 * lq);
            const f32x4 lo = f[kk], hi = f[kk + NKK / 2];
            f[kk] = lo * c - hi * sn;
            f[kk + NKK / 2] = hi * c + lo * sn;
        }
    };
    f32x4 kf[2][NKK], qf[NKK];
    load_rot(k0 + l15, kf[0]);
    load_rot(k0 + 16 + l15, kf[1]);
    const int pos2 = q0 + (l15 < window ? l15 : window - 1) + 1;      // the second rotary's table rows, fetched up front
    f32x4 c2[NNB / 2], s2[NNB / 2];
#pragma unroll
    for (int nb = 0; nb < NNB / 2; ++nb) {
        c2[nb] = *reinterpret_cast<const f32x4*>(cosT + (long)pos2 * HALF + 16 * nb + 4 * lq);
        s2[nb] = *reinterpret_cast<const f32x4*>(sinT + (long)pos2 * HALF + 16 * nb + 4 * lq);
    }
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk)
            *reinterpret_cast<f32x4*>(sm + (kb * 16 + l15) * RS + 16 * kk + 4 * lq) = kf[kb][kk];
    __builtin_amdgcn_s_waitcnt(0xc07f);               // the wave's own LDS writes (no other wave touches its region)
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk) qf[kk] = *reinterpret_cast<const f32x4*>(sm + (q0 - k0 + l15) * RS + 16 * kk + 4 * lq);
    // S^T[key][query]: lane (query l15, quad lq), register r <-> key 16kb + 4lq + r
    f32x4 s[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk)
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) s[kb] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[kb][kk][e], qf[kk][e], s[kb], 0, 0, 0);
    const float scale = 1.0f / sqrtf((float)E);
    float v[8];
    float mx = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int kk = kb * 16 + 4 * lq + r;
            float x = s[kb][r] * scale;
            if (kk >= nkeys || k0 + kk > q0 + l15) x = -INFINITY;     // look-back padding / causal
            v[kb * 4 + r] = x;
            mx = fmaxf(mx, x);
        }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    float sum = 0.0f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        v[j] = expf(v[j] - mx);
        sum += v[j];
    }
    sum += __shfl_xor(sum, 16);
    sum += __shfl_xor(sum, 32);
    const float inv = 1.0f / sum;
    // O^T[hd][query] = V^T P^T: k-step (kb, r), slot lq <-> key 16kb + 4lq + r
    f32x4 o[NNB];
#pragma unroll
    for (int nb = 0; nb < NNB; ++nb) o[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float pr = v[kb * 4 + r] * inv;
            const float* vr = sm + (kb * 16 + 4 * lq + r) * RS + l15;
#pragma unroll
            for (int nb = 0; nb < NNB; ++nb) o[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(vr[16 * nb], pr, o[nb], 0, 0, 0);
        }
    // second rotary at position t+1 (lane: query l15, head-dim 16nb + 4lq + r; partner block nb +- NNB/2), store
    if (active && l15 < window) {
        const int pos = q0 + l15 + 1;
        const long orow = ((long)b * (T + 1) + pos) * d + head * E;
#pragma unroll
        for (int nb = 0; nb < NNB / 2; ++nb) {
            const f32x4 c = c2[nb], sn = s2[nb];
            const f32x4 lo = o[nb], hi = o[nb + NNB / 2];
            const f32x4 rl = lo * c - hi * sn, rh = hi * c + lo * sn;
            *reinterpret_cast<f32x4*>(enc + orow + 16 * nb + 4 * lq) = rl;
            *reinterpret_cast<f32x4*>(enc + orow + 16 * (nb + NNB / 2) + 4 * lq) = rh;
            if (enc16) {
                typedef half_t h4 __attribute__((ext_vector_type(4)));
                *reinterpret_cast<h4*>(enc16 + orow + 16 * nb + 4 * lq) = h4{(half_t)rl[0], (half_t)rl[1], (half_t)rl[2], (half_t)rl[3]};
                *reinterpret_cast<h4*>(enc16 + orow + 16 * (nb + NNB / 2) + 4 * lq) = h4{(half_t)rh[0], (half_t)rh[1], (half_t)rh[2], (half_t)rh[3]};
            }
        }
    }
}

hipError_t launch_local_attention(const float* xseq, const float* cosT, const float* sinT, float* enc,
                                  _Float16* enc16_, int B, int T, int d, int heads, int window, hipStream_t s) {
    half_t* enc16 = reinterpret_cast<half_t*>(enc16_);
    const int e = d / heads;
    if (local_attention_mfma_supported(d, heads, window)) {
        const int nwork = B * heads * (T / window);
        const dim3 grid((nwork + 3) / 4), block(256);
        if (e == 128)
            hipLaunchKernelGGL(local_attention_mfma_kernel<128>, grid, block, 0, s, xseq, cosT, sinT, enc, enc16, nwork, T, d, heads, window);
        else if (e == 64)
            hipLaunchKernelGGL(local_attention_mfma_kernel<64>, grid, block, 0, s, xseq, cosT, sinT, enc, enc16, nwork, T, d, heads, window);
        else
            hipLaunchKernelGGL(local_attention_mfma_kernel<32>, grid, block, 0, s, xseq, cosT, sinT, enc, enc16, nwork, T, d, heads, window);
        return hipGetLastError();
    }
    const size_t lds = (size_t)(2 * window * (e + 1) + window * 2 * window + window * (e + 1)) * sizeof(float);
    const dim3 grid(B * heads * (T / window)), block(64);
    hipLaunchKernelGGL(local_attention_kernel, grid, block, lds, s, xseq, cosT, sinT, enc, enc16, T, d, heads, window);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// V2 front end of the fp16 mode (same maths as local_attention_kernel above) on the fp16 MFMA: one wave per
// (sample, local head, window), four waves per block.  q = k = v = RoPE(x) for the <= 2*window rows involved:
//   * each lane loads 8-half pieces of "its" row (row = lane & 15 of a 16-row block) for all head-dim steps, so both
//     halves of every rotary pair sit in the same lane: RoPE is in-lane, and the rotated pieces are directly the
//     MFMA fragments of S^T = K Q^T (K block 0, K block 1 and the query block are three such row blocks);
//   * softmax on the accumulator layout (query on the lane axis, 8 keys per lane; cross-lane max / sum by two
//     shuffles), probabilities rounded to fp16 = B operand of O^T += V^T P^T;
//   * V^T fragments: the rotated key rows are parked in LDS (8 KiB per wave, chunk-swizzled like attentionh.hip)
//     and read back with ds_read_b64_tr_b16;
//   * second RoPE (position t+1) on the O^T accumulators, again in-lane; fp16 store into the encoder input.
typedef half_t la_f16x8 __attribute__((ext_vector_type(8)));
typedef __fp16 la_fp16x4_t __attribute__((__vector_size__(4 * sizeof(__fp16))));

template <int E>
__global__ __launch_bounds__(256) void local_attention_h_kernel(const half_t* __restrict__ xseq,
                                                                const float* __restrict__ cosT,
                                                                const float* __restrict__ sinT,
                                                                half_t* __restrict__ enc16, float* __restrict__ enc32,
                                                                int nwork, int T, int d, int heads, int window) {
    constexpr int HALF = E / 2, NKS = E / 32, NNB = E / 16, ROWB = E * 2;
    __shared__ __attribute__((aligned(16))) char sm_all[4 * 32 * ROWB];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l15 = lane & 15, lq = lane >> 4;
    int work = blockIdx.x * 4 + wave;
    const bool active = work < nwork;
    work = active ? work : nwork - 1;                 // surplus waves redo the last window (EXEC must stay full for the
    char* sm = sm_all + wave * 32 * ROWB;             // transposed reads); they skip the stores
    const int nwin = T / window;
    const int w = work % nwin, head = (work / nwin) % heads, b = work / (nwin * heads);
    const int k0 = w == 0 ? 0 : (w - 1) * window;
    const int q0 = w * window;
    const int nkeys = q0 + window - k0;               // window or 2*window (<= 32)
    const half_t* xb = xseq + ((long)b * T) * d + head * E;
    auto fswz = [](int row) { return E == 64 ? ((row >> 1) & 3) << 1 : (row & 7) << 1; };

    // rotated row -> NKS fragments (8 halves at head-dim 32*ks + 8*lq .. +7); rows past the sequence read row T-1
    auto load_rot = [&](int pos, la_f16x8 (&f)[NKS]) {
        const int pc = pos < T ? pos : T - 1;
        const half_t* row = xb + (long)pc * d + 8 * lq;
        float v[NKS][8];
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            const la_f16x8 h = *reinterpret_cast<const la_f16x8*>(row + 32 * ks);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[ks][j] = (float)h[j];
        }
#pragma unroll
        for (int ks = 0; ks < NKS / 2; ++ks) {
            const float* cp = cosT + (long)pc * HALF + 32 * ks + 8 * lq;
            const float* sp = sinT + (long)pc * HALF + 32 * ks + 8 * lq;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float c = cp[j], s = sp[j];
                const float lo = v[ks][j], hi = v[ks + NKS / 2][j];
                v[ks][j] = lo * c - hi * s;
                v[ks + NKS / 2][j] = hi * c + lo * s;
            }
        }
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks)
            f[ks] = la_f16x8{(half_t)v[ks][0], (half_t)v[ks][1], (half_t)v[ks][2], (half_t)v[ks][3],
                             (half_t)v[ks][4], (half_t)v[ks][5], (half_t)v[ks][6], (half_t)v[ks][7]};
    };
    la_f16x8 kf[2][NKS], qf[NKS];
    load_rot(k0 + l15, kf[0]);
    load_rot(k0 + 16 + l15, kf[1]);
    // the second rotary's table rows (position t + 1) are fetched now: their latency hides under everything below
    const int pos2 = q0 + (l15 < window ? l15 : window - 1) + 1;
    f32x4 c2[NNB / 2], s2[NNB / 2];
#pragma unroll
    for (int nb = 0; nb < NNB / 2; ++nb) {
        c2[nb] = *reinterpret_cast<const f32x4*>(cosT + (long)pos2 * HALF + 16 * nb + 4 * lq);
        s2[nb] = *reinterpret_cast<const f32x4*>(sinT + (long)pos2 * HALF + 16 * nb + 4 * lq);
    }
    // park the rotated key rows for the transposed V reads
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            const int row = kb * 16 + l15;
            *reinterpret_cast<la_f16x8*>(sm + row * ROWB + (((ks * 4 + lq) ^ fswz(row)) << 4)) = kf[kb][ks];
        }
    // the queries ARE key rows q0 - k0 .. (rotated at the same positions): read back from the parked rows instead of
    // loading and rotating them a second time (rows past the window belong to lanes whose output is not stored)
    __builtin_amdgcn_s_waitcnt(0xc07f);               // the wave's own LDS writes (no other wave touches its region)
    {
        const int row = q0 - k0 + l15;                // <= 25 < 32
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks)
            qf[ks] = *reinterpret_cast<const la_f16x8*>(sm + row * ROWB + (((ks * 4 + lq) ^ fswz(row)) << 4));
    }
    // S^T[key][query]
    f32x4 s[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) s[kb] = GDX_MFMA16(kf[kb][ks], qf[ks], s[kb], 0, 0, 0);
    const float c_log2 = 1.4426950408889634f / sqrtf((float)E);
    float v[8];
    float mx = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int kk = kb * 16 + 4 * lq + e;
            float x = s[kb][e] * c_log2;
            if (kk >= nkeys || k0 + kk > q0 + l15) x = -INFINITY;     // look-back padding / causal
            v[kb * 4 + e] = x;
            mx = fmaxf(mx, x);
        }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    float sum = 0.0f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        v[j] = __builtin_amdgcn_exp2f(v[j] - mx);
        sum += v[j];
    }
    sum += __shfl_xor(sum, 16);
    sum += __shfl_xor(sum, 32);
    const float inv = 1.0f / sum;
    const la_f16x8 pf = la_f16x8{(half_t)(v[0] * inv), (half_t)(v[1] * inv), (half_t)(v[2] * inv), (half_t)(v[3] * inv),
                                 (half_t)(v[4] * inv), (half_t)(v[5] * inv), (half_t)(v[6] * inv), (half_t)(v[7] * inv)};
    // O^T[hd][query] += V^T P^T
    const int vrow = 4 * lq + (l15 >> 2);
    const int vbase = vrow * ROWB + ((fswz(vrow) >> 1) << 5) + (l15 & 3) * 8;
    f32x4 o[NNB];
#pragma unroll
    for (int nb = 0; nb < NNB; ++nb) {
        const la_fp16x4_t t0 = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) la_fp16x4_t*)(sm + (vbase ^ (nb << 5))));
        const la_fp16x4_t t1 = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) la_fp16x4_t*)(sm + ((vbase + 16 * ROWB) ^ (nb << 5))));
        const f16x4 v0 = __builtin_bit_cast(f16x4, t0), v1 = __builtin_bit_cast(f16x4, t1);
        const la_f16x8 vf = la_f16x8{v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
        o[nb] = GDX_MFMA16(vf, pf, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
    }
    // second rotary at position t+1 (lane: query l15, head-dim 16nb + 4lq + e; partner block nb +- NNB/2), store
    if (active && l15 < window) {
        const int pos = q0 + l15 + 1;
        const long orow = ((long)b * (T + 1) + pos) * d + head * E;
#pragma unroll
        for (int nb = 0; nb < NNB / 2; ++nb) {
            const f32x4 c = c2[nb], sn = s2[nb];
            const f32x4 lo = o[nb], hi = o[nb + NNB / 2];
            const f32x4 rl = lo * c - hi * sn, rh = hi * c + lo * sn;
            *reinterpret_cast<f16x4*>(enc16 + orow + 16 * nb + 4 * lq) = f16x4{(half_t)rl[0], (half_t)rl[1], (half_t)rl[2], (half_t)rl[3]};
            *reinterpret_cast<f16x4*>(enc16 + orow + 16 * (nb + NNB / 2) + 4 * lq) =
                f16x4{(half_t)rh[0], (half_t)rh[1], (half_t)rh[2], (half_t)rh[3]};
            if (enc32) {
                *reinterpret_cast<f32x4*>(enc32 + orow + 16 * nb + 4 * lq) = rl;
                *reinterpret_cast<f32x4*>(enc32 + orow + 16 * (nb + NNB / 2) + 4 * lq) = rh;
            }
        }
    }
}

bool local_attention_f16_supported(int d, int heads, int window) {
    const int e = d / heads;
    return (e == 64 || e == 128) && window >= 1 && window <= 16 && d % 8 == 0;
}

hipError_t launch_local_attention_f16(const _Float16* xseq_, const float* cosT, const float* sinT, _Float16* enc16_,
                                      float* enc32, int B, int T, int d, int heads, int window, hipStream_t s) {
    const half_t* xseq = reinterpret_cast<const half_t*>(xseq_);
    half_t* enc16 = reinterpret_cast<half_t*>(enc16_);
    const int e = d / heads;
    const int nwork = B * heads * (T / window);
    const dim3 grid((nwork + 3) / 4), block(256);
    if (e == 128)
        hipLaunchKernelGGL(local_attention_h_kernel<128>, grid, block, 0, s, xseq, cosT, sinT, enc16, enc32, nwork, T, d, heads, window);
    else if (e == 64)
        hipLaunchKernelGGL(local_attention_h_kernel<64>, grid, block, 0, s, xseq, cosT, sinT, enc16, enc32, nwork, T, d, heads, window);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

GDX_HNS_END
}  // namespace gdx
