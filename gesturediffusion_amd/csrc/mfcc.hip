// MFCC front end of y['mfcc'] (reference data_loaders/gesture/data/dataset.py:81-95 -> python_speech_features.mfcc):
// pre-emphasis + framing, power spectrum (the DFT itself is a GEMM against a cos / -sin table, gdx_mfcc below), log mel
// energies (GEMM against the filterbank), DCT-II + lifter + log-energy + z-score.  fp32 only.
#include "gdx_host.h"

namespace gdx {

//   frames[f][i] = s[f*step + i] with s[0] = x[0], s[n] = x[n] - preemph * x[n-1], zero past the signal; row stride ldf
__global__ void mfcc_frames_kernel(const float* __restrict__ x, long n, float* __restrict__ frames, int numframes,
                                   int frame_len, int frame_step, int ldf, float preemph) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)numframes * ldf) return;
    const int f = i / ldf, c = i % ldf;
    float v = 0.0f;
    const long idx = (long)f * frame_step + c;
    if (c < frame_len && idx < n) v = idx == 0 ? x[0] : x[idx] - preemph * x[idx - 1];
    frames[i] = v;
}

// pw[f][k] = (re^2 + im^2) / nfft for k < nbins (zero in the padding columns); energy[f] = sum_k pw[f][k] (0 -> eps)
// spec rows: [re(0..nbins-1) | pad][im(0..nbins-1) | pad], im block at column im_off.  One block per frame.
__global__ __launch_bounds__(256) void mfcc_power_kernel(const float* __restrict__ spec, int lds, int im_off,
                                                         float* __restrict__ pw, int ldp, float* __restrict__ energy,
                                                         int nbins, float inv_nfft) {
    __shared__ float red[256];
    const int f = blockIdx.x, tid = threadIdx.x;
    const float* sp = spec + (long)f * lds;
    float e = 0.0f;
    for (int k = tid; k < ldp; k += 256) {
        float p = 0.0f;
        if (k < nbins) {
            const float re = sp[k], im = sp[im_off + k];
            p = (re * re + im * im) * inv_nfft;
        }
        pw[(long)f * ldp + k] = p;
        e += p;
    }
    red[tid] = e;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) energy[f] = red[0] == 0.0f ? 2.220446049250313e-16f : red[0];
}

// out[f][c] = ((lift[c] * sum_j dct[c][j] * log(mel[f][j])) [c == 0: log(energy[f])] - mean[c]) / std[c]
__global__ void mfcc_cepstrum_kernel(const float* __restrict__ mel, int ldm, const float* __restrict__ energy,
                                     const float* __restrict__ dct, const float* __restrict__ lift,
                                     const float* __restrict__ mean, const float* __restrict__ stdv,
                                     float* __restrict__ out, int numframes, int nfilt, int numcep) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= numframes * numcep) return;
    const int f = i / numcep, c = i % numcep;
    float v;
    if (c == 0) {
        v = logf(energy[f]);
    } else {
        float acc = 0.0f;
        for (int j = 0; j < nfilt; ++j) {
            float m = mel[(long)f * ldm + j];
            m = m == 0.0f ? 2.220446049250313e-16f : m;
            acc = fmaf(dct[c * nfilt + j], logf(m), acc);
        }
        v = lift[c] * acc;
    }
    if (mean) v = (v - mean[c]) / stdv[c];
    out[i] = v;
}

hipError_t launch_mfcc_frames(const float* x, long n, float* frames, int numframes, int frame_len, int frame_step, int ldf,
                              float preemph, hipStream_t s) {
    const long total = (long)numframes * ldf;
    hipLaunchKernelGGL(mfcc_frames_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, n, frames, numframes,
                       frame_len, frame_step, ldf, preemph);
    return hipGetLastError();
}
hipError_t launch_mfcc_power(const float* spec, int lds, int im_off, float* pw, int ldp, float* energy, int numframes,
                             int nbins, int nfft, hipStream_t s) {
    hipLaunchKernelGGL(mfcc_power_kernel, dim3(numframes), dim3(256), 0, s, spec, lds, im_off, pw, ldp, energy, nbins,
                       1.0f / (float)nfft);
    return hipGetLastError();
}
hipError_t launch_mfcc_cepstrum(const float* mel, int ldm, const float* energy, const float* dct, const float* lift,
                                const float* mean, const float* stdv, float* out, int numframes, int nfilt, int numcep,
                                hipStream_t s) {
    const int total = numframes * numcep;
    hipLaunchKernelGGL(mfcc_cepstrum_kernel, dim3((total + 255) / 256), dim3(256), 0, s, mel, ldm, energy, dct, lift, mean,
                       stdv, out, numframes, nfilt, numcep);
    return hipGetLastError();
}

}  // namespace gdx

using namespace gdx;

// MFCC front end (reference data_loaders/gesture/data/dataset.py:81-95).  The caller supplies the tables (built once on the
// host in fp64, stored fp32) and the workspace; layouts:
//   dft  [2*nbp][Lp]   rows k < nbins: cos(2 pi k i / nfft), rows nbp + k: -sin(...), zero elsewhere; Lp = frame_len up to 32,
//                      nbp = nbins up to 64
//   mel  [64][nbp]     rows j < nfilt: triangular filter j over the nbins power bins, zero elsewhere
//   work               (numframes + GDX_ROW_PAD) * (Lp + 2*nbp + nbp + 64) + numframes floats
extern "C" int gdx_mfcc(const float* signal, int64_t n, int32_t frame_len, int32_t frame_step, int32_t numframes,
                        int32_t nfft, int32_t nfilt, int32_t numcep, float preemph, const float* dft, const float* mel,
                        const float* dct, const float* lifter, const float* mean, const float* stdv, float* work,
                        float* out, void* stream) {
    if (!signal || !dft || !mel || !dct || !lifter || !work || !out) return fail("gdx_mfcc: null argument");
    if (n <= 0 || frame_len <= 0 || frame_step <= 0 || numframes <= 0 || nfft < frame_len || nfilt <= 0 || nfilt > 64 ||
        numcep <= 0 || numcep > nfilt)
        return fail("gdx_mfcc: bad geometry");
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = gemm_init();
    if (e != hipSuccess) return fail(std::string("gemm_init: ") + hipGetErrorString(e));
    const int nbins = nfft / 2 + 1, Lp = round_up(frame_len, 32), nbp = round_up(nbins, 64), rows = numframes + GDX_ROW_PAD;
    float* frames = work;
    float* spec = frames + (size_t)rows * Lp;
    float* pw = spec + (size_t)rows * 2 * nbp;
    float* melv = pw + (size_t)rows * nbp;
    float* energy = melv + (size_t)rows * 64;
    HIPCHK(launch_mfcc_frames(signal, (long)n, frames, numframes, frame_len, frame_step, Lp, preemph, s));
    GemmParams p{frames, Lp, dft, Lp, nullptr, nullptr, 0, nullptr, 0, spec, 2 * nbp, numframes, 2 * nbp, Lp, 1};
    if (gemm(OUT_ROWS, EPI_BIAS, p, s)) return -1;                       // DFT: [F, L] x [2*nbins, L]^T
    HIPCHK(launch_mfcc_power(spec, 2 * nbp, nbp, pw, nbp, energy, numframes, nbins, nfft, s));
    GemmParams q{pw, nbp, mel, nbp, nullptr, nullptr, 0, nullptr, 0, melv, 64, numframes, 64, nbp, 1};
    if (gemm(OUT_ROWS, EPI_BIAS, q, s)) return -1;                       // mel energies
    HIPCHK(launch_mfcc_cepstrum(melv, 64, energy, dct, lifter, mean, stdv, out, numframes, nfilt, numcep, s));
    return 0;
}
