// Host-side helpers shared by api.hip (the model handle; defines the functions declared here) and testapi.hip (the handle-free
// test / bench entry points).
#pragma once
#include "gdx_internal.h"

#include <string>
#include <vector>

namespace gdx {

int fail(const std::string& m);   // records the text of gdx_last_error (thread-local); returns -1
#define HIPCHK(expr)                                                                       \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) return fail(std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

static inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// half-type dispatch: the reduced-precision kernels exist as gdx:: (fp16) and gdx::b16:: (bf16) builds of one source
#define HFN(bf, fn, ...) ((bf) ? gdx::b16::fn(__VA_ARGS__) : gdx::h16::fn(__VA_ARGS__))

int dev_alloc(std::vector<void*>& pool, void** p, size_t bytes);   // hipMalloc, recorded in pool
void free_pool(std::vector<void*>& pool);

// the fp32 GEMM dispatch every forward GEMM goes through: gemm2.hip where it takes the problem, else gemm.hip
int gemm(int om, int ep, const GemmParams& p, hipStream_t s, GemmCtl* ctl = nullptr);

// dst [npad][kpad] halves = src[r*src_ld + col0 + c] for r < n, c < k, zero elsewhere
int pack_f16_into(_Float16* dst, const float* src, int n, int src_ld, int col0, int k, int npad, int kpad, hipStream_t s,
                  bool bf = false);

// V2 front end (RoPE -> causal local attention -> RoPE at t+1) for compute dtype `dtype`: the one dispatch of the forwards and
// of the test entry point gdx_local_attention.  The 16-bit kernel (local_attention_half) reads xseq16 and writes enc16 plus the
// optional fp32 copy enc; otherwise the fp32 kernel (MFMA, or the scalar one for other head widths / windows) reads xseq and
// writes enc plus the optional 16-bit copy enc16.
bool local_attention_half(int dtype, int d, int heads, int window);
hipError_t launch_local_attention_any(int dtype, const float* xseq, const _Float16* xseq16, const float* cosT, const float* sinT,
                                      float* enc, _Float16* enc16, int B, int T, int d, int heads, int window, hipStream_t s);

// Average microseconds of `iters` calls of launch() after `warm` warm-up calls, between two events on s.  launch() returns 0,
// or -1 with the error recorded.  The events are destroyed on every path.
template <class F>
int time_launches(int warm, int iters, hipStream_t s, float* avg_us, F launch) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto timed = [&]() -> int {
        HIPCHK(hipEventCreate(&e0));
        HIPCHK(hipEventCreate(&e1));
        for (int i = 0; i < warm; ++i)
            if (launch()) return -1;
        HIPCHK(hipEventRecord(e0, s));
        for (int i = 0; i < iters; ++i)
            if (launch()) return -1;
        HIPCHK(hipEventRecord(e1, s));
        HIPCHK(hipEventSynchronize(e1));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, e0, e1));
        *avg_us = ms * 1000.0f / (float)iters;
        return 0;
    };
    const int rc = timed();
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    return rc;
}

}  // namespace gdx
