// libgdx.so: the handle-free test and bench entry points of the C ABI (include/gdx.h).  Each runs one kernel, through the
// dispatch the forwards use (gdx_host.h), on scratch copies of the caller's fp32 arrays laid out like the workspace.  What a call
// forces or wants reported travels in the launchers' control argument (GemmCtl / GemmHCtl), never in process-wide state.
#include "gdx_host.h"

#include <cstdio>
#include <cstdlib>

using namespace gdx;

// gdx_set_test_half_dtype / gdx_set_test_gemmh_tile: element type and forced tile (negative: none) of the entry points that take
// neither as an argument (gdx_linear_f16, gdx_attention_f16, gdx_bench_gemm_f16, gdx_bench_attention)
static bool t_bf16 = false;
static int t_gemmh_mb = -1, t_gemmh_nbw = -1;

namespace {

// Device scratch of one call.  Leaving the scope on any path waits for the stream and frees it.
struct Scratch {
    const std::string who;
    const hipStream_t s;
    const bool bf;                 // 16-bit element type of to_half / widen
    std::vector<void*> pool;
    Scratch(const char* who, hipStream_t s, bool bf = false) : who(who), s(s), bf(bf) {}
    ~Scratch() {
        (void)hipStreamSynchronize(s);
        free_pool(pool);
    }
    template <class T>
    int alloc(T** p, size_t bytes) { return dev_alloc(pool, (void**)p, bytes); }
    // *h = n 16-bit elements, filled with src rounded to the half type when src is given (an input, or an output staged from
    // the caller's own values so that elements the kernel does not store come back unchanged: NaN stays NaN)
    int to_half(_Float16** h, const float* src, int64_t n) {
        if (alloc(h, 2 * (size_t)n)) return -1;
        if (src && HFN(bf, launch_convert_f16, src, *h, n, s) != hipSuccess) return fail(who + ": convert failed");
        return 0;
    }
    int widen(const _Float16* h, float* dst, int64_t n) {
        if (HFN(bf, launch_convert_f32, h, dst, n, s) != hipSuccess) return fail(who + ": convert failed");
        return 0;
    }
    // the same for an fp32 output: *d = n floats staged from the caller's own values; unstage copies all of them back
    int stage(float** d, const float* src, int64_t n) {
        if (alloc(d, sizeof(float) * (size_t)n)) return -1;
        if (hipMemcpyAsync(*d, src, sizeof(float) * (size_t)n, hipMemcpyDeviceToDevice, s) != hipSuccess)
            return fail(who + ": staging failed");
        return 0;
    }
    int unstage(const float* d, float* dst, int64_t n) {
        if (hipMemcpyAsync(dst, d, sizeof(float) * (size_t)n, hipMemcpyDeviceToDevice, s) != hipSuccess)
            return fail(who + ": copy-out failed");
        return 0;
    }
};

// One extra launch with in-kernel stamps when GDX_GEMM_DEBUG is set (diagnostic path only): launch(stamps) gets a zeroed
// 512-byte device buffer, whose first n words come back in host[].  False: nothing to decode.
template <class F>
bool stamped_launch(Scratch& sc, unsigned long long* host, int n, F launch) {
    unsigned long long* d = nullptr;
    if (!getenv("GDX_GEMM_DEBUG") || sc.alloc(&d, 512)) return false;
    (void)hipMemsetAsync(d, 0, 512, sc.s);
    launch(d);
    (void)hipMemcpyAsync(host, d, 8 * n, hipMemcpyDeviceToHost, sc.s);
    (void)hipStreamSynchronize(sc.s);
    return true;
}

}  // namespace

// Stand-alone GEMM timing on scratch buffers (measurement helper for tools/gemm_sweep.py and bench.py).
extern "C" int gdx_bench_gemm(int32_t M, int32_t N, int32_t K, int32_t epi, int32_t iters, float* avg_us, void* stream) {
    if (!avg_us || M <= 0 || N <= 0 || K <= 0 || K % 32 || iters <= 0) return fail("gdx_bench_gemm: bad argument");
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = gemm_init();
    if (e != hipSuccess) return fail(std::string("gemm_init: ") + hipGetErrorString(e));
    const int npad = round_up(N, 128);
    float *A = nullptr, *W = nullptr, *bias = nullptr, *R = nullptr, *C = nullptr;
    Scratch sc("gdx_bench_gemm", s);
    if (sc.alloc(&A, sizeof(float) * (size_t)(M + GDX_ROW_PAD) * K) || sc.alloc(&W, sizeof(float) * (size_t)npad * K) ||
        sc.alloc(&bias, sizeof(float) * npad) || sc.alloc(&R, sizeof(float) * (size_t)M * N) ||
        sc.alloc(&C, sizeof(float) * (size_t)(M + GDX_ROW_PAD) * N))
        return -1;
    // non-trivial operand values (zero operands raise the clock: cdna_hip_programming.md rule 25)
    HIPCHK(gdx_randn(A, 1, (int64_t)M * K, 1, 0, 0, stream) ? hipErrorUnknown : hipSuccess);
    HIPCHK(gdx_randn(W, 1, (int64_t)npad * K, 2, 0, 0, stream) ? hipErrorUnknown : hipSuccess);
    HIPCHK(gdx_randn(R, 1, (int64_t)M * N, 3, 0, 0, stream) ? hipErrorUnknown : hipSuccess);
    HIPCHK(gdx_randn(bias, 1, npad, 4, 0, 0, stream) ? hipErrorUnknown : hipSuccess);
    GemmParams p{A, K, W, K, bias, R, N, nullptr, 0, C, N, M, N, K, 1};
    if (time_launches(3, iters, s, avg_us, [&] { return gemm(OUT_ROWS, epi, p, s); })) return -1;
    unsigned long long h[40] = {0};
    GemmCtl ctl;
    if (stamped_launch(sc, h, 40, [&](unsigned long long* st) { ctl.stamps = st; (void)gemm(OUT_ROWS, epi, p, s, &ctl); })) {
        if (h[9]) {
            fprintf(stderr, "[gemm2 stamps] barrier B of step 40, cycles relative to wave0 release (arrive/release):");
            for (int w = 0; w < 12; ++w)
                fprintf(stderr, " w%d:%lld/%lld", w, (long long)(h[8 + 2 * w] - h[9]), (long long)(h[9 + 2 * w] - h[9]));
            fprintf(stderr, "\n");
        }
        if (h[2])
            fprintf(stderr, "[gemm2 stamps] block0 consumer: %llu cycles, %.2f us, %llu K-steps -> %.0f cycles/step, clock %.2f GHz\n",
                    h[0], h[1] / 100.0, h[2], (double)h[0] / h[2], h[1] ? (double)h[0] / (h[1] * 10.0) : 0.0);
    }
    return 0;
}

// gdx_linear_full / gdx_linear_f32: one launch through gemm() on scratch copies laid out like the workspace.  A and R carry
// GDX_ROW_PAD rows of NaN bit patterns behind the caller's rows (in the forwards those rows hold whatever the last whole-tile
// store left there; the kernels read whole tiles of A); C is staged from the caller's own values and copied back whole.
static int linear_full(const char* who, const float* A, const float* W, const float* bias, const float* R, int32_t ldr,
                       const float* V, int32_t ldv, float* C, int32_t c_rows, int32_t M, int32_t N, int32_t K, int32_t T,
                       int32_t rowmap, int32_t gelu, int32_t kernel, int32_t tile_mb, int32_t tile_nbw, int32_t tile_bk,
                       int32_t* launched, hipStream_t s) {
    // every refusal comes before the first HIP call (tests/test_host_logic.py checks them without a GPU)
    const std::string w(who);
    if (!A || !W || !C || M <= 0 || N <= 0 || K <= 0 || K % 32 || T <= 0) return fail(w + ": bad argument");
    const long out_rows = rowmap ? (long)M + (M - 1) / T + 1 : M;    // rows the epilogue stores (rowmap: m + m/T + 1)
    if (c_rows < out_rows) return fail(w + ": c_rows below the stored rows");
    if ((R && ldr < N) || (V && ldv < N)) return fail(w + ": ldr / ldv below N");
    if (kernel < 0 || kernel > 2) return fail(w + ": unknown kernel (0 = dispatch, 1 = gemm2.hip, 2 = gemm.hip)");
    if (tile_mb < 0 || tile_nbw < 0 || tile_bk < 0 || ((tile_mb == 0) != (tile_nbw == 0)) || ((tile_mb == 0) != (tile_bk == 0)))
        return fail(w + ": (tile_mb, tile_nbw, tile_bk) all positive, or (0, 0, 0)");
    if (tile_mb && kernel == 2) return fail(w + ": a forced tile is for the persistent kernel (kernel 0 or 1) only");
    // the mode / epilogue pair of the forward that has this operand set (forward_core); anything else has no launch
    int om = OUT_ROWS, ep = EPI_BIAS;
    if (gelu) {
        if (R || V || rowmap) return fail(w + ": no launch in the forwards: GELU goes with the bias epilogue only (FFN-1)");
        ep = EPI_GELU;
    } else if (V) {
        if (!R || bias || rowmap)
            return fail(w + ": no launch in the forwards: V goes with R, without bias and without a row map (V2 proj_pose)");
        ep = EPI_RES_VEC;
    } else if (R) {
        ep = EPI_RES;
        if (rowmap) om = OUT_TOKROWS;
    } else if (rowmap) {
        return fail(w + ": no launch in the forwards: the row map goes with R (V1 input linear)");
    }
    const size_t arow = (size_t)M + GDX_ROW_PAD, crow = (size_t)c_rows + GDX_ROW_PAD;
    const size_t r_rows = R ? (size_t)out_rows : 0, rrow = r_rows + GDX_ROW_PAD;
    if (4 * arow * K >= (1ull << 31) || 4 * crow * N >= (1ull << 31) || (R && 4 * rrow * ldr >= (1ull << 31)))
        return fail(w + ": an operand exceeds the 2 GiB buffer-descriptor range; run the batch in smaller pieces");
    hipError_t e = gemm_init();
    if (e != hipSuccess) return fail(std::string("gemm_init: ") + hipGetErrorString(e));
    const int npad = round_up(N, 128);
    float *a = nullptr, *wp = nullptr, *r = nullptr, *c = nullptr;
    Scratch sc(who, s);
    if (sc.alloc(&a, sizeof(float) * arow * K) || sc.alloc(&wp, sizeof(float) * (size_t)npad * K) ||
        (R && sc.alloc(&r, sizeof(float) * rrow * ldr)) || sc.alloc(&c, sizeof(float) * crow * N))
        return -1;
    // 0xff bytes: every padding float is a NaN; the packed weight's padding rows are zero, as gdx_set_weight leaves them
    if (hipMemsetAsync(a + (size_t)M * K, 0xff, sizeof(float) * GDX_ROW_PAD * K, s) != hipSuccess ||
        hipMemsetAsync(wp, 0, sizeof(float) * (size_t)npad * K, s) != hipSuccess ||
        (R && hipMemsetAsync(r + r_rows * ldr, 0xff, sizeof(float) * GDX_ROW_PAD * ldr, s) != hipSuccess) ||
        hipMemsetAsync(c + (size_t)c_rows * N, 0xff, sizeof(float) * GDX_ROW_PAD * N, s) != hipSuccess ||
        hipMemcpyAsync(a, A, sizeof(float) * (size_t)M * K, hipMemcpyDeviceToDevice, s) != hipSuccess ||
        hipMemcpyAsync(wp, W, sizeof(float) * (size_t)N * K, hipMemcpyDeviceToDevice, s) != hipSuccess ||
        (R && hipMemcpyAsync(r, R, sizeof(float) * r_rows * ldr, hipMemcpyDeviceToDevice, s) != hipSuccess) ||
        hipMemcpyAsync(c, C, sizeof(float) * (size_t)c_rows * N, hipMemcpyDeviceToDevice, s) != hipSuccess)
        return fail(w + ": staging failed");
    GemmParams p{a, K, wp, K, bias, r, ldr, V, ldv, c, N, M, N, K, T};
    GemmCtl ctl;
    ctl.file = kernel;
    ctl.mb = tile_mb; ctl.nbw = tile_nbw; ctl.bk = tile_bk;
    const int rc = gemm(om, ep, p, s, &ctl);
    if (launched) {
        const GemmLaunched& l = ctl.ran;
        launched[0] = l.file; launched[1] = l.mb; launched[2] = l.nbw; launched[3] = l.bk; launched[4] = l.nst; launched[5] = l.resp;
    }
    if (!rc && hipMemcpyAsync(C, c, sizeof(float) * (size_t)c_rows * N, hipMemcpyDeviceToDevice, s) != hipSuccess)
        return fail(w + ": copy-out failed");
    return rc;
}

extern "C" int gdx_linear_full(const float* A, const float* W, const float* bias, const float* R, int32_t ldr, const float* V,
                               int32_t ldv, float* C, int32_t c_rows, int32_t M, int32_t N, int32_t K, int32_t T, int32_t rowmap,
                               int32_t gelu, int32_t kernel, int32_t tile_mb, int32_t tile_nbw, int32_t tile_bk,
                               int32_t* launched, void* stream) {
    return linear_full("gdx_linear_full", A, W, bias, R, ldr, V, ldv, C, c_rows, M, N, K, T, rowmap, gelu, kernel, tile_mb,
                       tile_nbw, tile_bk, launched, (hipStream_t)stream);
}

// the plain / GELU / residual epilogues of the same call, R and C [M][N], through the dispatcher
extern "C" int gdx_linear_f32(const float* A, const float* W, const float* bias, const float* R, float* C, int32_t M,
                              int32_t N, int32_t K, int32_t epi, int32_t tile_mb, int32_t tile_nbw, int32_t tile_bk,
                              void* stream) {
    if (epi < EPI_BIAS || epi > EPI_RES || (epi == EPI_RES && !R)) return fail("gdx_linear_f32: bad argument");
    return linear_full("gdx_linear_f32", A, W, bias, epi == EPI_RES ? R : nullptr, N, nullptr, 0, C, M, M, N, K, 1, 0,
                       epi == EPI_GELU, 0, tile_mb, tile_nbw, tile_bk, nullptr, (hipStream_t)stream);
}

extern "C" int gdx_set_test_half_dtype(int32_t dtype) {
    if (dtype != GDX_DTYPE_F16 && dtype != GDX_DTYPE_BF16) return fail("gdx_set_test_half_dtype: GDX_DTYPE_F16 or GDX_DTYPE_BF16");
    t_bf16 = dtype == GDX_DTYPE_BF16;
    return 0;
}

extern "C" int gdx_set_test_gemmh_tile(int32_t mb, int32_t nbw) {
    if (mb < 0 || nbw < 0 || (mb == 0) != (nbw == 0)) return fail("gdx_set_test_gemmh_tile: (mb, nbw) both positive, or (0, 0)");
    t_gemmh_mb = mb;
    t_gemmh_nbw = nbw;
    return 0;
}

// gdx_linear_half / gdx_linear_f16.  (force_mb, force_nbw) as GemmHCtl takes them: negative = no say.
static int linear_half(const char* who, const float* A, const float* W, const float* bias, const float* R, int32_t ldr,
                       const float* V, int32_t ldv, float* C32, float* C16, int32_t c_rows, int32_t M, int32_t N, int32_t K,
                       int32_t T, int32_t rowmap, int32_t gelu, bool bf, int32_t force_mb, int32_t force_nbw,
                       int32_t* launched, hipStream_t s) {
    const std::string w(who);
    const long out_rows = rowmap ? (long)M + (M - 1) / T + 1 : M;    // rows the epilogue stores (rowmap: m + m/T + 1)
    if (!A || !W || (!C32 && !C16) || M <= 0 || N <= 0 || K <= 0 || K % 64 || N % 64 || T <= 0 || c_rows < out_rows ||
        (R && (ldr < N || ldr % 4)) || (V && (ldv < N || ldv % 4)))
        return fail(w + ": bad argument");
    const int npad = round_up(N, 256);
    if (2 * (size_t)M * K >= (1ull << 31) || 2 * (size_t)npad * K >= (1ull << 31) || 2 * (size_t)c_rows * N >= (1ull << 31))
        return fail(w + ": an operand exceeds the 2 GiB buffer-descriptor range; run the batch in smaller pieces");
    _Float16 *a16 = nullptr, *w16 = nullptr, *c16 = nullptr;
    Scratch sc(who, s, bf);
    if (sc.to_half(&a16, A, (int64_t)M * K) || sc.alloc(&w16, 2 * (size_t)npad * K) ||
        (C16 && sc.to_half(&c16, C16, (int64_t)c_rows * N)) || pack_f16_into(w16, W, N, K, 0, K, npad, K, s, bf))
        return -1;
    GemmHParams p{a16, K, w16, K, (int)((size_t)M * K * 2), (int)((size_t)npad * K * 2), bias, R, ldr, V, ldv,
                  C32, N, c16, N, M, N, K, T, rowmap, gelu};
    GemmHCtl ctl;
    ctl.mb = force_mb; ctl.nbw = force_nbw;
    const hipError_t e = HFN(bf, launch_gemmh, p, s, &ctl);
    if (launched) {
        const GemmHLaunched& l = ctl.ran;
        launched[0] = l.mb; launched[1] = l.nbw; launched[2] = l.main_rows; launched[3] = l.tail_mb; launched[4] = l.tail_nbw;
    }
    if (e != hipSuccess) return fail(std::string("launch_gemmh: ") + hipGetErrorString(e));
    return C16 ? sc.widen(c16, C16, (int64_t)c_rows * N) : 0;
}

extern "C" int gdx_linear_half(const float* A, const float* W, const float* bias, const float* R, int32_t ldr, const float* V,
                               int32_t ldv, float* C32, float* C16, int32_t c_rows, int32_t M, int32_t N, int32_t K, int32_t T,
                               int32_t rowmap, int32_t gelu, int32_t dtype, int32_t tile_mb, int32_t tile_nbw,
                               int32_t* launched, void* stream) {
    if ((dtype != GDX_DTYPE_F16 && dtype != GDX_DTYPE_BF16) || tile_mb < 0 || tile_nbw < 0 || (tile_mb == 0) != (tile_nbw == 0))
        return fail("gdx_linear_half: bad argument");
    return linear_half("gdx_linear_half", A, W, bias, R, ldr, V, ldv, C32, C16, c_rows, M, N, K, T, rowmap, gelu,
                       dtype == GDX_DTYPE_BF16, tile_mb, tile_nbw, launched, (hipStream_t)stream);
}

extern "C" int gdx_linear_f16(const float* A, const float* W, const float* bias, float* C32, float* C16, int32_t M,
                              int32_t N, int32_t K, int32_t gelu, void* stream) {
    return linear_half("gdx_linear_f16", A, W, bias, nullptr, 0, nullptr, 0, C32, C16, M, M, N, K, 1, 0, gelu, t_bf16,
                       t_gemmh_mb, t_gemmh_nbw, nullptr, (hipStream_t)stream);
}

extern "C" int gdx_layernorm(const float* x, const float* res, const float* gamma, const float* beta, float* out32,
                             float* out16, int32_t out_rows, int32_t rows, int32_t d, int32_t compact_S, int32_t half_input,
                             int32_t dtype, void* stream) {
    const long need = compact_S > 0 ? (long)rows - (rows + compact_S - 1) / compact_S : rows;
    if (!x || !gamma || !beta || (!out32 && !out16) || rows <= 0 || d <= 0 || d % 32 || d > 2048 || compact_S < 0 ||
        out_rows < need || (dtype != GDX_DTYPE_F32 && dtype != GDX_DTYPE_F16 && dtype != GDX_DTYPE_BF16) ||
        (dtype == GDX_DTYPE_F32 && (half_input || out16)) || (half_input && !out16))
        return fail("gdx_layernorm: bad argument");
    hipStream_t s = (hipStream_t)stream;
    const bool bf = dtype == GDX_DTYPE_BF16;
    const int64_t n_in = (int64_t)rows * d, n_out = (int64_t)out_rows * d;
    _Float16 *x16 = nullptr, *r16 = nullptr, *o16 = nullptr;
    Scratch sc("gdx_layernorm", s, bf);
    if ((half_input && (sc.to_half(&x16, x, n_in) || (res && sc.to_half(&r16, res, n_in)))) ||
        (out16 && sc.to_half(&o16, out16, n_out)))
        return -1;
    const hipError_t e = half_input ? HFN(bf, launch_layernorm_f16, x16, r16, gamma, beta, o16, out32, rows, d, compact_S, s)
                                    : HFN(bf, launch_layernorm, x, res, gamma, beta, out32, o16, rows, d, compact_S, s);
    if (e != hipSuccess) return fail(std::string("launch_layernorm: ") + hipGetErrorString(e));
    return out16 ? sc.widen(o16, out16, n_out) : 0;
}

extern "C" int gdx_local_attention(const float* xseq, const float* cosT, const float* sinT, float* enc, float* enc16,
                                   int32_t enc_rows, int32_t B, int32_t T, int32_t d, int32_t heads, int32_t window,
                                   int32_t dtype, int32_t* kernel, void* stream) {
    const bool dt_ok = dtype == GDX_DTYPE_F32 || dtype == GDX_DTYPE_F16 || dtype == GDX_DTYPE_BF16;
    if (!xseq || !cosT || !sinT || !dt_ok || B <= 0 || T <= 0 || heads <= 0 || d <= 0 || d % heads || (d / heads) % 2 ||
        window <= 0 || T % window || enc_rows < (long)B * (T + 1) || (dtype == GDX_DTYPE_F32 && enc16))
        return fail("gdx_local_attention: bad argument");
    const bool half = local_attention_half(dtype, d, heads, window);
    if (!half && !enc) return fail("gdx_local_attention: the fp32 kernel needs enc");
    if (half && !enc16) return fail("gdx_local_attention: the 16-bit kernel needs enc16");
    hipStream_t s = (hipStream_t)stream;
    const int64_t n_in = (int64_t)B * T * d, n_out = (int64_t)enc_rows * d;
    _Float16 *x16 = nullptr, *e16 = nullptr;
    Scratch sc("gdx_local_attention", s, dtype == GDX_DTYPE_BF16);
    if (kernel) *kernel = half ? 2 : local_attention_mfma_supported(d, heads, window) ? 1 : 0;
    if ((half && sc.to_half(&x16, xseq, n_in)) || (enc16 && sc.to_half(&e16, enc16, n_out))) return -1;
    const hipError_t e = launch_local_attention_any(dtype, xseq, x16, cosT, sinT, enc, e16, B, T, d, heads, window, s);
    if (e != hipSuccess) return fail(std::string("launch_local_attention: ") + hipGetErrorString(e));
    return enc16 ? sc.widen(e16, enc16, n_out) : 0;
}

// ---- the boundary kernels of the denoiser step (boundary.hip, boundaryh.hip), each through the launcher the forwards call.  Inputs are read where
// the caller put them (strides and the rows behind them included); every output is staged from the caller's own values and
// copied back whole, so elements the kernel does not store come back unchanged.  Every refusal comes before the first HIP call
// (tests/test_host_logic.py checks them without a GPU).
static bool dtype_known(int dtype) { return dtype == GDX_DTYPE_F32 || dtype == GDX_DTYPE_F16 || dtype == GDX_DTYPE_BF16; }

extern "C" int gdx_transpose_in(const float* x, float* xt, int32_t xt_rows, int32_t B, int32_t Bsrc, int32_t J, int32_t T,
                                int32_t ldx, int32_t dtype, void* stream) {
    if (!x || !xt || B <= 0 || B > 65535 || Bsrc <= 0 || Bsrc > B || J <= 0 || T <= 0) return fail("gdx_transpose_in: bad argument");
    if (!dtype_known(dtype)) return fail("gdx_transpose_in: unknown dtype");
    if (ldx < J) return fail("gdx_transpose_in: ldx below J");
    if (xt_rows < (long)B * T) return fail("gdx_transpose_in: xt_rows below B*T");
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = (int64_t)xt_rows * ldx;
    Scratch sc("gdx_transpose_in", s, dtype == GDX_DTYPE_BF16);
    if (dtype == GDX_DTYPE_F32) {
        float* o = nullptr;
        if (sc.stage(&o, xt, n)) return -1;
        const hipError_t e = launch_transpose_in(x, o, B, Bsrc, J, T, ldx, s);
        if (e != hipSuccess) return fail(std::string("launch_transpose_in: ") + hipGetErrorString(e));
        return sc.unstage(o, xt, n);
    }
    _Float16* o16 = nullptr;
    if (sc.to_half(&o16, xt, n)) return -1;
    const hipError_t e = HFN(sc.bf, launch_transpose_in_f16, x, o16, B, Bsrc, J, T, ldx, s);
    if (e != hipSuccess) return fail(std::string("launch_transpose_in_f16: ") + hipGetErrorString(e));
    return sc.widen(o16, xt, n);
}

extern "C" int gdx_transpose_out(const float* yt, float* y, int32_t y_rows, int32_t B, int32_t J, int32_t T, int32_t ldy,
                                 void* stream) {
    if (!yt || !y || B <= 0 || B > 65535 || J <= 0 || T <= 0) return fail("gdx_transpose_out: bad argument");
    if (ldy < J) return fail("gdx_transpose_out: ldy below J");
    if (y_rows < (long)B * J) return fail("gdx_transpose_out: y_rows below B*J");
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = (int64_t)y_rows * T;
    float* o = nullptr;
    Scratch sc("gdx_transpose_out", s);
    if (sc.stage(&o, y, n)) return -1;
    const hipError_t e = launch_transpose_out(yt, o, B, J, T, ldy, s);
    if (e != hipSuccess) return fail(std::string("launch_transpose_out: ") + hipGetErrorString(e));
    return sc.unstage(o, y, n);
}

extern "C" int gdx_small_linear(const float* A, int32_t lda, const float* W, int32_t ldw, const float* bias, float* out,
                                int32_t out_rows, int32_t ldo, int32_t M, int32_t N, int32_t K, int32_t act, void* stream) {
    if (!A || !W || !out || M <= 0 || M > 4 * 65535 || N <= 0 || K <= 0) return fail("gdx_small_linear: bad argument");
    if (act != 0 && act != 1) return fail("gdx_small_linear: unknown act (0 = none, 1 = SiLU)");
    if (lda < K || ldw < K) return fail("gdx_small_linear: lda / ldw below K");
    if (ldo < N) return fail("gdx_small_linear: ldo below N");
    if (out_rows < M) return fail("gdx_small_linear: out_rows below M");
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = (int64_t)out_rows * ldo;
    float* o = nullptr;
    Scratch sc("gdx_small_linear", s);
    if (sc.stage(&o, out, n)) return -1;
    const hipError_t e = launch_small_linear(A, lda, W, ldw, bias, o, ldo, M, N, K, act, s);
    if (e != hipSuccess) return fail(std::string("launch_small_linear: ") + hipGetErrorString(e));
    return sc.unstage(o, out, n);
}

extern "C" int gdx_gather_rows(const float* table, const int64_t* idx, float* out, int32_t out_rows, int32_t M, int32_t d,
                               int32_t max_rows, void* stream) {
    if (!table || !idx || !out || M <= 0 || d <= 0 || max_rows <= 0) return fail("gdx_gather_rows: bad argument");
    if (out_rows < M) return fail("gdx_gather_rows: out_rows below M");
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = (int64_t)out_rows * d;
    float* o = nullptr;
    Scratch sc("gdx_gather_rows", s);
    if (sc.stage(&o, out, n)) return -1;
    const hipError_t e = launch_gather_rows(table, idx, o, M, d, max_rows, s);
    if (e != hipSuccess) return fail(std::string("launch_gather_rows: ") + hipGetErrorString(e));
    return sc.unstage(o, out, n);
}

extern "C" int gdx_mfcc_project(const float* mfcc, const float* W, int32_t ldw, const float* bias, const float* pe, float* out,
                                int32_t out_rows, int32_t B, int32_t Bsrc, int32_t C, int32_t T, int32_t d, int32_t rps,
                                int32_t off, void* stream) {
    if (!mfcc || !W || !bias || !out || B <= 0 || Bsrc <= 0 || Bsrc > B || C <= 0 || T <= 0 || d <= 0 || off < 0 ||
        (long)B * T > 64l * 65535)
        return fail("gdx_mfcc_project: bad argument");
    if (C > 32) return fail("gdx_mfcc_project: C above 32 (the kernel holds a weight row in 32 registers)");
    if (ldw < C) return fail("gdx_mfcc_project: ldw below C");
    if (rps < (long)T + off) return fail("gdx_mfcc_project: rps below T + off");
    if (out_rows < (long)(B - 1) * rps + off + T) return fail("gdx_mfcc_project: out_rows below the stored rows");
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = (int64_t)out_rows * d;
    float* o = nullptr;
    Scratch sc("gdx_mfcc_project", s);
    if (sc.stage(&o, out, n)) return -1;
    const hipError_t e = launch_mfcc_project(mfcc, W, ldw, bias, pe, o, B, Bsrc, C, T, d, rps, off, s);
    if (e != hipSuccess) return fail(std::string("launch_mfcc_project: ") + hipGetErrorString(e));
    return sc.unstage(o, out, n);
}

extern "C" int gdx_token0(const float* temb, int32_t tstride, const float* seed_emb, const float* pe0, float* enc, float* enc16,
                          int32_t enc_rows, const float* c2t, const float* c2_seed, float* c2, int32_t c2_rows,
                          const int32_t* state, int32_t B, int32_t Bsrc, int32_t S, int32_t d, int32_t dtype, void* stream) {
    if (!temb || !seed_emb || !enc || B <= 0 || Bsrc <= 0 || Bsrc > B || S <= 0 || d <= 0 || (long)B * d >= (1l << 31))
        return fail("gdx_token0: bad argument");
    if (!dtype_known(dtype)) return fail("gdx_token0: unknown dtype");
    if (enc16 && dtype == GDX_DTYPE_F32) return fail("gdx_token0: GDX_DTYPE_F32 takes no enc16");
    if (tstride != 0 && tstride < d) return fail("gdx_token0: tstride must be 0 (one row for the batch) or at least d");
    if ((c2 != nullptr) != (c2t != nullptr) || (c2 != nullptr) != (c2_seed != nullptr))
        return fail("gdx_token0: c2t, c2_seed and c2 go together");
    if (enc_rows < (long)(B - 1) * S + 1) return fail("gdx_token0: enc_rows below the stored rows");
    if (c2 && c2_rows < B) return fail("gdx_token0: c2_rows below B");
    hipStream_t s = (hipStream_t)stream;
    const int64_t n_enc = (int64_t)enc_rows * d, n_c2 = (int64_t)c2_rows * d;
    float *e32 = nullptr, *o2 = nullptr;
    _Float16* e16 = nullptr;
    Scratch sc("gdx_token0", s, dtype == GDX_DTYPE_BF16);
    if (sc.stage(&e32, enc, n_enc) || (enc16 && sc.to_half(&e16, enc16, n_enc)) || (c2 && sc.stage(&o2, c2, n_c2))) return -1;
    const hipError_t e = HFN(sc.bf, launch_token0, temb, tstride, seed_emb, pe0, e32, e16, c2t, c2_seed, o2, state, B, Bsrc, S, d, s);
    if (e != hipSuccess) return fail(std::string("launch_token0: ") + hipGetErrorString(e));
    if (sc.unstage(e32, enc, n_enc) || (c2 && sc.unstage(o2, c2, n_c2))) return -1;
    return enc16 ? sc.widen(e16, enc16, n_enc) : 0;
}

extern "C" int gdx_attention_f16(const float* qkv, float* ctx, int32_t B, int32_t S, int32_t H, int32_t d, void* stream) {
    if (!qkv || !ctx || B <= 0 || S <= 0 || H <= 0 || d <= 0 || d % H || !HFN(t_bf16, attentionh_supported, S, H, d))
        return fail("gdx_attention_f16: bad argument / unsupported shape (head_dim " GDX_HEAD_DIMS ")");
    hipStream_t s = (hipStream_t)stream;
    const size_t rows = (size_t)B * S;
    _Float16 *q16 = nullptr, *c16 = nullptr;
    Scratch sc("gdx_attention_f16", s, t_bf16);
    if (sc.to_half(&q16, qkv, (int64_t)rows * 3 * d) || sc.to_half(&c16, nullptr, (int64_t)rows * d)) return -1;
    const hipError_t e = HFN(sc.bf, launch_attentionh, q16, c16, B, S, H, d, (long)rows, s);
    if (e != hipSuccess) return fail(std::string("launch_attentionh: ") + hipGetErrorString(e));
    return sc.widen(c16, ctx, (int64_t)rows * d);
}

extern "C" int gdx_attention_half(const float* qkv, int32_t qkv_rows, float* ctx, int32_t ctx_rows, int32_t B, int32_t S,
                                  int32_t H, int32_t d, int32_t dtype, int32_t kernel, int32_t grid, int32_t* launched,
                                  void* stream) {
    // every refusal comes before the first HIP call (tests/test_host_logic.py checks them without a GPU)
    if (dtype != GDX_DTYPE_F16 && dtype != GDX_DTYPE_BF16) return fail("gdx_attention_half: dtype must be GDX_DTYPE_F16 or _BF16");
    if (!qkv || !ctx || B <= 0 || S <= 0 || H <= 0 || d <= 0 || d % H || !HFN(dtype == GDX_DTYPE_BF16, attentionh_supported, S, H, d))
        return fail("gdx_attention_half: bad argument / unsupported shape (head_dim " GDX_HEAD_DIMS ")");
    if (kernel < 0 || kernel > 3) return fail("gdx_attention_half: unknown kernel (0 = dispatch, 1 = h8, 2 = h8q, 3 = h8p)");
    if (kernel >= 2 && !HFN(dtype == GDX_DTYPE_BF16, attentionh_multiblock, d / H))
        return fail("gdx_attention_half: h8q / h8p have no head_dim " + std::to_string(d / H) + " instantiation");
    if (grid < 0 || (grid > 0 && kernel != 3)) return fail("gdx_attention_half: grid is for the persistent kernel (kernel 3) only");
    if ((long)qkv_rows < (long)B * S || (long)ctx_rows < (long)B * S) return fail("gdx_attention_half: qkv_rows / ctx_rows below B*S");
    if (2 * (size_t)qkv_rows * 3 * d >= (1ull << 31) || 2 * (size_t)ctx_rows * d >= (1ull << 31))
        return fail("gdx_attention_half: a buffer exceeds the 2 GiB buffer-descriptor range; run the batch in smaller pieces");
    hipStream_t s = (hipStream_t)stream;
    const int64_t n_in = (int64_t)qkv_rows * 3 * d, n_out = (int64_t)ctx_rows * d;
    _Float16 *q16 = nullptr, *c16 = nullptr;
    Scratch sc("gdx_attention_half", s, dtype == GDX_DTYPE_BF16);
    if (sc.to_half(&q16, qkv, n_in) || sc.to_half(&c16, ctx, n_out)) return -1;
    const hipError_t e = HFN(sc.bf, launch_attentionh_kernel, q16, c16, B, S, H, d, (long)qkv_rows, kernel, grid, launched, s);
    if (e != hipSuccess) return fail(std::string("launch_attentionh_kernel: ") + hipGetErrorString(e));
    return sc.widen(c16, ctx, n_out);
}

// fp32 SDPA core on a caller's [B*S][3d] buffer (test entry point).  The kernels read whole K/V tiles past the last
// sample, so the call works on a scratch copy with GDX_ROW_PAD zero rows behind it, like the workspace of gdx_prepare.
extern "C" int gdx_attention_f32(const float* qkv, float* ctx, int32_t B, int32_t S, int32_t H, int32_t d, int32_t version,
                                 void* stream) {
    if (!qkv || !ctx || B <= 0 || S <= 0 || H <= 0 || d <= 0 || d % H) return fail("gdx_attention_f32: bad argument");
    const int hd = d / H;
    if (!head_dim_supported(hd)) return fail("gdx_attention_f32: head_dim must be " GDX_HEAD_DIMS);
    if (version == 2) return fail("gdx_attention_f32: kernel version 2 (attention2.hip) was removed in round 3");
    if ((version == 3 || version == 5) && !attention3_supported(S, H, d))
        return fail("gdx_attention_f32: shape not supported by the requested kernel");
    hipStream_t s = (hipStream_t)stream;
    const size_t rows = (size_t)B * S, prow = rows + GDX_ROW_PAD;
    float *q = nullptr, *c = nullptr;
    Scratch sc("gdx_attention_f32", s);
    if (sc.alloc(&q, sizeof(float) * prow * 3 * d) || sc.alloc(&c, sizeof(float) * prow * d)) return -1;
    if (hipMemsetAsync(q, 0, sizeof(float) * prow * 3 * d, s) != hipSuccess ||
        hipMemcpyAsync(q, qkv, sizeof(float) * rows * 3 * d, hipMemcpyDeviceToDevice, s) != hipSuccess)
        return fail("gdx_attention_f32: staging failed");
    hipError_t e;
    if (version == 5) e = launch_attention3(q, c, B, S, H, d, s, (B * H + 2) / 3);   // persistent, ~3 items per workgroup
    else if (version == 3 || (version == 0 && attention3_supported(S, H, d))) e = launch_attention3(q, c, B, S, H, d, s);
    else e = launch_attention(q, c, B, S, H, d, s);
    if (e != hipSuccess) return fail(std::string("gdx_attention_f32: ") + hipGetErrorString(e));
    if (hipMemcpyAsync(ctx, c, sizeof(float) * rows * d, hipMemcpyDeviceToDevice, s) != hipSuccess)
        return fail("gdx_attention_f32: copy-out failed");
    return 0;
}

// The same kernels on exactly the caller's buffers' extents: device copies of qkv_rows x 3d inputs (no hidden pad: what lies
// behind B*S is the caller's) and of the whole ctx_rows x d output, which comes back whole.
extern "C" int gdx_attention_f32_rows(const float* qkv, int32_t qkv_rows, float* ctx, int32_t ctx_rows, int32_t B, int32_t S,
                                      int32_t H, int32_t d, int32_t kernel, int32_t grid, int32_t* launched, void* stream) {
    // every refusal comes before the first HIP call (tests/test_host_logic.py checks them without a GPU)
    if (!qkv || !ctx || B <= 0 || S <= 0 || H <= 0 || d <= 0 || d % H) return fail("gdx_attention_f32_rows: bad argument");
    if (!head_dim_supported(d / H)) return fail("gdx_attention_f32_rows: head_dim must be " GDX_HEAD_DIMS);
    if (kernel != 0 && kernel != 1 && kernel != 3 && kernel != 5)
        return fail("gdx_attention_f32_rows: unknown kernel (0 = dispatch, 1 = attention.hip, 3 = attention3.hip, 5 = its persistent form)");
    const bool a3 = kernel == 3 || kernel == 5 || (kernel == 0 && attention3_supported(S, H, d));   // the rule of attend() (forward.hip)
    if (kernel && a3 && !attention3_supported(S, H, d))
        return fail("gdx_attention_f32_rows: shape not supported by attention3.hip (head_dim 64 / 128, at most 256 tokens)");
    if (grid < 0 || (grid > 0 && kernel != 5) || (grid == 0 && kernel == 5))
        return fail("gdx_attention_f32_rows: grid is for the persistent form (kernel 5) only, which needs one");
    if (kernel == 5 && (long)grid >= (long)B * H)
        return fail("gdx_attention_f32_rows: the persistent form walks items: grid must be below B*H");
    if ((long)qkv_rows < (long)B * S || (long)ctx_rows < (long)B * S) return fail("gdx_attention_f32_rows: qkv_rows / ctx_rows below B*S");
    if (a3 && (long)qkv_rows < (long)B * S + 64)
        return fail("gdx_attention_f32_rows: attention3.hip reads whole 64-key tiles: qkv_rows below B*S + 64");
    // attention.hip addresses with 64-bit offsets and puts the items on grid.y; attention3.hip's buffer loads carry 32-bit byte
    // offsets from each item's base and its items are an int
    if ((long)B * H > (a3 ? (1l << 31) - 1 : 65535l) || (a3 && (S + 64l) * 12 * d >= (1l << 31)))
        return fail("gdx_attention_f32_rows: a buffer exceeds the kernel's addressing (B*H items, or one sample's rows past 2 GiB)");
    hipStream_t s = (hipStream_t)stream;
    const int64_t n_in = (int64_t)qkv_rows * 3 * d, n_out = (int64_t)ctx_rows * d;
    float *q = nullptr, *c = nullptr;
    Scratch sc("gdx_attention_f32_rows", s);
    if (sc.stage(&q, qkv, n_in) || sc.stage(&c, ctx, n_out)) return -1;
    int ran[3] = {1, (S + 127) / 128, B * H};
    const hipError_t e = a3 ? launch_attention3(q, c, B, S, H, d, s, grid, ran) : launch_attention(q, c, B, S, H, d, s);
    if (e != hipSuccess) return fail(std::string("gdx_attention_f32_rows: ") + hipGetErrorString(e));
    if (launched)
        for (int i = 0; i < 3; ++i) launched[i] = ran[i];
    return sc.unstage(c, ctx, n_out);
}

extern "C" int gdx_bench_gemm_f16(int32_t M, int32_t N, int32_t K, int32_t gelu, int32_t iters, float* avg_us, void* stream) {
    if (!avg_us || M <= 0 || N <= 0 || K <= 0 || K % 64 || N % 64 || iters <= 0) return fail("gdx_bench_gemm_f16: bad argument");
    hipStream_t s = (hipStream_t)stream;
    const int npad = round_up(N, 256);
    if (2 * (size_t)M * K >= (1ull << 31) || 2 * (size_t)npad * K >= (1ull << 31))
        return fail("gdx_bench_gemm_f16: an operand exceeds the 2 GiB buffer-descriptor range");
    float *Af = nullptr, *bias = nullptr;
    _Float16 *a16 = nullptr, *w16 = nullptr, *c16 = nullptr;
    Scratch sc("gdx_bench_gemm_f16", s, t_bf16);
    const size_t nmax = (size_t)(M > npad ? M : npad) * K;
    if (sc.alloc(&Af, 4 * nmax) || sc.alloc(&bias, 4 * (size_t)npad) || sc.alloc(&c16, 2 * (size_t)M * N)) return -1;
    // non-trivial operand values (zero operands raise the clock: cdna_hip_programming.md rule 25)
    if (gdx_randn(Af, 1, (int64_t)M * K, 1, 0, 0, stream) || sc.to_half(&a16, Af, (int64_t)M * K) ||
        gdx_randn(Af, 1, (int64_t)npad * K, 2, 0, 0, stream) || sc.to_half(&w16, Af, (int64_t)npad * K) ||
        gdx_randn(bias, 1, npad, 4, 0, 0, stream))
        return fail("gdx_bench_gemm_f16: operand fill failed");
    GemmHParams p{a16, K, w16, K, (int)((size_t)M * K * 2), (int)((size_t)npad * K * 2), bias, nullptr, 0, nullptr, 0,
                  nullptr, 0, c16, N, M, N, K, 1, 0, gelu};
    GemmHCtl ctl;
    ctl.mb = t_gemmh_mb; ctl.nbw = t_gemmh_nbw;
    auto launch = [&]() { return HFN(sc.bf, launch_gemmh, p, s, &ctl) != hipSuccess ? fail("launch_gemmh failed") : 0; };
    if (time_launches(3, iters, s, avg_us, launch)) return -1;
    unsigned long long hh[48] = {0};
    if (stamped_launch(sc, hh, 48, [&](unsigned long long* st) { ctl.stamps = st; (void)launch(); })) {
        if (hh[12] && hh[11])
            fprintf(stderr, "[gemmh8 stamps] block 0, wave 0: %llu tiles, loop %.1f us at %.2f GHz; per tile: drain before the stores %.0f cycles, "
                    "epilogue (bias, convert, stores issued) %.0f; step pair in steady state %.0f cycles (%llu pairs), first two pairs after an "
                    "epilogue %.0f cycles each\n", hh[12], hh[5] / 100.0, hh[5] ? (double)hh[4] / (hh[5] * 10.0) : 0.0,
                    (double)hh[6] / hh[12], (double)hh[7] / hh[12], (double)hh[10] / hh[11], hh[11], hh[9] ? (double)hh[8] / hh[9] : 0.0);
        if (hh[3])
            fprintf(stderr, "[gemmh stamps] loader wave, block 0: %llu steps; per step: issue %.0f, vmcnt wait %.0f, barrier wait %.0f, total %.0f cycles; loop %.1f us -> s_memtime at %.2f GHz\n",
                    hh[3], (double)hh[0] / hh[3], (double)hh[1] / hh[3], (double)hh[2] / hh[3], (double)hh[4] / hh[3],
                    hh[5] / 100.0, hh[5] ? (double)hh[4] / (hh[5] * 10.0) : 0.0);
    }
    return 0;
}

// Stand-alone attention timing on scratch buffers (measurement helper for tools/attn_one.py).
extern "C" int gdx_bench_attention(int32_t B, int32_t S, int32_t H, int32_t d, int32_t version, int32_t iters,
                                   float* avg_us, void* stream) {
    if (!avg_us || B <= 0 || S <= 0 || H <= 0 || d <= 0 || d % H || iters <= 0) return fail("gdx_bench_attention: bad argument");
    if (!head_dim_supported(d / H)) return fail("gdx_bench_attention: head_dim must be " GDX_HEAD_DIMS);
    hipStream_t s = (hipStream_t)stream;
    float *qkv = nullptr, *ctx = nullptr;
    Scratch sc("gdx_bench_attention", s, t_bf16);
    const size_t rows = (size_t)B * S + GDX_ROW_PAD;
    if (sc.alloc(&qkv, sizeof(float) * rows * 3 * d) || sc.alloc(&ctx, sizeof(float) * rows * d)) return -1;
    HIPCHK(gdx_randn(qkv, 1, (int64_t)rows * 3 * d, 5, 0, 0, stream) ? hipErrorUnknown : hipSuccess);
    _Float16 *qkv16 = nullptr, *ctx16 = nullptr;
    if (version == 3) {
        if (!HFN(sc.bf, attentionh_supported, S, H, d)) return fail("gdx_bench_attention: shape not supported by the fp16 kernel");
        if (sc.to_half(&qkv16, qkv, (int64_t)rows * 3 * d) || sc.to_half(&ctx16, nullptr, (int64_t)rows * d)) return -1;
    }
    auto run = [&](unsigned long long* stamps) -> int {
        if (version == 3) HIPCHK(HFN(sc.bf, launch_attentionh_kernel, qkv16, ctx16, B, S, H, d, (long)rows, 0, 0, nullptr, s, stamps));
        else if (version == 4 && attention3_supported(S, H, d)) HIPCHK(launch_attention3(qkv, ctx, B, S, H, d, s));
        else HIPCHK(launch_attention(qkv, ctx, B, S, H, d, s));
        return 0;
    };
    if (time_launches(3, iters, s, avg_us, [&] { return run(nullptr); })) return -1;
    unsigned long long hh[16] = {0};
    // (the stamps exist in the persistent fp16 kernel only)
    if (version == 3 && stamped_launch(sc, hh, 16, [&](unsigned long long* st) { (void)run(st); })) {
        for (int wv = 0; wv < 2; ++wv) {
            const unsigned long long* o = hh + 8 * wv;
            if (o[5])
                fprintf(stderr, "[attentionh8p stamps] workgroup 0, wave %d: %llu tiles, kernel %.1f us at %.2f GHz; cycles per tile: DMA issue %.0f, "
                        "QK^T %.0f, softmax %.0f, PV %.0f, wait + barrier %.0f\n", wv ? 7 : 0, o[5], o[7] / 100.0,
                        o[7] ? (double)o[6] / (o[7] * 10.0) : 0.0, (double)o[0] / o[5], (double)o[1] / o[5], (double)o[2] / o[5],
                        (double)o[3] / o[5], (double)o[4] / o[5]);
        }
    }
    return 0;
}
