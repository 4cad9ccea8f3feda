// Device one-liners shared by the kernel files of libgdx.so (gfx950 only): vector types, the 16-bit MFMA of the build's half
// type, the counted vector-memory wait, the wave sum and the XCD-contiguous workgroup id.  Included after gdx_internal.h.
#pragma once
#include "gdx_internal.h"

// the 16x16x32 MFMA of half_t (fp16, or bf16 under -DGDX_BF16)
#ifdef GDX_BF16
#define GDX_MFMA16 __builtin_amdgcn_mfma_f32_16x16x32_bf16
#else
#define GDX_MFMA16 __builtin_amdgcn_mfma_f32_16x16x32_f16
#endif

namespace gdx {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef half_t f16x8 __attribute__((ext_vector_type(8)));
typedef half_t f16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;

// s_waitcnt vmcnt(N): all but the youngest N vector-memory operations of the wave have retired
template <int N>
__device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// sum over the 64 lanes of the wave, in every lane
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Logical workgroup id with the workgroups of one XCD contiguous (blocks b, b + 8, b + 16, ... share an XCD and its L2; bijective
// for any grid size G).  Work that shares operands gets consecutive logical ids and so runs on ONE XCD at about the same time:
// the tiles of an A row-panel in the GEMMs, the query chunks of one (sample, head) in the 16-bit attention, whose K / V tiles
// are then fetched into that L2 once instead of once per chunk through different L2s.
__device__ __forceinline__ int xcd_lid(int bid, int G) {
    const int q = G >> 3, r = G & 7, xcd = bid & 7, idx = bid >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

}  // namespace gdx
