// Encoder self-attention core of the fp16 mode: softmax(Q K^T / sqrt(hd)) V per (sample, head) on
// v_mfma_f32_16x16x32_f16, fp32 scores / softmax / accumulators, fp16 Q, K, V, P operands and output.
//   qkv [B*S][3d] halves (q | k | v, heads contiguous inside each)  ->  ctx [B*S][d] halves.
//
// Structure: one 512-thread workgroup per (sample, head, query chunk) -- or, persistent, per CU walking such items; all eight
// waves compute, each keeps one or two query blocks of 16 resident (Q fragments + O^T accumulators in registers), walks all
// K/V tiles of 32 keys once and issues 1/8 of every tile's LDS-DMA into a 3-stage ring (counted vmcnt, raw barriers); behind the
// ring every wave owns a 16-row slice of LDS through which its Q fragments arrive and its output blocks leave as WHOLE ROWS
// (round 3: loaded / stored in the fragment layout they were 6 144 partial-line requests per workgroup and item).
// (The first kernel of this file, 4 compute + 4 loader waves, was removed in round 3; restructures that were measured and
// not kept -- one wave per SIMD with 512 registers, SIMD partners rotated by half a tile -- are recorded in
// profiles/r03b_fp16_attention_experiments.txt.)
//   * S^T = K Q^T (K fragment = A operand, ds_read_b128 of 8 consecutive head-dim halves of one key): the query sits
//     on the accumulator's lane axis, so max / sum / rescale are per-lane scalars and the 8 probabilities a lane
//     holds for a 32-key tile (2 blocks x 4 registers), rounded to fp16, ARE the B operand of the next product --
//     with the key order of the k axis chosen to match (k slot 8g + j <-> key 16*(j>>2) + 4g + (j&3));
//   * O^T += V^T P^T: the A operand needs V column-wise; V stays row-major in LDS (as it comes from HBM) and is read
//     with ds_read_b64_tr_b16 (hardware transpose: two reads = 8 keys x 16 head-dim columns per lane group);
//   * LDS rows are un-padded (LDS-DMA is lane-linear); the 16-byte chunks of a row are permuted,
//     phys = chunk ^ f(row), f = (row & 7) << 1 (rows of >= 256 B), ((row >> 1) & 3) << 1 (128-B rows) or
//     ((row >> 2) & 1) << 1 (64-B rows), on the DMA
//     source address and on both kinds of read: every ds_read_b128 lane group and every 32-lane half of a
//     transposed read then covers all 64 banks exactly once;  head_dim 96 / 192 (rows of 12 / 24 chunks, 8 x 1 kernel only)
//     take the function of the power-of-two row with the same stride mod 256 B -- see ah_fswz;
//   * deferred max in the log2 domain: the reference value is raised (cross-lane shuffles + O rescale) only when a
//     score exceeds it by more than 8 (p <= 2^8 is far inside fp16 range; the running sum and O are fp32).
// K/V rows past S are the next sample's rows or read as zeros (exact buffer size in the descriptor); their scores
// are masked to -inf.  (The head_dim 96 / 192 instantiations re-read key S - 1 instead and never look past the sample.)
//
// Layout of this file: the three kernels (8 waves x 1 block, 8 x 2 blocks, 8 x 2 persistent) are the same arithmetic per query
// block, and every piece of it is written ONCE, in front of them: the geometry (AhGeom), the per-wave DMA piece table and the
// piece loop of one stage (ah_piece_table, ah_issue), the fragment addresses (AhFrag), the tile body (ah_qk, ah_v_prefetch,
// ah_softmax, ah_pv, composed by ah_tile with a stamp hook between the pieces), the stage hand-over (ah_handover), Q through
// the slice (ah_q_dma, ah_q_read), the output (ah_inv_l, ah_store_rows) and an item's geometry (ah_item); the one-liners shared with the other kernel files
// (xcd_lid, wait_vm, GDX_MFMA16, vector types) are in gdx_device.h.  A kernel is what is
// left: which tile / item the stream fetches next, when Q arrives and when the output leaves.  The host side likewise has one
// launcher template (launch_ah), one head-width ladder and one function for the (chunks, items, grid) of a kernel (ah_plan).
#include "gdx_internal.h"
#include "gdx_device.h"

#include <cstdlib>
#include <type_traits>

namespace gdx {
int gemm2_num_cus();
GDX_HNS_BEGIN

typedef __fp16 fp16x4_t __attribute__((__vector_size__(4 * sizeof(__fp16))));
typedef __amdgpu_buffer_rsrc_t ah_rsrc_t;

// bytes readable from a (sample, head) base: the descriptor's range check only matters at the very end of the buffer,
// so a remaining size above the 2 GiB descriptor range is clamped (a workgroup reads < S + 32 rows from its base)
__device__ __forceinline__ int ah_records(long remaining) { return remaining > 0x7ffffff0L ? 0x7ffffff0 : (int)remaining; }

// descriptor of the rest of qkv from element `off` on
__device__ __forceinline__ ah_rsrc_t ah_rsrc(const _Float16* qkv, long off, long qkv_bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(qkv + off), (short)0, ah_records(qkv_bytes - off * 2), 0x00020000);
}

__device__ __forceinline__ f16x4 lds_read_tr(const char* p) {
    const fp16x4_t v = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fp16x4_t*)(p));
    return __builtin_bit_cast(f16x4, v);
}

// The chunk swizzle: 16-byte chunk c of tile row `row` lives at chunk c ^ ah_fswz<HD>(row) of that row.  What decides the banks
// is the row stride mod the 256-byte bank row, so a row of 12 chunks (head_dim 96, 192 B = 256 - 64) takes the function of the
// 64-byte row and a row of 24 chunks (head_dim 192, 384 B = 256 + 128) that of the 128-byte row.  The function is even and below
// 4 (96) / 8 (192), and 12 / 24 chunks are whole multiples of 4 / 8: the XOR permutes chunks inside an aligned group of 4 / 8 and
// never leaves the row, and the two chunks of a 16-column block stay adjacent for the transposed reads.
// Bank argument, slot = 16-byte position mod 16 inside the bank row, key row r = lane & 15, lq = lane >> 4, k-step ks:
//   ds_read_b128 (K, Q fragments; a lane group is rows {0-3, 12-15} at lq and rows {4-11} at lq + 1, lq even -- or the converse):
//     96:  slot = 12 r + ((4 ks + lq) ^ f) = 4 ((ks - r) mod 4) + 2 bit2(r) + (lq & 1) (+ 2 for lq >= 2): rows 0-3 / 12-15 differ in
//          (r mod 4, bit2), rows 4-7 / 8-11 likewise, and the two row sets differ in lq & 1 -- 16 slots, each once.
//     192: slot = 8 r + ((4 ks + lq) ^ f) = const ^ (lq & 1) ^ 2 ((r >> 1) & 3) ^ 8 (r & 1): bits 1-3 spell r mod 8, which is
//          0..7 over rows {0-3, 12-15} and over rows {4-11}, and bit 0 tells the two sets apart -- 16 slots, each once.
//   ds_read_b64_tr_b16 (V; a 32-lane half is 8 consecutive rows v, four lanes on each 32-byte block nb ^ (f >> 1)):
//     96:  32-byte position mod 8 = 6 v + (nb ^ bit2(v)): {0, 6, 4, 2} + nb for v = 0..3 and the same set moved by one for
//          v = 4..7 -- eight positions, each once.
//     192: 12 v + (nb ^ ((v >> 1) & 3)) = nb ^ ((v >> 1) & 3) ^ 4 (v & 1): the low three bits spell v -- each once.
// Row + 16 has the same f in every case, so the second 16-key block of a tile is the first one 16 rows further on.
template <int HD>
__device__ __forceinline__ constexpr int ah_fswz(int row) {
    constexpr int RM = (HD * 2) % 256;
    static_assert(HD == 32 || HD == 64 || HD == 96 || HD == 128 || HD == 192 || HD == 256, "no chunk swizzle for this head_dim");
    return RM == 64 || RM == 192 ? ((row >> 2) & 1) << 1 : RM == 128 ? ((row >> 1) & 3) << 1 : (row & 7) << 1;
}

// ---------------------------------------------------------------------------------------------------------------
// Geometry of a head width: the kernels' pointer arithmetic and the launcher's LDS size both read it here.  A stage of the ring is
// a K tile and a V tile of 32 rows; a tile is T_P pieces of 1 KiB (one LDS-DMA instruction of a wave), a wave issues PW of the
// 2 T_P pieces of a stage.  SLICES: eight 16-row slices, one per wave, behind the ring (Q in, output out, as whole rows).
template <int HD_, int NST_, bool SLICES>
struct AhGeom {
    static constexpr int HD = HD_, NST = NST_;
    static constexpr int ROWB = HD * 2, CPR = ROWB / 16, T_BYTES = 32 * ROWB, STAGE_BYTES = 2 * T_BYTES;
    static constexpr int T_P = T_BYTES / 1024, P = 2 * T_P, PW = (P + 7) / 8;
    static constexpr int NKS = HD / 32, NNB = HD / 16;
    static constexpr int NR = 2 * NKS, PD = NR < 4 ? NR - 1 : 3;        // K fragment reads of a tile, depth of their register ring
    static constexpr int VD = NNB < 4 ? NNB - 1 : 3;                    // depth of the V ring
    static constexpr bool POW2 = (HD & (HD - 1)) == 0;                  // rows of 12 / 24 chunks (head_dim 96 / 192) otherwise
    static constexpr int RPP = 1024 / ROWB;                             // rows per 1 KiB piece (16 at head_dim 32)
    static constexpr int NPQ = 16 / RPP;                                // pieces per 16-row block
    static constexpr int GM = CPR < 16 ? CPR - 1 : 15;                  // row mask of the output slice's chunk permutation
    static constexpr int RING_BYTES = NST * STAGE_BYTES, SLICE_BYTES = 16 * ROWB;
    static constexpr int LDS_BYTES = RING_BYTES + (SLICES ? 8 * SLICE_BYTES : 0);
    static constexpr int VM_TILE = (NST - 2) * PW;                      // a wave's DMA still in flight when its next tile has landed
    static_assert(!SLICES || POW2, "whole rows per 1 KiB piece and XOR-composed fragment addresses: power-of-two head_dim only");
};
template <int HD> using AhGeom1 = AhGeom<HD, 4, false>;                 // 8 waves x 1 block
template <int HD> using AhGeom2 = AhGeom<HD, 3, true>;                  // 8 waves x 2 blocks, also persistent

constexpr float AH_RESCALE_THR = 8.0f;

// ---- the K/V stream ---------------------------------------------------------------------------------------------
// This wave's pieces (piece = wave + 8i) of every tile: a 1 KiB piece is 64 consecutive chunks of the tile image, whole rows
// (power-of-two head_dim) or not: lane -> (row, physical chunk) -> source address.  CLAMP: the table of the LAST tile at
// head_dim 96 / 192, whose rows past key S - 1 (row_cap) re-read key S - 1 (as the Q rows do), so nothing past the sample is
// ever read: a masked key has p = 0, but 0 x V is only 0 for a finite V, and the rows behind the last sample are the caller's.
template <class G, bool CLAMP>
__device__ __forceinline__ void ah_piece_table(int (&voff)[G::PW], int wave, int lane, long ld, int row_cap = 0) {
#pragma unroll
    for (int i = 0; i < G::PW; ++i) {
        int piece = wave + 8 * i;
        piece = piece < G::P ? piece : G::P - 1;
        const int pl = piece < G::T_P ? piece : piece - G::T_P;
        const int g = G::POW2 ? lane : pl * 64 + lane;
        const int row = G::POW2 ? pl * G::RPP + lane / G::CPR : g / G::CPR;
        voff[i] = (int)((CLAMP ? min(row, row_cap) : row) * ld * 2) + (((g % G::CPR) ^ ah_fswz<G::HD>(row)) * 16);
    }
}

// One stage's LDS-DMA of this wave: EVERY wave issues exactly PW pieces per tile, whatever it computes -- the counted
// wait_vm<G::VM_TILE> is only right then.  `last` (wave-uniform) takes the offsets from voff_l.
template <class G>
__device__ __forceinline__ void ah_issue(ah_rsrc_t rsrcK, ah_rsrc_t rsrcV, char* sb, const int (&voff)[G::PW],
                                         const int (&voff_l)[G::PW], bool last, int so, int wave) {
#pragma unroll
    for (int i = 0; i < G::PW; ++i) {
        int piece = wave + 8 * i;
        piece = piece < G::P ? piece : G::P - 1;                        // surplus issues (head_dim 32, 96) re-write the last piece
        const int vo = last ? voff_l[i] : voff[i];
        if (piece < G::T_P)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrcK, (lds_ptr_t)(sb + piece * 1024), 16, vo, so, 0, 0);
        else
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrcV, (lds_ptr_t)(sb + G::T_BYTES + (piece - G::T_P) * 1024), 16, vo, so, 0, 0);
    }
}

// Stage hand-over at the end of a tile: this wave's pieces of the next tile have landed, its fragment reads of this one are
// done; behind the barrier that holds for all waves, and the stage just read is the one the next issue may overwrite.
template <class G>
__device__ __forceinline__ void ah_handover(int& stage, int& wst) {
    wait_vm<G::VM_TILE>();
    __builtin_amdgcn_s_waitcnt(0xc07f);                                 // lgkmcnt(0)
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    stage = stage == G::NST - 1 ? 0 : stage + 1;
    wst = wst == G::NST - 1 ? 0 : wst + 1;
}

// ---- fragment addresses -------------------------------------------------------------------------------------------
// K fragment r of a stage (or of a slice holding a query block): rows l15 (+ 16 for the second key block), k-step r % NKS;
// V fragment: column block nb, key half.  Power-of-two rows start on a 256-byte boundary, so the swizzle is folded into the
// base and the k-step / column block XORed on top; rows of 12 / 24 chunks do not, and there the chunk (32-byte block) index is
// formed first, then added to the row.
template <class G>
struct AhFrag {
    int kb, kz, vb, vz, lq;
    __device__ __forceinline__ AhFrag(int l15, int lq_) : lq(lq_) {
        const int vrow = 4 * lq + (l15 >> 2);
        kz = ah_fswz<G::HD>(l15);
        vz = ah_fswz<G::HD>(vrow) >> 1;
        kb = l15 * G::ROWB + (G::POW2 ? (lq ^ kz) << 4 : 0);
        vb = G::T_BYTES + vrow * G::ROWB + (G::POW2 ? vz << 5 : 0) + (l15 & 3) * 8;
    }
    __device__ __forceinline__ f16x8 kread(const char* St, int r) const {
        if constexpr (G::POW2)
            return *reinterpret_cast<const f16x8*>(St + ((kb + (r / G::NKS) * 16 * G::ROWB) ^ ((r % G::NKS) << 6)));
        else
            return *reinterpret_cast<const f16x8*>(St + kb + (r / G::NKS) * 16 * G::ROWB + (((lq + 4 * (r % G::NKS)) ^ kz) << 4));
    }
    __device__ __forceinline__ f16x4 vread(const char* St, int nb, int half) const {
        if constexpr (G::POW2) return lds_read_tr(St + ((vb + half * 16 * G::ROWB) ^ (nb << 5)));
        else return lds_read_tr(St + vb + half * 16 * G::ROWB + ((nb ^ vz) << 5));
    }
};

// ---- the tile body ------------------------------------------------------------------------------------------------
// S^T = K Q^T for the wave's NQ query blocks, K fragments through a register ring PD reads ahead
template <class G, int QB, int NQ>
__device__ __forceinline__ void ah_qk(const AhFrag<G>& fr, const char* St, const f16x8 (&qf)[QB][G::NKS], f32x4 (&s)[NQ][2]) {
#pragma unroll
    for (int qi = 0; qi < NQ; ++qi) s[qi][0] = s[qi][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    f16x8 kring[G::PD + 1];
#pragma unroll
    for (int r = 0; r < G::PD; ++r) kring[r] = fr.kread(St, r);
#pragma unroll
    for (int r = 0; r < G::NR; ++r) {
        if (r + G::PD < G::NR) kring[(r + G::PD) % (G::PD + 1)] = fr.kread(St, r + G::PD);
#pragma unroll
        for (int qi = 0; qi < NQ; ++qi)
            s[qi][r / G::NKS] = GDX_MFMA16(kring[r % (G::PD + 1)], qf[qi][r % G::NKS], s[qi][r / G::NKS], 0, 0, 0);
    }
}

// the first VD column blocks of V, on their way while the softmax runs
template <class G>
__device__ __forceinline__ void ah_v_prefetch(const AhFrag<G>& fr, const char* St, f16x4 (&vring)[G::VD + 1][2]) {
#pragma unroll
    for (int nb = 0; nb < G::VD; ++nb) {
        vring[nb][0] = fr.vread(St, nb, 0);
        vring[nb][1] = fr.vread(St, nb, 1);
    }
}

// One query block's softmax step on the raw scores of tile kt; the scale (log2 e / sqrt(hd) > 0) is applied inside the exp2
// argument (one fma per element).  Returns the 8 probabilities of the lane, packed: the B operand of P V.
template <class G>
__device__ __forceinline__ f16x8 ah_softmax(const f32x4 (&s)[2], int kt, int S, int lq, float c_log2, float& m_run, float& l_run,
                                            f32x4 (&o)[G::NNB]) {
    float v[8];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int e = 0; e < 4; ++e) v[kb * 4 + e] = s[kb][e];
    if (kt * 32 + 32 > S) {                                             // block-uniform: only the last tile masks
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (kt * 32 + (j >> 2) * 16 + 4 * lq + (j & 3) >= S) v[j] = -INFINITY;
    }
    float mx = fmaxf(fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])), fmaxf(fmaxf(v[4], v[5]), fmaxf(v[6], v[7]))) * c_log2;
    if (__any(mx > m_run + AH_RESCALE_THR)) {                           // every lane votes, also those of query rows past S
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float m_new = fmaxf(m_run, mx);
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
        l_run *= alpha;
#pragma unroll
        for (int nb = 0; nb < G::NNB; ++nb) o[nb] *= alpha;
        m_run = m_new;
    }
    float psum = 0.0f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        v[j] = __builtin_amdgcn_exp2f(fmaf(v[j], c_log2, -m_run));
        psum += v[j];
    }
    l_run += psum;
    return f16x8{(half_t)v[0], (half_t)v[1], (half_t)v[2], (half_t)v[3], (half_t)v[4], (half_t)v[5], (half_t)v[6], (half_t)v[7]};
}

// O^T += V^T P^T, V fragments through a ring VD column blocks ahead (ah_v_prefetch filled it)
template <class G, int QB, int NQ>
__device__ __forceinline__ void ah_pv(const AhFrag<G>& fr, const char* St, f16x4 (&vring)[G::VD + 1][2], const f16x8 (&pf)[NQ],
                                      f32x4 (&o)[QB][G::NNB]) {
#pragma unroll
    for (int nb = 0; nb < G::NNB; ++nb) {
        if (nb + G::VD < G::NNB) {
            vring[(nb + G::VD) % (G::VD + 1)][0] = fr.vread(St, nb + G::VD, 0);
            vring[(nb + G::VD) % (G::VD + 1)][1] = fr.vread(St, nb + G::VD, 1);
        }
        const f16x4 v0 = vring[nb % (G::VD + 1)][0], v1 = vring[nb % (G::VD + 1)][1];
        const f16x8 vf = f16x8{v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
#pragma unroll
        for (int qi = 0; qi < NQ; ++qi) o[qi][nb] = GDX_MFMA16(vf, pf[qi], o[qi][nb], 0, 0, 0);
    }
}

// Diagnostic stamps of the persistent kernel (GDX_GEMM_DEBUG only): cycles per tile spent issuing the DMA pieces, in QK^T, in
// the softmax, in PV and in the wait + barrier.  The plain build carries an empty hook.
template <bool DBG>
struct AhStamps {
    unsigned long long d_is = 0, d_qk = 0, d_sm = 0, d_pv = 0, d_bar = 0, n_t = 0, t_a = 0;
    __device__ __forceinline__ void start() {
        if constexpr (DBG) { __builtin_amdgcn_sched_barrier(0); t_a = __builtin_amdgcn_s_memtime(); }
    }
    __device__ __forceinline__ void mark(unsigned long long& acc) {
        if constexpr (DBG) {
            __builtin_amdgcn_sched_barrier(0);
            const unsigned long long t_b = __builtin_amdgcn_s_memtime();
            acc += t_b - t_a;
            t_a = t_b;
        }
    }
};

// One K/V tile for the wave's NQ (of QB) query blocks; NQ = 0: a wave without a block only streams.
template <class G, int QB, int NQ, bool DBG>
__device__ __forceinline__ void ah_tile(const AhFrag<G>& fr, const char* St, const f16x8 (&qf)[QB][G::NKS], int kt, int S, float c_log2,
                                        float (&m_run)[QB], float (&l_run)[QB], f32x4 (&o)[QB][G::NNB], AhStamps<DBG>& st) {
    if constexpr (NQ > 0) {
        f32x4 s[NQ][2];
        ah_qk<G, QB, NQ>(fr, St, qf, s);
        st.mark(st.d_qk);
        f16x4 vring[G::VD + 1][2];
        ah_v_prefetch<G>(fr, St, vring);
        f16x8 pf[NQ];
#pragma unroll
        for (int qi = 0; qi < NQ; ++qi) pf[qi] = ah_softmax<G>(s[qi], kt, S, fr.lq, c_log2, m_run[qi], l_run[qi], o[qi]);
        st.mark(st.d_sm);
        ah_pv<G, QB, NQ>(fr, St, vring, pf, o);
    }
    st.mark(st.d_pv);
}

// ---- items, Q through the slice, output -----------------------------------------------------------------------------
// Work item w = (sample, head, query chunk): element offset of its (sample, head) inside qkv, its first query block and its block
// count (<= 8 * QB).  SCALAR: the results are forced into scalar registers -- integer division runs on the vector ALU, and
// without the readfirstlanes these wave-uniform values sit in vector registers through the whole tile loop of the persistent
// kernel, which has none to spare.
struct AhItem {
    long off;
    int b, h, qb_lo, nblk;
};
template <bool SCALAR>
__device__ __forceinline__ AhItem ah_item(int w, int nchunk, int H, int S, long ld, int hd) {
    auto u = [](int x) { return SCALAR ? __builtin_amdgcn_readfirstlane(x) : x; };
    const int nqb = (S + 15) / 16;
    AhItem it;
    const int ci = u(w % nchunk);
    it.h = u((w / nchunk) % H);
    it.b = u(w / (nchunk * H));
    it.off = (long)it.b * S * ld + it.h * hd;
    it.qb_lo = u((int)((long)ci * nqb / nchunk));
    it.nblk = u((int)((long)(ci + 1) * nqb / nchunk)) - it.qb_lo;
    return it;
}
// the query blocks of a chunk go to the waves round-robin: blocks qb_lo + wave + 8 qi, qi < this
template <int QB>
__device__ __forceinline__ int ah_my_blocks(int nblk, int wave) { return wave < nblk ? min((nblk - wave + 7) / 8, QB) : 0; }

// Q fragments and output blocks travel as WHOLE ROWS through the wave's own 16-row slice of LDS (behind the K/V ring).
// Loaded straight into the fragment layout a Q load instruction takes 64 bytes from each of 16 rows, and an output store puts
// 32 bytes into each of 16 rows: 6 144 partial-line requests per workgroup and item, which the CU's address unit serves at
// about two cycles each -- round-3 stamps: 6-10 k cycles to ISSUE a wave's 16 Q loads and 5.9 k for its 32 stores, ~13 us per
// item outside the tile loop.  A query block is 16 rows of ROWB bytes, exactly a 16-key K block: staged by LDS-DMA with K's
// chunk swizzle it is read back with K's fragment read; an output block is written to the slice in the accumulator layout
// (chunk-swizzled by row) and leaves as 16-byte pieces of whole rows.
// Rows past S repeat row S - 1 (as in attentionh8_kernel): a query that is never stored still takes part in the block's
// rescale vote, so it must not come from the next sample or the pad -- or a sample's bits would depend on its neighbours.
template <class G>
__device__ __forceinline__ void ah_q_dma(ah_rsrc_t rsrcQ, char* sl, int q0, int S, long ld, int ln) {
#pragma unroll
    for (int j = 0; j < G::NPQ; ++j) {
        const int row = j * G::RPP + ln / G::CPR;
        const int vo = (int)(min(q0 + row, S - 1) * ld * 2) + (((ln % G::CPR) ^ ah_fswz<G::HD>(row)) * 16);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrcQ, (lds_ptr_t)(sl + j * 1024), 16, vo, 0, 0, 0);
    }
}
template <class G>
__device__ __forceinline__ void ah_q_read(const AhFrag<G>& fr, const char* sl, f16x8 (&qf)[G::NKS]) {
#pragma unroll
    for (int ks = 0; ks < G::NKS; ++ks) qf[ks] = fr.kread(sl, ks);
}
template <class G>
__device__ __forceinline__ void ah_q_zero(f16x8 (&qf)[G::NKS]) {
#pragma unroll
    for (int ks = 0; ks < G::NKS; ++ks) qf[ks] = f16x8{0, 0, 0, 0, 0, 0, 0, 0};
}

// 1 / (the softmax denominator of the lane's query): the four lanes of a query hold a quarter of the keys each
__device__ __forceinline__ float ah_inv_l(float l_run) {
    float l_tot = l_run;
    l_tot += __shfl_xor(l_tot, 16);
    l_tot += __shfl_xor(l_tot, 32);
    return 1.0f / l_tot;
}

// Output of the wave's query blocks (the first `mine` of QB; block qi is query block qb0 + 8 qi): a lane holds columns
// 16 nb + 4 lq .. + 3 of query l15; through the slice (16-byte chunk c of row r at c ^ (r mod chunks-per-row, at most 16): the
// sixteen rows of a column land in sixteen different bank groups) and out as whole rows.  ln: the lane id (the persistent kernel
// passes its laundered copy).  The loop over the blocks is in here on purpose: as a helper for ONE block, called from a loop in the
// kernel, it cost attentionh8p_kernel<256, 2> 33 spilled registers instead of 2 (profiles/attnh_once_isa_compare.txt).
template <class G, int QB>
__device__ __forceinline__ void ah_store_rows(const f32x4 (&o)[QB][G::NNB], const float (&l_run)[QB], int mine, char* sl, int ln,
                                              _Float16* ctx, int b, int h, int qb0, int S, int d) {
    const int e15 = ln & 15, eq = ln >> 4;
#pragma unroll
    for (int qi = 0; qi < QB; ++qi) {
        if (qi >= mine) continue;
        const float inv = ah_inv_l(l_run[qi]);
#pragma unroll
        for (int nb = 0; nb < G::NNB; ++nb) {
            const f32x4 r = o[qi][nb] * inv;
            *reinterpret_cast<f16x4*>(sl + e15 * G::ROWB + (((2 * nb + (eq >> 1)) ^ (e15 & G::GM)) << 4) + (eq & 1) * 8) =
                f16x4{(half_t)r[0], (half_t)r[1], (half_t)r[2], (half_t)r[3]};
        }
        const int q0 = 16 * (qb0 + 8 * qi);
#pragma unroll
        for (int j = 0; j < G::NPQ; ++j) {
            const int row = j * G::RPP + ln / G::CPR, c = ln % G::CPR;
            const f16x8 v = *reinterpret_cast<const f16x8*>(sl + row * G::ROWB + ((c ^ (row & G::GM)) << 4));
            if (q0 + row < S) *reinterpret_cast<f16x8*>(ctx + ((long)b * S + q0 + row) * d + h * G::HD + 8 * c) = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Eight compute waves, every wave owns ONE query block of 16 and issues 1/8 of the K/V tile DMA itself.
// With one MFMA wave per SIMD (the removed 4 + 4 kernel) the softmax VALU work, the fragment-read latency and the MFMAs of a
// wave are serial (measured 3 300 cycles per 32-key tile at head_dim 256 against 1 024 cycles of MFMA); two waves
// per SIMD cover each other's softmax and LDS latency, and a wave needs half the registers (64 accumulators + 32
// Q-fragment registers at head_dim 256), which leaves room for the fragment prefetch rings.
template <int HD>
__global__ __launch_bounds__(512, 1) void attentionh8_kernel(const _Float16* __restrict__ qkv, _Float16* __restrict__ ctx,
                                                             int S, int H, int d, int nchunk, float c_log2,
                                                             long qkv_bytes) {
#if defined(__HIP_DEVICE_COMPILE__)
    using G = AhGeom1<HD>;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid) >> 6;
    const int l15 = lane & 15, lq = lane >> 4;
    const long ld = 3L * d;
    const AhItem im = ah_item<false>(xcd_lid((int)blockIdx.x, (int)gridDim.x), nchunk, H, S, ld, HD);
    const int ntiles = (S + 31) / 32;
    const bool mine = wave < im.nblk;                                 // wave-uniform

    // ---- Q fragments first (ordinary loads: their wait must not sit behind the DMA stream)
    f16x8 qf[1][G::NKS];
    {
        int q = 16 * (im.qb_lo + wave) + l15;
        q = q < S ? q : S - 1;
        const _Float16* qp = qkv + im.off + (long)q * ld + 8 * lq;
#pragma unroll
        for (int ks = 0; ks < G::NKS; ++ks) qf[0][ks] = *reinterpret_cast<const f16x8*>(qp + 32 * ks);
    }
    wait_vm<0>();

    // ---- the K/V stream: past the end, harmless re-reads of the last tile
    const ah_rsrc_t rsrcK = ah_rsrc(qkv, im.off + d, qkv_bytes), rsrcV = ah_rsrc(qkv, im.off + 2 * d, qkv_bytes);
    int voff[G::PW], voff_l[G::PW];
    ah_piece_table<G, false>(voff, wave, lane, ld);
    ah_piece_table<G, !G::POW2>(voff_l, wave, lane, ld, S - 1 - 32 * (ntiles - 1));
    int ld_kt = 0;
    auto issue = [&](int stage) {
        ah_issue<G>(rsrcK, rsrcV, smem + stage * G::STAGE_BYTES, voff, voff_l, !G::POW2 && ld_kt == ntiles - 1,
                    (int)((long)ld_kt * 32 * ld * 2), wave);
        ld_kt = ld_kt + 1 < ntiles ? ld_kt + 1 : ntiles - 1;
    };

    f32x4 o[1][G::NNB];
#pragma unroll
    for (int nb = 0; nb < G::NNB; ++nb) o[0][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run[1] = {-INFINITY}, l_run[1] = {0.0f};
    const AhFrag<G> fr(l15, lq);
    AhStamps<false> st;

#pragma unroll
    for (int s = 0; s < G::NST - 1; ++s) issue(s);
    wait_vm<G::VM_TILE>();                                            // this wave's pieces of tile 0
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    int stage = 0, wst = G::NST - 1;
    for (int kt = 0; kt < ntiles; ++kt) {
        const char* St = smem + stage * G::STAGE_BYTES;
        issue(wst);                                                   // tile kt+NST-1 -> the stage freed by the last barrier
        if (mine) ah_tile<G, 1, 1>(fr, St, qf, kt, S, c_log2, m_run, l_run, o, st);
        ah_handover<G>(stage, wst);
    }
    wait_vm<0>();
    if (mine) {
        const float inv = ah_inv_l(l_run[0]);
        const int q = 16 * (im.qb_lo + wave) + l15;
        if (q < S) {
            _Float16* op = ctx + ((long)im.b * S + q) * d + im.h * HD + 4 * lq;
#pragma unroll
            for (int nb = 0; nb < G::NNB; ++nb) {
                const f32x4 r = o[0][nb] * inv;
                *reinterpret_cast<f16x4*>(op + 16 * nb) = f16x4{(half_t)r[0], (half_t)r[1], (half_t)r[2], (half_t)r[3]};
            }
        }
    }
#endif
}

// ---------------------------------------------------------------------------------------------------------------
// Eight compute waves x QB = 2 query blocks each (256 queries per workgroup): the K/V fragments are shared by a wave's
// two blocks, every K/V tile is staged once for twice as many queries, and the two waves of a SIMD cover each other's
// softmax / latency as in the kernel above.  The query blocks of a chunk go to the waves round-robin (block
// qb_lo + w + 8 qi), so the two waves of a SIMD (w, w + 4) hold 4, 3 or 2 blocks between them.
template <int HD, int QB>
__global__ __launch_bounds__(512, 1) void attentionh8q_kernel(const _Float16* __restrict__ qkv, _Float16* __restrict__ ctx,
                                                              int S, int H, int d, int nchunk, float c_log2,
                                                              long qkv_bytes) {
#if defined(__HIP_DEVICE_COMPILE__)
    using G = AhGeom2<HD>;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid) >> 6;
    const int l15 = lane & 15, lq = lane >> 4;
    const long ld = 3L * d;
    const AhItem im = ah_item<false>(xcd_lid((int)blockIdx.x, (int)gridDim.x), nchunk, H, S, ld, HD);
    const int ntiles = (S + 31) / 32;
    const int mine = ah_my_blocks<QB>(im.nblk, wave);

    char* sl = smem + G::RING_BYTES + wave * G::SLICE_BYTES;
    const AhFrag<G> fr(l15, lq);
    const ah_rsrc_t rsrcQ = ah_rsrc(qkv, im.off, qkv_bytes);
    auto dma_q = [&](int qi) { ah_q_dma<G>(rsrcQ, sl, 16 * (im.qb_lo + wave + 8 * qi), S, ld, lane); };
    f16x8 qf[QB][G::NKS];
#pragma unroll
    for (int qi = 0; qi < QB; ++qi) ah_q_zero<G>(qf[qi]);
    if (mine > 0) dma_q(0);                                             // block 0 travels with the ring fill below

    // ---- the K/V stream: past the end, harmless re-reads of the last tile
    const ah_rsrc_t rsrcK = ah_rsrc(qkv, im.off + d, qkv_bytes), rsrcV = ah_rsrc(qkv, im.off + 2 * d, qkv_bytes);
    int voff[G::PW];
    ah_piece_table<G, false>(voff, wave, lane, ld);
    int ld_kt = 0;
    auto issue = [&](int stage) {
        ah_issue<G>(rsrcK, rsrcV, smem + stage * G::STAGE_BYTES, voff, voff, false, (int)((long)ld_kt * 32 * ld * 2), wave);
        ld_kt = ld_kt + 1 < ntiles ? ld_kt + 1 : ntiles - 1;
    };

    f32x4 o[QB][G::NNB];
    float m_run[QB], l_run[QB];
#pragma unroll
    for (int qi = 0; qi < QB; ++qi) {
#pragma unroll
        for (int nb = 0; nb < G::NNB; ++nb) o[qi][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
        m_run[qi] = -INFINITY;
        l_run[qi] = 0.0f;
    }
    AhStamps<false> st;

#pragma unroll
    for (int s = 0; s < G::NST - 1; ++s) issue(s);
    wait_vm<0>();
    if (mine > 0) ah_q_read<G>(fr, sl, qf[0]);
    if (mine > 1) {                                                     // the slice is reused once block 0 is in registers
        __builtin_amdgcn_s_waitcnt(0xc07f);
        asm volatile("" ::: "memory");
        dma_q(1);
        wait_vm<0>();
        ah_q_read<G>(fr, sl, qf[1]);
    }
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    int stage = 0, wst = G::NST - 1;
    auto run_tiles = [&](auto nq_tag) {
        for (int kt = 0; kt < ntiles; ++kt) {
            const char* St = smem + stage * G::STAGE_BYTES;
            issue(wst);
            ah_tile<G, QB, decltype(nq_tag)::value>(fr, St, qf, kt, S, c_log2, m_run, l_run, o, st);
            ah_handover<G>(stage, wst);
        }
    };
    if (mine == 2) run_tiles(std::integral_constant<int, 2>{});
    else if (mine == 1) run_tiles(std::integral_constant<int, 1>{});
    else run_tiles(std::integral_constant<int, 0>{});
    wait_vm<0>();
    ah_store_rows<G, QB>(o, l_run, mine, sl, lane, ctx, im.b, im.h, im.qb_lo + wave, S, d);
#endif
}

// ---------------------------------------------------------------------------------------------------------------
// PERSISTENT form of the kernel above: one workgroup per CU walks the work items (sample, head, query chunk) w = block,
// block + G, ...  The kernel above keeps one workgroup per CU resident (128 KiB of LDS, 8 x 256 registers), so between two
// of them nothing overlaps: every item pays its ring fill (three 32-KiB tiles from L2), its Q loads and its output stores
// with the matrix pipe idle.  Here the K/V stream simply runs on into the next item's tiles while the current item's last
// tiles are being multiplied (the ring and its stage counters never restart), and the output stores of an item drain under
// the next item's first tiles.  The counted vmcnt waits stay valid with the extra Q loads / stores in the queue: memory
// operations retire in order, so "all but the youngest N" can only cover MORE than the tile it is meant to cover.  Per item
// the arithmetic is the kernel above's -- the same ah_tile in the same tile order on the same online-softmax state: bit-identical.
template <int HD, int QB, bool DBG>
__global__ __launch_bounds__(512, 1) void attentionh8p_kernel(const _Float16* __restrict__ qkv, _Float16* __restrict__ ctx,
                                                              int S, int H, int d, int nchunk, int nitems, float c_log2,
                                                              long qkv_bytes, unsigned long long* dbg) {
#if defined(__HIP_DEVICE_COMPILE__)
    using G = AhGeom2<HD>;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid) >> 6;
    const int l15 = lane & 15, lq = lane >> 4;
    const long ld = 3L * d;
    const int ntiles = (S + 31) / 32;
    const int NG = gridDim.x;
    const int lid = xcd_lid((int)blockIdx.x, NG);
    const int my_items = lid < nitems ? (nitems - lid + NG - 1) / NG : 0;
    if (my_items == 0) return;
    // item i of this workgroup -> element offset of its (sample, head) inside qkv
    auto item_off = [&](int i) -> long {                              // past the end: harmless re-reads of the last item
        return ah_item<false>(lid + (i < my_items ? i : my_items - 1) * NG, nchunk, H, S, ld, HD).off;
    };

    // ---- the K/V stream: tile ld_kt of stream item ld_it goes to ring stage wst; it runs NST - 1 tiles ahead of the MFMAs
    int voff[G::PW];
    ah_piece_table<G, false>(voff, wave, lane, ld);
    int ld_it = 0, ld_kt = 0;
    long st_off = item_off(0);
    auto issue = [&](int stage) {
        ah_issue<G>(ah_rsrc(qkv, st_off + d, qkv_bytes), ah_rsrc(qkv, st_off + 2 * d, qkv_bytes), smem + stage * G::STAGE_BYTES, voff,
                    voff, false, (int)((long)ld_kt * 32 * ld * 2), wave);
        if (++ld_kt == ntiles) {                                      // on into the next item's tiles
            ld_kt = 0;
            ++ld_it;
            st_off = item_off(ld_it);
        }
    };
    const AhFrag<G> fr(l15, lq);

    // Q fragments and output blocks travel as whole rows through the wave's 16-row slice of LDS (see ah_q_dma).  Item
    // i + 1's fragments are fetched at the END of item i, once its accumulators are packed to 16 bits, and IN FRONT of its output
    // stores: vector-memory operations retire in order, and nothing should have to wait for a store's acknowledgement.
    char* sl = smem + G::RING_BYTES + wave * G::SLICE_BYTES;
    f16x8 qf[QB][G::NKS];
    auto load_q = [&](int i) {
        const AhItem im = ah_item<true>(lid + i * NG, nchunk, H, S, ld, HD);
        const int mine = ah_my_blocks<QB>(im.nblk, wave);
        const ah_rsrc_t rsrcQ = ah_rsrc(qkv, im.off, qkv_bytes);
        int ln = lane;                                                  // laundered: per-lane address arithmetic derived from it stays
        asm volatile("" : "+v"(ln));                                    // here instead of being hoisted out of the item loop (and spilled)
        const AhFrag<G> frq(ln & 15, ln >> 4);
#pragma unroll
        for (int qi = 0; qi < QB; ++qi) {
            if (qi >= mine) {                                           // wave-uniform.  (Every fragment register is written on every
                ah_q_zero<G>(qf[qi]);                                   //  path: a conditionally kept one stays live through the
                continue;                                               //  epilogue, beside O and its packed copy: spills)
            }
            __builtin_amdgcn_s_waitcnt(0xc07f);                          // the slice's previous reads
            asm volatile("" ::: "memory");
            ah_q_dma<G>(rsrcQ, sl, 16 * (im.qb_lo + wave + 8 * qi), S, ld, ln);
            wait_vm<0>();
            ah_q_read<G>(frq, sl, qf[qi]);
        }
    };
#pragma unroll
    for (int qi = 0; qi < QB; ++qi) ah_q_zero<G>(qf[qi]);

#pragma unroll
    for (int s = 0; s < G::NST - 1; ++s) issue(s);
    load_q(0);
    wait_vm<0>();
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    int stage = 0, wst = G::NST - 1;
    AhStamps<DBG> st;                                                 // (waves 0 and 7 of workgroup 0 report)
    const unsigned long long tk0 = DBG ? __builtin_amdgcn_s_memtime() : 0, tr0 = DBG ? __builtin_amdgcn_s_memrealtime() : 0;

    for (int it = 0; it < my_items; ++it) {
        const AhItem im = ah_item<true>(lid + it * NG, nchunk, H, S, ld, HD);
        const int mine = ah_my_blocks<QB>(im.nblk, wave);

        f32x4 o[QB][G::NNB];
        float m_run[QB], l_run[QB];
#pragma unroll
        for (int qi = 0; qi < QB; ++qi) {
#pragma unroll
            for (int nb = 0; nb < G::NNB; ++nb) o[qi][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
            m_run[qi] = -INFINITY;
            l_run[qi] = 0.0f;
        }
        auto run_tiles = [&](auto nq_tag) {
            for (int kt = 0; kt < ntiles; ++kt) {
                const char* St = smem + stage * G::STAGE_BYTES;
                st.start();
                issue(wst);
                st.mark(st.d_is);
                ah_tile<G, QB, decltype(nq_tag)::value>(fr, St, qf, kt, S, c_log2, m_run, l_run, o, st);
                ah_handover<G>(stage, wst);
                st.mark(st.d_bar);
                if constexpr (DBG) ++st.n_t;
            }
        };
        if (mine == 2) run_tiles(std::integral_constant<int, 2>{});
        else if (mine == 1) run_tiles(std::integral_constant<int, 1>{});
        else run_tiles(std::integral_constant<int, 0>{});
        // the next item's fragments go into the registers of this item's (dead after the last tile), while the accumulators are
        // still where the MFMAs left them
        asm volatile("" ::: "memory");
        if (it + 1 < my_items) {
            load_q(it + 1);                                               // in front of the stores
        } else {
#pragma unroll
            for (int qi = 0; qi < QB; ++qi) ah_q_zero<G>(qf[qi]);
        }
        asm volatile("" ::: "memory");
        int ln = lane;
        asm volatile("" : "+v"(ln));                                      // (as in load_q)
        ah_store_rows<G, QB>(o, l_run, mine, sl, ln, ctx, im.b, im.h, im.qb_lo + wave, S, d);
    }
    if (DBG && dbg && blockIdx.x == 0 && lane == 0 && (wave == 0 || wave == 7)) {
        unsigned long long* o = dbg + (wave == 0 ? 0 : 8);
        o[0] = st.d_is; o[1] = st.d_qk; o[2] = st.d_sm; o[3] = st.d_pv; o[4] = st.d_bar; o[5] = st.n_t;
        o[6] = __builtin_amdgcn_s_memtime() - tk0; o[7] = __builtin_amdgcn_s_memrealtime() - tr0;
    }
    wait_vm<0>();
#endif
}

// ---- host -------------------------------------------------------------------------------------------------------
// kernel: 1 = attentionh8_kernel, 2 = attentionh8q_kernel, 3 = attentionh8p_kernel
// The query chunks (8 blocks of 16 per workgroup pass for kernel 1, 16 for 2 / 3), work items and workgroups of a kernel choice.
// grid: the persistent form's workgroups, 0 = one per CU and at most one per item.
struct AhPlan {
    int nchunk;
    long items;
    int grid;
};
static AhPlan ah_plan(int kernel, int B, int S, int H, int grid, int num_cus) {
    const int nqb = (S + 15) / 16;
    AhPlan p;
    p.nchunk = kernel == 1 ? (nqb + 7) / 8 : (nqb + 15) / 16;
    p.items = (long)B * H * p.nchunk;
    p.grid = kernel != 3 ? (int)p.items : grid != 0 ? grid : p.items < num_cus ? (int)p.items : num_cus;
    return p;
}

// head widths with an 8 x 2 and a persistent instantiation
constexpr bool ah_multiblock(int hd) { return hd == 64 || hd == 128 || hd == 256; }

template <int KERNEL, int HD>
static hipError_t launch_ah(const _Float16* qkv, _Float16* ctx, int S, int H, int d, long qkv_bytes, const AhPlan& p, hipStream_t s,
                            unsigned long long* stamps) {
    using G = std::conditional_t<KERNEL == 1, AhGeom1<HD>, AhGeom2<HD>>;
    constexpr size_t lds = G::LDS_BYTES;
    static bool attr_done = false;
    if (!attr_done) {
        auto raise = [&](auto* k) {
            return hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        };
        hipError_t e;
        if constexpr (KERNEL == 1) e = raise(&attentionh8_kernel<HD>);
        else if constexpr (KERNEL == 2) e = raise(&attentionh8q_kernel<HD, 2>);
        else {
            e = raise(&attentionh8p_kernel<HD, 2, false>);
            if (e == hipSuccess) e = raise(&attentionh8p_kernel<HD, 2, true>);
        }
        if (e != hipSuccess) return e;
        attr_done = true;
    }
    const float c_log2 = 1.4426950408889634f / sqrtf((float)HD);
    if constexpr (KERNEL == 1)
        hipLaunchKernelGGL((attentionh8_kernel<HD>), dim3(p.grid), dim3(512), lds, s, qkv, ctx, S, H, d, p.nchunk, c_log2, qkv_bytes);
    else if constexpr (KERNEL == 2)
        hipLaunchKernelGGL((attentionh8q_kernel<HD, 2>), dim3(p.grid), dim3(512), lds, s, qkv, ctx, S, H, d, p.nchunk, c_log2, qkv_bytes);
    else if (stamps)                                              // the stamped build of the kernel (diagnostic launches only)
        hipLaunchKernelGGL((attentionh8p_kernel<HD, 2, true>), dim3(p.grid), dim3(512), lds, s, qkv, ctx, S, H, d, p.nchunk,
                           (int)p.items, c_log2, qkv_bytes, stamps);
    else
        hipLaunchKernelGGL((attentionh8p_kernel<HD, 2, false>), dim3(p.grid), dim3(512), lds, s, qkv, ctx, S, H, d, p.nchunk,
                           (int)p.items, c_log2, qkv_bytes, stamps);
    return hipGetLastError();
}

template <int HD>
static hipError_t launch_ah_kernel(int kernel, const _Float16* qkv, _Float16* ctx, int S, int H, int d, long qkv_bytes, const AhPlan& p,
                                   hipStream_t s, unsigned long long* stamps) {
    if constexpr (ah_multiblock(HD)) {
        if (kernel == 3) return launch_ah<3, HD>(qkv, ctx, S, H, d, qkv_bytes, p, s, stamps);
        if (kernel == 2) return launch_ah<2, HD>(qkv, ctx, S, H, d, qkv_bytes, p, s, stamps);
    }
    return kernel == 1 ? launch_ah<1, HD>(qkv, ctx, S, H, d, qkv_bytes, p, s, stamps) : hipErrorInvalidValue;
}

bool attentionh_supported(int S, int H, int d) {
    const int hd = d / H;
    return head_dim_supported(hd) && d % 8 == 0 && S >= 1;
}

bool attentionh_multiblock(int hd) { return ah_multiblock(hd); }

// The one dispatch of the forward and of the test entry point gdx_attention_half.  kernel: 0 = the forward's choice, 1 = the
// 8-wave x 1-block kernel, 2 = 8 x 2 blocks, 3 = the persistent form (the callers refuse 2 / 3 at head_dim 32, 96 and 192, which
// have no instantiation of them: attentionh_multiblock); grid > 0: workgroups of the persistent form (0 = one per CU, at most one per item).  launched
// (optional, 3 entries): the kernel that ran (1-3), its grid and its work-item count.  qkv_rows: rows of the qkv buffer that are
// readable (>= B*S); reads past them return zeros.  stamps (optional): the persistent form runs its stamped build and writes there.
hipError_t launch_attentionh_kernel(const _Float16* qkv, _Float16* ctx, int B, int S, int H, int d, long qkv_rows, int kernel,
                                    int grid, int* launched, hipStream_t s, unsigned long long* stamps) {
    const int hd = d / H;
    const long bytes = qkv_rows * 3L * d * 2;
    // measured (tools/attnh_one.py, us): B=128 S=521 hd=256: 8 waves x 1 block 373, 8 waves x 2 blocks 292, persistent 273-285;
    // B=16 (config 5's per-GPU share): 58.9 / 37.4;  B=64 S=197 hd=128: 19.9 / 18.7.  The 8 x 2 kernels need enough
    // workgroups to fill the chip (they make half as many), so small problems keep one block per wave.
    // (Round 3, XCD-aware items + whole-row Q / output traffic: persistent 257-261, B=16 33.0, B=256 S=197 hd=128 55.7.)
    const int num_cus = gemm2_num_cus();
    if (kernel == 0) {
        const long nitems = ah_plan(2, B, S, H, 0, num_cus).items;
        // persistent form once every CU has at least two items to chain (profiles/r02h_*)
        if (ah_multiblock(hd) && nitems >= 2L * num_cus) kernel = 3;
        else if (ah_multiblock(hd) && nitems >= 128) kernel = 2;
        else kernel = 1;
    }
    if ((kernel != 1 && (!ah_multiblock(hd) || kernel > 3)) || kernel < 1 || (grid != 0 && kernel != 3) || grid < 0) return hipErrorInvalidValue;
    const AhPlan p = ah_plan(kernel, B, S, H, grid, num_cus);
    if (launched) {
        launched[0] = kernel;
        launched[1] = p.grid;
        launched[2] = (int)p.items;
    }
    switch (hd) {
    case 256: return launch_ah_kernel<256>(kernel, qkv, ctx, S, H, d, bytes, p, s, stamps);
    case 192: return launch_ah_kernel<192>(kernel, qkv, ctx, S, H, d, bytes, p, s, stamps);
    case 128: return launch_ah_kernel<128>(kernel, qkv, ctx, S, H, d, bytes, p, s, stamps);
    case 96: return launch_ah_kernel<96>(kernel, qkv, ctx, S, H, d, bytes, p, s, stamps);
    case 64: return launch_ah_kernel<64>(kernel, qkv, ctx, S, H, d, bytes, p, s, stamps);
    case 32: return launch_ah_kernel<32>(kernel, qkv, ctx, S, H, d, bytes, p, s, stamps);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_attentionh(const _Float16* qkv, _Float16* ctx, int B, int S, int H, int d, long qkv_rows, hipStream_t s) {
    return launch_attentionh_kernel(qkv, ctx, B, S, H, d, qkv_rows, 0, 0, nullptr, s);
}

GDX_HNS_END
}  // namespace gdx
