// The weights of a model handle: which tensors the configuration has (describe_weights), how a state-dict tensor becomes its
// zero-padded device buffers (gdx_set_weight), and the packed image of all of them (gdx_export_packed / gdx_import_packed).
#include "gdx_host.h"

#include <cstring>

namespace gdx {

// dst[r][c] = (r < n && c < k) ? src[r*src_ld + col0 + c] : 0      (dst is [npad][kpad])
__global__ void pack_weight_kernel(const float* __restrict__ src, int src_ld, int col0, int n, int k,
                                   float* __restrict__ dst, int npad, int kpad) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)npad * kpad) return;
    const int r = i / kpad, c = i % kpad;
    dst[i] = (r < n && c < k) ? src[(long)r * src_ld + col0 + c] : 0.0f;
}

// dst[r][c] = (r < n && c < k) ? (fp16) src[r*src_ld + col0 + c] : 0      (dst is [npad][kpad] halves)
__global__ void pack_weight_f16_kernel(const float* __restrict__ src, int src_ld, int col0, int n, int k,
                                       _Float16* __restrict__ dst, int npad, int kpad) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)npad * kpad) return;
    const int r = i / kpad, c = i % kpad;
    dst[i] = (r < n && c < k) ? (_Float16)src[(long)r * src_ld + col0 + c] : (_Float16)0.0f;
}

// the same with bf16 elements (GDX_DTYPE_BF16); the destination is passed as an opaque 16-bit pointer like every half buffer
__global__ void pack_weight_bf16_kernel(const float* __restrict__ src, int src_ld, int col0, int n, int k,
                                        _Float16* __restrict__ dst_, int npad, int kpad) {
    __bf16* dst = reinterpret_cast<__bf16*>(dst_);
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)npad * kpad) return;
    const int r = i / kpad, c = i % kpad;
    dst[i] = (r < n && c < k) ? (__bf16)src[(long)r * src_ld + col0 + c] : (__bf16)0.0f;
}

int pack_f16_into(_Float16* dst, const float* src, int n, int src_ld, int col0, int k, int npad, int kpad, hipStream_t s, bool bf) {
    const long total = (long)npad * kpad;
    hipLaunchKernelGGL(bf ? pack_weight_bf16_kernel : pack_weight_f16_kernel, dim3((total + 255) / 256), dim3(256), 0, s, src,
                       src_ld, col0, n, k, dst, npad, kpad);
    HIPCHK(hipGetLastError());
    return 0;
}

// P (dims from describe_weights) = columns [col0, col0 + P.k) of the [P.n][src_ld] tensor src
static int pack(gdx_model* h, Packed& P, const float* src, int src_ld, int col0, hipStream_t s) {
    if (!P.w && dev_alloc(h->allocs, (void**)&P.w, sizeof(float) * P.npad * (size_t)P.kpad)) return -1;
    const long total = (long)P.npad * P.kpad;
    hipLaunchKernelGGL(pack_weight_kernel, dim3((total + 255) / 256), dim3(256), 0, s, src, src_ld, col0, P.n, P.k, P.w,
                       P.npad, P.kpad);
    HIPCHK(hipGetLastError());
    if (h->f16) {
        if (!P.w16 && dev_alloc(h->allocs, (void**)&P.w16, 2 * (size_t)P.npad16 * P.kpad16)) return -1;
        if (pack_f16_into(P.w16, src, P.n, src_ld, col0, P.k, P.npad16, P.kpad16, s, h->bf16)) return -1;
    }
    return 0;
}

static int pack_vec(gdx_model* h, float** dst, const float* src, long n, long npad, hipStream_t s) {
    if (!*dst && dev_alloc(h->allocs, (void**)dst, sizeof(float) * npad)) return -1;
    HIPCHK(hipMemsetAsync(*dst, 0, sizeof(float) * npad, s));
    HIPCHK(hipMemcpyAsync(*dst, src, sizeof(float) * n, hipMemcpyDeviceToDevice, s));
    return 0;
}

// The padding rule of a packed Linear weight: the fp32 GEMMs read whole 128 x 32 panels of it (gdx_internal.h), the 16-bit
// GEMM 256 x 64 ones (gemmh.hip)
static void padded_dims(Packed& P, int n, int k, bool f16) {
    P.n = n; P.k = k; P.npad = round_up(n, 128); P.kpad = round_up(k, 32);
    P.npad16 = f16 ? round_up(n, 256) : 0; P.kpad16 = f16 ? round_up(k, 64) : 0;
}

void describe_weights(gdx_model* h) {
    const int d = h->d, J = h->J, ff = h->ff, mf = h->cfg.mfcc_dim;
    const bool v2 = h->cfg.arch == GDX_ARCH_MDM;
    auto& t = h->weights;
    int group = 0;
    // a Linear [n][cols]: `weight` becomes one panel per {P, first column, columns}, `bias` goes with the first
    struct Cut { Packed* P; int col0, k; };
    auto linear = [&](const std::string& weight, const std::string& bias, int n, int cols, std::initializer_list<Cut> cuts) {
        WeightSpec w{WeightSpec::LINEAR, weight, {n, cols}};
        for (const Cut& c : cuts) {
            padded_dims(*c.P, n, c.k, h->f16);
            w.slices.push_back({c.P, c.col0});
        }
        w.group = group;
        t.push_back(w);
        WeightSpec b{WeightSpec::BIAS, bias, {n}};
        b.P = cuts.begin()->P;
        b.P->has_bias = true;
        b.group = group;
        t.push_back(b);
    };
    auto buffer = [&](WeightSpec::Kind kind, const std::string& key, std::vector<int64_t> shape, float** dst, bool rotary = false) {
        WeightSpec v{kind, key, shape};
        v.vec = dst; v.rotary = rotary;
        v.group = group;
        t.push_back(v);
    };
    // in the order of the packed image; `group` is the order of the "missing weights" report: the base model, its positional
    // table, what GDX_ARCH_MDM adds, the layers
    const std::string te = "embed_timestep.time_embed.", in = "input_process.poseEmbedding.";
    linear(te + "0.weight", te + "0.bias", d, d, {{&h->time0, 0, d}});
    linear(te + "2.weight", te + "2.bias", d, d, {{&h->time2, 0, d}});
    // use_text (model/mdm.py:36-50): embed_text fills the first text_dim columns of the coarse condition, the seed encoder the rest
    const int td = h->cfg.text_dim;
    linear("seed_pose_encoder.seed_embed.weight", "seed_pose_encoder.seed_embed.bias", d - td, J * h->cfg.seed_poses,
           {{&h->seed, 0, J * h->cfg.seed_poses}});
    if (td > 0) {
        group = 2;
        linear("embed_text.weight", "embed_text.bias", td, h->cfg.clip_dim, {{&h->text, 0, h->cfg.clip_dim}});
        group = 0;
    }
    if (v2) {
        linear(in + "weight", in + "bias", d, J, {{&h->in_x, 0, J}});
        group = 2;   // project_to_lat reads [pose embedding | mfcc | timestep + seed embedding]
        linear("project_to_lat.weight", "project_to_lat.bias", d, 2 * d + mf,
               {{&h->proj_pose, 0, d}, {&h->proj_audio, d, mf}, {&h->proj_coa, d + mf, d}});
        group = 0;
    } else {
        linear(in + "weight", in + "bias", d, J + mf, {{&h->in_x, 0, J}, {&h->in_mfcc, J, mf}});   // [pose | mfcc]
    }
    linear("output_process.poseFinal.weight", "output_process.poseFinal.bias", J, d, {{&h->outp, 0, d}});
    group = 3;
    for (int l = 0; l < h->L; ++l) {
        Layer& ly = h->layers[l];
        const std::string p = "seqTransEncoder.layers." + std::to_string(l) + ".";
        linear(p + "self_attn.in_proj_weight", p + "self_attn.in_proj_bias", 3 * d, d, {{&ly.qkv, 0, d}});
        linear(p + "self_attn.out_proj.weight", p + "self_attn.out_proj.bias", d, d, {{&ly.out, 0, d}});
        linear(p + "linear1.weight", p + "linear1.bias", ff, d, {{&ly.ff1, 0, d}});
        linear(p + "linear2.weight", p + "linear2.bias", d, ff, {{&ly.ff2, 0, ff}});
        buffer(WeightSpec::VECTOR, p + "norm1.weight", {d}, &ly.g1);
        buffer(WeightSpec::VECTOR, p + "norm1.bias", {d}, &ly.b1);
        buffer(WeightSpec::VECTOR, p + "norm2.weight", {d}, &ly.g2);
        buffer(WeightSpec::VECTOR, p + "norm2.bias", {d}, &ly.b2);
    }
    group = 1;
    buffer(WeightSpec::TABLE, "sequence_pos_encoder.pe", {0, 1, d}, &h->pe);
    if (v2) {
        group = 2;
        buffer(WeightSpec::TABLE, "rope.cos", {0, d / h->cfg.cl_head / 2}, &h->rope_cos, true);
        buffer(WeightSpec::TABLE, "rope.sin", {0, d / h->cfg.cl_head / 2}, &h->rope_sin, true);
    }
    for (int g = 0; g <= 3; ++g)
        for (const WeightSpec& w : t)
            if (w.group == g) h->required.push_back(w.key);
}

// whatever depends on the weights (the conditioning terms, the loops' timestep tables) has to be rebuilt
static void weights_changed(gdx_model* h) {
    h->cond_set = false;
    h->late.c2t_valid = false;
    h->late.tables_valid = false;
}

}  // namespace gdx

using namespace gdx;

extern "C" int gdx_set_weight(gdx_handle_t h, const char* name_c, const float* p, const int64_t* shape, int32_t ndim,
                              void* stream) {
    if (!h || !name_c || !p || !shape) return fail("gdx_set_weight: null argument");
    hipStream_t s = (hipStream_t)stream;
    const std::string name(name_c);
    const WeightSpec* w = nullptr;
    for (const WeightSpec& c : h->weights)
        if (c.key == name) w = &c;
    if (!w) return fail("gdx_set_weight: unexpected key " + name);   // load_model_wo_clip asserts no unexpected keys
    const bool tab = w->kind == WeightSpec::TABLE;
    bool fits = ndim == (int)w->shape.size();
    for (int i = tab ? 1 : 0; fits && i < ndim; ++i) fits = shape[i] == w->shape[i];
    if (!fits) return fail("gdx_set_weight: unexpected shape for " + name);
    int rc = 0;
    long count = 1;
    for (int i = 0; i < ndim; ++i) count *= shape[i];
    switch (w->kind) {
    case WeightSpec::LINEAR:
        for (const WeightSlice& sl : w->slices)
            if (!rc) rc = pack(h, *sl.P, p, (int)shape[1], sl.col0, s);
        break;
    case WeightSpec::BIAS:
        rc = pack_vec(h, &w->P->bias, p, count, w->P->npad, s);
        break;
    case WeightSpec::VECTOR:
        rc = pack_vec(h, w->vec, p, count, count, s);
        break;
    case WeightSpec::TABLE:
        // a fresh buffer on every call (the size may have changed); the old one stays in the pool until gdx_destroy
        (w->rotary ? h->rope_rows : h->pe_rows) = (int)shape[0];
        *w->vec = nullptr;
        rc = pack_vec(h, w->vec, p, count, count, s);
        break;
    }
    if (rc) return rc;
    h->have.insert(name);
    weights_changed(h);
    return 0;
}

extern "C" int gdx_weights_ready(gdx_handle_t h) {
    if (!h) return fail("gdx_weights_ready: null handle");
    std::string missing;
    for (const auto& n : h->required)
        if (!h->have.count(n)) missing += (missing.empty() ? "" : ", ") + n;
    if (!missing.empty()) return fail("missing weights: " + missing);
    return 0;
}

// ---- packed-weight image (the weight pre-packing cache) ----------------------------------------------
// Everything gdx_set_weight builds -- the zero-padded K-contiguous fp32 panels, their fp16 twins in the fp16 mode, padded
// bias vectors, LayerNorm vectors, the positional / rotary tables -- as ONE host blob: a header (magic, the gdx_config_t
// it was built for, record count) and one {id, dims, byte count, bytes} record per device buffer in a fixed walk order.
// A blob only loads into a handle created with the same configuration; its records are checked against the sizes the
// handle computes itself, so a stale or foreign file is rejected instead of producing a wrong model.  The magic stays
// "GDXPACK3" although gdx_config_t grew by text_dim / clip_dim: an image with the shorter header has its (positive) record
// count where text_dim is read and half its checksum where clip_dim is, so the configuration compare refuses it (always for a
// handle without text; a text handle whose two fields happened to match still fails the record and checksum checks behind).
namespace {
struct PackRec { int32_t id, n, k, npad, kpad, npad16, kpad16, pad; int64_t bytes; };
struct PackHdr { char magic[8]; gdx_config_t cfg; int32_t nrec, pad; };
const char PACK_MAGIC[8] = {'G', 'D', 'X', 'P', 'A', 'C', 'K', '3'};
// 64-bit FNV-1a over the 8-byte words of the payload (records + buffers; everything behind the extras block, whose length is a
// multiple of 8): the image's integrity check.  It lives in PackHdr::pad (low half) and the fourth extras word (high half).
static uint64_t pack_hash(const char* p, const char* end) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (; p + 8 <= end; p += 8) {
        uint64_t w;
        memcpy(&w, p, 8);
        h = (h ^ w) * 0x100000001b3ull;
    }
    for (; p < end; ++p) h = (h ^ (unsigned char)*p) * 0x100000001b3ull;
    return h;
}
struct PackBuf { void** ptr; size_t bytes; PackRec rec; };
const size_t PACK_PAYLOAD_AT = sizeof(PackHdr) + 4 * sizeof(int32_t);   // header + extras {pe_rows, rope_rows, dtype, hash high}
static size_t padded16(size_t bytes) { return (bytes + 15) / 16 * 16; }   // a buffer's bytes in the image
}  // namespace

// the walk: every device weight buffer of the table with the size it has (export) or must have (import), the positional /
// rotary tables at the given row counts.  Per Packed: w, bias, w16, with zero-byte records where it has none.
static std::vector<PackBuf> pack_walk(const std::vector<WeightSpec>& table, int pe_rows, int rope_rows) {
    std::vector<PackBuf> out;
    int id = 0;
    auto vec = [&](float** p, long n) {
        PackRec r{};
        r.id = id++; r.n = (int32_t)n; r.bytes = (int64_t)sizeof(float) * n;
        out.push_back({(void**)p, (size_t)r.bytes, r});
    };
    for (const WeightSpec& w : table) {
        for (const WeightSlice& sl : w.slices) {
            Packed& P = *sl.P;
            PackRec r{};
            r.n = P.n; r.k = P.k; r.npad = P.npad; r.kpad = P.kpad; r.npad16 = P.npad16; r.kpad16 = P.kpad16;
            r.id = id++; r.bytes = (int64_t)sizeof(float) * P.npad * P.kpad;
            out.push_back({(void**)&P.w, (size_t)r.bytes, r});
            r.id = id++; r.bytes = P.has_bias ? (int64_t)sizeof(float) * P.npad : 0;
            out.push_back({(void**)&P.bias, (size_t)r.bytes, r});
            r.id = id++; r.bytes = (int64_t)2 * P.npad16 * P.kpad16;
            out.push_back({(void**)&P.w16, (size_t)r.bytes, r});
        }
        if (w.kind == WeightSpec::VECTOR) vec(w.vec, w.shape[0]);
        if (w.kind == WeightSpec::TABLE) {
            long n = w.rotary ? rope_rows : pe_rows;
            for (size_t i = 1; i < w.shape.size(); ++i) n *= w.shape[i];
            vec(w.vec, n);
        }
    }
    return out;
}

extern "C" int gdx_packed_bytes(gdx_handle_t h, int64_t* bytes) {
    if (!h || !bytes) return fail("gdx_packed_bytes: null argument");
    if (gdx_weights_ready(h)) return -1;
    int64_t total = PACK_PAYLOAD_AT;
    for (const PackBuf& b : pack_walk(h->weights, h->pe_rows, h->rope_rows)) total += sizeof(PackRec) + (int64_t)padded16(b.bytes);
    *bytes = total;
    return 0;
}

extern "C" int gdx_export_packed(gdx_handle_t h, void* host, int64_t bytes, void* stream) {
    if (!h || !host) return fail("gdx_export_packed: null argument");
    int64_t need = 0;
    if (gdx_packed_bytes(h, &need)) return -1;
    if (bytes != need) return fail("gdx_export_packed: buffer size does not match gdx_packed_bytes");
    hipStream_t s = (hipStream_t)stream;
    const std::vector<PackBuf> bufs = pack_walk(h->weights, h->pe_rows, h->rope_rows);
    PackHdr hd{};
    memcpy(hd.magic, PACK_MAGIC, 8);
    hd.cfg = h->cfg; hd.nrec = (int32_t)bufs.size();
    int32_t extra[4] = {h->pe_rows, h->rope_rows, h->cfg.compute_dtype, 0};
    char* const payload = (char*)host + PACK_PAYLOAD_AT;
    char* p = payload;
    memset(payload, 0, (size_t)bytes - PACK_PAYLOAD_AT);            // the 16-byte alignment gaps are part of the hashed payload
    for (const PackBuf& b : bufs) {
        memcpy(p, &b.rec, sizeof(PackRec)); p += sizeof(PackRec);
        if (b.bytes) {
            if (!*b.ptr) return fail("gdx_export_packed: a weight buffer is missing");
            HIPCHK(hipMemcpyAsync(p, *b.ptr, b.bytes, hipMemcpyDeviceToHost, s));
        }
        p += padded16(b.bytes);
    }
    HIPCHK(hipStreamSynchronize(s));
    const uint64_t hash = pack_hash(payload, (char*)host + bytes);
    hd.pad = (int32_t)(uint32_t)hash;
    extra[3] = (int32_t)(uint32_t)(hash >> 32);
    memcpy(host, &hd, sizeof(hd));
    memcpy((char*)host + sizeof(hd), extra, sizeof(extra));
    return 0;
}

// Is the blob a whole, uncorrupted image of a model with this configuration (whose weights `table` describes)?  Touches
// neither the GPU nor the handle: `why` is the refusal, or nullptr with the row counts of the image's tables.
struct ImageCheck { const char* why; int pe_rows, rope_rows; };
static ImageCheck check_image(const void* host, int64_t bytes, const gdx_config_t& cfg, const std::vector<WeightSpec>& table) {
    if (bytes < (int64_t)PACK_PAYLOAD_AT) return {"gdx_import_packed: blob too small", 0, 0};
    const char* p = (const char*)host;
    const char* end = p + bytes;
    PackHdr hd;
    memcpy(&hd, p, sizeof(hd)); p += sizeof(hd);
    if (memcmp(hd.magic, PACK_MAGIC, 8)) return {"gdx_import_packed: not a packed-weight image (bad magic)", 0, 0};
    if (memcmp(&hd.cfg, &cfg, sizeof(gdx_config_t))) return {"gdx_import_packed: image was built for another configuration", 0, 0};
    int32_t extra[4];
    memcpy(extra, p, sizeof(extra)); p += sizeof(extra);
    const uint64_t stored = (uint64_t)(uint32_t)hd.pad | ((uint64_t)(uint32_t)extra[3] << 32);
    if (extra[2] != cfg.compute_dtype) return {"gdx_import_packed: image was built for another compute dtype", 0, 0};
    const int rope_need = cfg.arch == GDX_ARCH_MDM ? 1 : 0;
    if (extra[0] <= 0 || extra[0] > (1 << 20) || extra[1] < rope_need || extra[1] > (1 << 20))
        return {"gdx_import_packed: implausible table sizes", 0, 0};
    const std::vector<PackBuf> bufs = pack_walk(table, extra[0], extra[1]);
    if (hd.nrec != (int32_t)bufs.size()) return {"gdx_import_packed: record count mismatch", 0, 0};
    const char* q = p;
    for (const PackBuf& b : bufs) {
        if (q + sizeof(PackRec) > end) return {"gdx_import_packed: truncated image", 0, 0};
        if (memcmp(q, &b.rec, sizeof(PackRec))) return {"gdx_import_packed: record does not match this configuration", 0, 0};
        q += sizeof(PackRec) + padded16(b.bytes);
        if (q > end) return {"gdx_import_packed: truncated image", 0, 0};
    }
    if (q != end) return {"gdx_import_packed: trailing bytes", 0, 0};
    if (pack_hash(p, end) != stored) return {"gdx_import_packed: payload checksum mismatch (corrupted image)", 0, 0};
    return {nullptr, extra[0], extra[1]};
}

extern "C" int gdx_import_packed(gdx_handle_t h, const void* host, int64_t bytes, void* stream) {
    if (!h || !host) return fail("gdx_import_packed: null argument");
    const ImageCheck img = check_image(host, bytes, h->cfg, h->weights);   // the whole blob, before touching the handle
    if (img.why) return fail(img.why);
    // the tables may change size with the image: let them be re-allocated
    if (img.pe_rows != h->pe_rows) h->pe = nullptr;
    if (img.rope_rows != h->rope_rows) { h->rope_cos = nullptr; h->rope_sin = nullptr; }
    h->pe_rows = img.pe_rows; h->rope_rows = img.rope_rows;
    hipStream_t s = (hipStream_t)stream;
    // from here on the handle's weights are being overwritten: it is "not ready" until the last byte has arrived (a failed
    // allocation or copy must not leave a half-uploaded model that gdx_weights_ready accepts)
    h->have.clear();
    weights_changed(h);
    const char* p = (const char*)host + PACK_PAYLOAD_AT;
    for (const PackBuf& b : pack_walk(h->weights, h->pe_rows, h->rope_rows)) {
        p += sizeof(PackRec);
        if (b.bytes) {
            if (!*b.ptr && dev_alloc(h->allocs, b.ptr, b.bytes)) return -1;
            HIPCHK(hipMemcpyAsync(*b.ptr, p, b.bytes, hipMemcpyHostToDevice, s));
        }
        p += padded16(b.bytes);
    }
    HIPCHK(hipStreamSynchronize(s));                             // the caller may free the host blob on return
    h->have.insert(h->required.begin(), h->required.end());
    return 0;
}
