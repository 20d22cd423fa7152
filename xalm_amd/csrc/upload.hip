// upload.hip — weights and KV rows onto the device: the device layout of each tensor, host,
// file and synthetic uploads, the fp8 special-code scan (xh_upload*, xh_kv_*).
#include <hip/hip_runtime.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstring>
#include <thread>
#include <vector>

#include "../../include/xalm_synth.h"
#include "ctx.h"

using namespace xalm;

namespace {

// Destination of one logical tensor [rows][cols] inside the device layout: the buffer
// (allocated on first use), the byte offset of row 0 and the byte pitch between rows.
struct Slot {
    char* base = nullptr;
    size_t pitch = 0;
    size_t rows = 0, cols = 0;
};

int tensor_slot(xh_ctx* ctx, int kind, int layer, int dtype, Slot* out) {
    const xh_config& c = ctx->c;
    const bool per_layer = !(kind == XH_EMBED || kind == XH_FINAL_NORM || kind == XH_WCLS);
    if (per_layer && (layer < 0 || layer >= c.n_layers))
        return set_err(ctx, XH_E_INVALID, "layer %d out of range", layer);
    size_t rows = 0, cols = 0;
    bool is_norm = false;
    switch (kind) {
        case XH_EMBED: case XH_WCLS: rows = c.vocab_size; cols = c.dim; break;
        case XH_ATTN_NORM: case XH_FFN_NORM: case XH_FINAL_NORM: rows = 1; cols = c.dim; is_norm = true; break;
        case XH_WQ: rows = ctx->q_dim; cols = c.dim; break;
        case XH_WK: case XH_WV: rows = ctx->kv_dim; cols = c.dim; break;
        case XH_WO: rows = c.dim; cols = ctx->q_dim; break;
        case XH_W1: case XH_W3: rows = c.hidden_dim; cols = c.dim; break;
        case XH_W2: rows = c.dim; cols = c.hidden_dim; break;
        default: return set_err(ctx, XH_E_INVALID, "unknown tensor kind %d", kind);
    }
    if (is_norm ? !(dtype == XH_F32 || dtype == XH_BF16) : !matrix_dtype_ok(dtype))
        return set_err(ctx, XH_E_INVALID, "tensor kind %d: unsupported dtype %d", kind, dtype);
    if (gq_dt(dtype) && cols % gq_group(dtype))
        return set_err(ctx, XH_E_INVALID, "tensor kind %d: %zu columns, not whole %d-element blocks", kind, cols, gq_group(dtype));
    // a matvec input: its x image must fit the CU's LDS (the embedding is one only when tied)
    if (!is_norm && (kind != XH_EMBED || c.tie_word_embeddings) && matrix_lds_bytes(dtype, (int)cols) > GEMV_LDS_MAX)
        return set_err(ctx, XH_E_INVALID, "tensor kind %d: the %zu-element input of dtype %d needs %zu bytes of LDS, over %zu",
                       kind, cols, dtype, matrix_lds_bytes(dtype, (int)cols), GEMV_LDS_MAX);
    const size_t rb = dev_row_bytes(dtype, cols);
    out->rows = rows;
    out->cols = cols;
    out->pitch = rb;
    drop_graphs(ctx);
    auto plain = [&](void** dst, int* dst_dt, bool* special = nullptr, uint8_t* er = nullptr) -> int {
        if (special) *special = false;  // a whole-buffer upload: rescanned after the copy
        if (er) { er[0] = 255; er[1] = 0; }
        if (*dst && *dst_dt != dtype) {
            if (*dst == ctx->wcls && *dst != ctx->embed) ctx->wcls = nullptr;
            hipFree(*dst);
            *dst = nullptr;
        }
        if (!*dst) HIP_TRY(ctx, hipMalloc(dst, rows * rb));
        *dst_dt = dtype;
        out->base = (char*)*dst;
        return 0;
    };
    if (kind == XH_EMBED) {
        const bool alias = ctx->wcls != nullptr && ctx->wcls == ctx->embed;
        if (alias) ctx->wcls = nullptr;
        int rc = plain(&ctx->embed, &ctx->embed_dt);
        if (alias) { ctx->wcls = ctx->embed; ctx->wcls_dt = ctx->embed_dt; }
        return rc;
    }
    if (kind == XH_FINAL_NORM) return plain(&ctx->final_norm, &ctx->final_norm_dt);
    if (kind == XH_WCLS) {
        if (ctx->wcls == ctx->embed) ctx->wcls = nullptr;
        return plain(&ctx->wcls, &ctx->wcls_dt, &ctx->wcls_x, ctx->wcls_e);
    }
    LayerW& w = ctx->L[layer];
    switch (kind) {
        case XH_ATTN_NORM: return plain(&w.attn_norm, &w.an_dt);
        case XH_FFN_NORM: return plain(&w.ffn_norm, &w.fn_dt);
        case XH_WO: return plain(&w.wo, &w.wo_dt, &w.wo_x, w.wo_e);
        case XH_W2: return plain(&w.w2, &w.w2_dt, &w.w2_x, w.w2_e);
        case XH_WQ: case XH_WK: case XH_WV: {
            // fused [Wq; Wk; Wv] rows, one dtype
            if (w.wqkv && w.qkv_dt != dtype) {
                if (w.qkv_have & ~(1u << (kind - XH_WQ)))
                    return set_err(ctx, XH_E_INVALID, "layer %d: q/k/v must share one dtype", layer);
                hipFree(w.wqkv); w.wqkv = nullptr; w.qkv_have = 0;
            }
            if (!(w.qkv_have & ~(1u << (kind - XH_WQ)))) {  // no other part holds codes
                w.qkv_x = false;
                w.qkv_e[0] = 255; w.qkv_e[1] = 0;
            }
            if (!w.wqkv) HIP_TRY(ctx, hipMalloc(&w.wqkv, (size_t)(ctx->q_dim + 2 * ctx->kv_dim) * rb));
            w.qkv_dt = dtype;
            const size_t row0 = kind == XH_WQ ? 0 : kind == XH_WK ? ctx->q_dim : ctx->q_dim + ctx->kv_dim;
            out->base = (char*)w.wqkv + row0 * rb;
            w.qkv_have |= 1u << (kind - XH_WQ);
            return 0;
        }
        case XH_W1: case XH_W3: {
            // fused gate/up, rows interleaved: row 2i = W1[i], row 2i+1 = W3[i]
            const unsigned bit = kind == XH_W1 ? 1u : 2u;
            if (w.w13 && w.w13_dt != dtype) {
                if (w.w13_have & ~bit) return set_err(ctx, XH_E_INVALID, "layer %d: w1/w3 must share one dtype", layer);
                hipFree(w.w13); w.w13 = nullptr; w.w13_have = 0;
            }
            if (!(w.w13_have & ~bit)) {
                w.w13_x = false;
                w.w13_e[0] = 255; w.w13_e[1] = 0;
            }
            if (!w.w13) HIP_TRY(ctx, hipMalloc(&w.w13, (size_t)2 * c.hidden_dim * rb));
            w.w13_dt = dtype;
            out->base = (char*)w.w13 + (kind == XH_W3 ? rb : 0);
            out->pitch = 2 * rb;
            w.w13_have |= bit;
            return 0;
        }
    }
    return set_err(ctx, XH_E_INVALID, "unhandled kind");
}

// any NaN/Inf fp8 code (f8_special) in a [rows][cols] byte matrix of row pitch `pitch`
__global__ void f8_special_scan_kernel(const uint8_t* base, size_t pitch, size_t rows, size_t cols, int e5m2, int* flag) {
    int hit = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows * cols; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / cols;
        hit |= f8_special(base[r * pitch + (i - r * cols)], e5m2 != 0);
    }
    if (hit) *flag = 1;
}

// after an upload into slot s: record whether the fp8 matrix holds NaN/Inf codes
int scan_f8(xh_ctx* ctx, int kind, int layer, int dtype, const Slot& s) {
    if (dtype != XH_F8_E4M3 && dtype != XH_F8_E5M2) return 0;
    if (kind == XH_EMBED || kind == XH_ATTN_NORM || kind == XH_FFN_NORM || kind == XH_FINAL_NORM) return 0;
    HIP_TRY(ctx, hipMemsetAsync(ctx->scan_flag, 0, sizeof(int), ctx->stream));
    hipLaunchKernelGGL(f8_special_scan_kernel, dim3(2048), dim3(256), 0, ctx->stream, (const uint8_t*)s.base, s.pitch,
                       s.rows, s.cols, (int)(dtype == XH_F8_E5M2), ctx->scan_flag);
    int hit = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&hit, ctx->scan_flag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (!hit) return 0;
    drop_graphs(ctx);
    if (kind == XH_WCLS) { ctx->wcls_x = true; return 0; }
    LayerW& w = ctx->L[layer];
    switch (kind) {
        case XH_WQ: case XH_WK: case XH_WV: w.qkv_x = true; break;
        case XH_W1: case XH_W3: w.w13_x = true; break;
        case XH_WO: w.wo_x = true; break;
        case XH_W2: w.w2_x = true; break;
    }
    return 0;
}

// MXFP4: the least and greatest scale byte of the planar rows of a slot (the e plane behind the
// codes), into range[0] (min, preset to 255) and range[1] (max, preset to 0)
__global__ void mx_e_scan_kernel(const uint8_t* base, size_t pitch, size_t rows, size_t cols, int* range) {
    const size_t nb = cols / 32, off = gq_d_off(XH_MXFP4, cols);
    int lo = 255, hi = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows * nb; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / nb;
        const int e = base[r * pitch + off + (i - r * nb)];
        lo = min(lo, e);
        hi = max(hi, e);
    }
    if (lo <= hi) {
        atomicMin(range, lo);
        atomicMax(range + 1, hi);
    }
}

// after an upload into slot s: merge the MXFP4 matrix's scale range into its record; a matrix
// with a scale outside [MX_E_F16_LO, MX_E_F16_HI] has no exact f16 image (the *_x flag: the prompt
// passes decode it in registers).  e = 255 (NaN) never gets here from a host route (checked before
// the copy) and the quantizer cannot emit it; a slot that holds one all the same is refused.
int scan_mx(xh_ctx* ctx, int kind, int layer, int dtype, const Slot& s) {
    if (!gq_mx(dtype) || kind == XH_ATTN_NORM || kind == XH_FFN_NORM || kind == XH_FINAL_NORM) return 0;
    const int init[2] = {255, 0};
    int got[2] = {255, 0};
    HIP_TRY(ctx, hipMemcpyAsync(ctx->scan_flag, init, sizeof init, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(mx_e_scan_kernel, dim3(1024), dim3(256), 0, ctx->stream, (const uint8_t*)s.base, s.pitch, s.rows,
                       s.cols, ctx->scan_flag);
    HIP_TRY(ctx, hipMemcpyAsync(got, ctx->scan_flag, sizeof got, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (got[1] == 255) return set_err(ctx, XH_E_INVALID, "tensor kind %d: an MXFP4 block with e = 255 (NaN)", kind);
    uint8_t* er = nullptr;
    bool* x = nullptr;
    if (kind == XH_WCLS) { er = ctx->wcls_e; x = &ctx->wcls_x; }
    else if (kind != XH_EMBED) {
        LayerW& w = ctx->L[layer];
        switch (kind) {
            case XH_WQ: case XH_WK: case XH_WV: er = w.qkv_e; x = &w.qkv_x; break;
            case XH_W1: case XH_W3: er = w.w13_e; x = &w.w13_x; break;
            case XH_WO: er = w.wo_e; x = &w.wo_x; break;
            case XH_W2: er = w.w2_e; x = &w.w2_x; break;
        }
    }
    if (!er) return 0;
    er[0] = (uint8_t)std::min<int>(er[0], got[0]);
    er[1] = (uint8_t)std::max<int>(er[1], got[1]);
    *x = er[0] < MX_E_F16_LO || er[1] > MX_E_F16_HI;
    return 0;
}
// a host tensor of MXFP4 blocks before it is copied: e = 255 refused
int check_mx_host(xh_ctx* ctx, int kind, int dtype, const void* host, size_t bytes) {
    if (!gq_mx(dtype)) return 0;
    uint8_t lo, hi;
    mx_e_range((const uint8_t*)host, bytes / gq_block_bytes(dtype), &lo, &hi);
    if (lo <= hi && hi == 255) return set_err(ctx, XH_E_INVALID, "tensor kind %d: an MXFP4 block with e = 255 (NaN)", kind);
    return 0;
}

__global__ void synth_fill_kernel(char* base, size_t pitch, size_t rows, size_t cols, int dtype, uint64_t seed,
                                  float mean, float std) {
    const size_t n = rows * cols;
    const size_t esz = dtype == XH_F32 ? 4 : (dtype == XH_F16 || dtype == XH_BF16) ? 2 : 1;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / cols, cidx = i - r * cols;
        xs_store(base + r * pitch, cidx, dtype, xs_value(seed, i, mean, std));
        (void)esz;
    }
}

// xh_kv_fill_synthetic on an fp8 KV ring: the e4m3 rounding (kv8_pack) of the value the fp16 fill
// stores, f16(xs_value); master (K rows, null otherwise): rows of slots < 2 also as their fp16 image
__global__ void synth_fill_kv8_kernel(uint8_t* base, size_t rows, size_t cols, int slot0, uint16_t* master,
                                      uint64_t seed, float std) {
    const size_t n = rows * cols;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const uint32_t code = kv8_pack(f16_bits_to_f32(xs_to_f16(xs_value(seed, i, 0.0f, std))), 0.f) & 0xffu;
        base[i] = (uint8_t)code;
        const size_t slot = slot0 + i / cols;
        if (master && slot < 2) master[slot * cols + i % cols] = (uint16_t)kv8_image_f16x2(code);
    }
}

// the fp16 bits of an e4m3 code (finite codes; exact)
uint16_t f8_e4m3_f16_bits(const uint8_t b) {
    const int e = (b >> 3) & 15, m = b & 7;
    const float v = e ? ldexpf((float)(8 + m), e - 10) : ldexpf((float)m, -9);
    return __builtin_bit_cast(uint16_t, (_Float16)((b & 0x80) ? -v : v));
}

}  // namespace

// gguf blocks: file layout ([rows][cols/32 blocks: f16 d, f16 m (affine), u32 qh (5-bit), codes])
// -> planar device rows ([codes][qh per block][d per block][m per block][zero pad], pitch
// gq_pitch; common.h), on the host, split over threads
void xalm::gq_repack(int dt, const uint8_t* src, size_t rows, size_t cols, uint8_t* dst) {
    if (gq_k(dt)) {
        const size_t nsb = cols / 256, bs = gq_block_bytes(dt), pitch = gq_pitch(dt, cols);
        const size_t end = dt == XH_Q4_K ? pitch : kq6_d_off(cols) + 2 * nsb;
        auto part = [&](size_t r0, size_t r1) {
            for (size_t r = r0; r < r1; r++) {
                for (size_t b = 0; b < nsb; b++) kq_repack_sb(dt, src + (r * nsb + b) * bs, dst + r * pitch, cols, b);
                memset(dst + r * pitch + end, 0, pitch - end);
            }
        };
        const size_t nt = std::min<size_t>(16, std::max<size_t>(1, rows / 256));
        std::vector<std::thread> th;
        for (size_t t = 1; t < nt; t++) th.emplace_back(part, rows * t / nt, rows * (t + 1) / nt);
        part(0, rows / nt);
        for (auto& x : th) x.join();
        return;
    }
    const size_t nb = cols / 32, bs = gq_block_bytes(dt);
    const size_t hm = gq_has_m(dt) ? 2 : 0, hq = gq_has_qh(dt) ? 4 : 0;  // header bytes behind d
    const size_t ds = gq_mx(dt) ? 1 : 2;                                 // d (MXFP4: the scale byte e)
    const size_t qb = bs - gq_head_bytes(dt);
    const size_t pitch = gq_pitch(dt, cols), qbytes = gq_qbytes(dt, cols);
    const size_t d_off = gq_d_off(dt, cols), m_off = gq_m_off(dt, cols), end = gq_mx(dt) ? d_off + nb : m_off + hm * nb;
    auto part = [&](size_t r0, size_t r1) {
        for (size_t r = r0; r < r1; r++) {
            const uint8_t* in = src + r * nb * bs;
            uint8_t* out = dst + r * pitch;
            for (size_t b = 0; b < nb; b++) {
                memcpy(out + b * qb, in + b * bs + ds + hm + hq, qb);
                memcpy(out + d_off + ds * b, in + b * bs, ds);
                if (hm) memcpy(out + m_off + 2 * b, in + b * bs + 2, 2);
                if (hq) memcpy(out + qbytes + 4 * b, in + b * bs + 2 + hm, 4);
            }
            memset(out + end, 0, pitch - end);
        }
    };
    const size_t nt = std::min<size_t>(16, std::max<size_t>(1, rows / 256));
    std::vector<std::thread> th;
    for (size_t t = 1; t < nt; t++) th.emplace_back(part, rows * t / nt, rows * (t + 1) / nt);
    part(0, rows / nt);
    for (auto& x : th) x.join();
}

void xalm::mx_e_range(const uint8_t* src, size_t n_blocks, uint8_t* lo, uint8_t* hi) {
    uint8_t l = 255, h = 0;
    for (size_t b = 0; b < n_blocks; b++) {
        const uint8_t e = src[b * 17];
        l = std::min(l, e);
        h = std::max(h, e);
    }
    *lo = l;
    *hi = h;
}

namespace {

// synthetic gguf blocks: one thread per block, the values and quantizer of xalm_synth.h
// (xs_block: the oracle's bytes exactly), written straight into the planar rows of the slot
__global__ void synth_gq_kernel(char* base, size_t pitch, size_t rows, size_t cols, int dtype, uint64_t seed, float mean,
                                float std) {
    const size_t nb = cols / 32, qbytes = gq_qbytes(dtype, cols);
    const size_t hm = gq_has_m(dtype) ? 2 : 0, hq = gq_has_qh(dtype) ? 4 : 0;  // header bytes behind d
    const size_t qb = gq_block_bytes(dtype) - gq_head_bytes(dtype);
    const size_t d_off = gq_d_off(dtype, cols), m_off = gq_m_off(dtype, cols);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows * nb; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / nb, b = i - r * nb;
        uint8_t blk[34];
        xs_block(blk, dtype, seed, r, cols, b, mean, std);
        char* row = base + r * pitch;
        if (gq_mx(dtype)) {  // e, then the codes
            for (size_t k = 0; k < qb; k++) row[b * qb + k] = (char)blk[1 + k];
            row[d_off + b] = (char)blk[0];
            continue;
        }
        for (size_t k = 0; k < qb; k++) row[b * qb + k] = (char)blk[2 + hm + hq + k];
        row[d_off + 2 * b] = (char)blk[0];
        row[d_off + 2 * b + 1] = (char)blk[1];
        for (size_t k = 0; k < hm; k++) row[m_off + 2 * b + k] = (char)blk[2 + k];
        for (size_t k = 0; k < hq; k++) row[qbytes + 4 * b + k] = (char)blk[2 + hm + k];
    }
}

// synthetic K-quant super-blocks (xs_superblock), one thread each, into the planar rows.  A row's
// threads write disjoint bytes; the pad behind a Q6_K row's d plane is never read.
__global__ void synth_kq_kernel(char* base, size_t pitch, size_t rows, size_t cols, int dtype, uint64_t seed, float mean,
                                float std) {
    const size_t nsb = cols / 256;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows * nsb; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / nsb, b = i - r * nsb;
        uint8_t blk[210];
        xs_superblock(blk, dtype, seed, r, cols, b, mean, std);
        kq_repack_sb(dtype, blk, (uint8_t*)base + r * pitch, cols, b);
    }
}

// the byte count of a tensor upload against the config (load_tensor's checks,
// src/model.cpp:62-76), before the device layout is touched
int check_bytes(xh_ctx* ctx, int kind, int dtype, size_t bytes) {
    const xh_config& c = ctx->c;
    size_t rows = 0, cols = 0;
    switch (kind) {
        case XH_EMBED: case XH_WCLS: rows = c.vocab_size; cols = c.dim; break;
        case XH_ATTN_NORM: case XH_FFN_NORM: case XH_FINAL_NORM: rows = 1; cols = c.dim; break;
        case XH_WQ: rows = ctx->q_dim; cols = c.dim; break;
        case XH_WK: case XH_WV: rows = ctx->kv_dim; cols = c.dim; break;
        case XH_WO: rows = c.dim; cols = ctx->q_dim; break;
        case XH_W1: case XH_W3: rows = c.hidden_dim; cols = c.dim; break;
        case XH_W2: rows = c.dim; cols = c.hidden_dim; break;
        default: return set_err(ctx, XH_E_INVALID, "unknown tensor kind %d", kind);
    }
    const size_t rb = file_row_bytes(dtype, cols);
    if (gq_k(dtype) && cols % 256)
        return set_err(ctx, XH_E_INVALID, "tensor kind %d: %zu columns, not whole 256-element super-blocks", kind, cols);
    if (rb == 0 || (gq_dt(dtype) && cols % 32) || bytes != rows * rb)
        return set_err(ctx, XH_E_INVALID, "tensor kind %d: %zu bytes, expected %zu ([%zu,%zu] of dtype %d)", kind,
                       bytes, rows * rb, rows, cols, dtype);
    return 0;
}

}  // namespace

extern "C" {

int xh_upload(xh_ctx* ctx, int kind, int layer, int dtype, const void* host, size_t bytes) {
    if (!ctx || !host) return set_err(ctx, XH_E_INVALID, "null argument");
    HIP_TRY(ctx, hipSetDevice(ctx->dev));
    Slot s;
    int rc = check_bytes(ctx, kind, dtype, bytes);
    if (!rc) rc = check_mx_host(ctx, kind, dtype, host, bytes);
    if (!rc) rc = tensor_slot(ctx, kind, layer, dtype, &s);
    if (rc) return rc;
    if (gq_dt(dtype)) {
        const size_t rb = dev_row_bytes(dtype, s.cols);
        std::vector<uint8_t> tmp(s.rows * rb);
        gq_repack(dtype, (const uint8_t*)host, s.rows, s.cols, tmp.data());
        HIP_TRY(ctx, copy2d_sync(ctx, s.base, s.pitch, tmp.data(), rb, rb, s.rows));
        return scan_mx(ctx, kind, layer, dtype, s);
    }
    HIP_TRY(ctx, copy2d_sync(ctx, s.base, s.pitch, host, s.cols * dtype_size(dtype), s.cols * dtype_size(dtype),
                                 s.rows));
    return scan_f8(ctx, kind, layer, dtype, s);
}

// Tensor bytes straight from a file (the .xalm layout: tensor data at an absolute, 32-B
// aligned offset, convert.py:248-321) into the device slot.  The range is mapped with
// MAP_POPULATE (read ahead in one pass), registered with the runtime for the duration of
// the copy and moved by one DMA: no host copy of the tensor.  Measured on MI355X with the
// file in the page cache (tools/load_bench.py): 45 GB/s, against 16 GB/s for pread into
// two pinned staging buffers and 33 GB/s for a pageable copy of the mapping.
int xh_upload_file(xh_ctx* ctx, int kind, int layer, int dtype, const char* path, uint64_t offset, size_t bytes) {
    if (!ctx || !path) return set_err(ctx, XH_E_INVALID, "null argument");
    HIP_TRY(ctx, hipSetDevice(ctx->dev));
    int rc = check_bytes(ctx, kind, dtype, bytes);
    if (rc) return rc;
    const int fd = open(path, O_RDONLY | O_CLOEXEC);
    if (fd < 0) return set_err(ctx, XH_E_INVALID, "%s: %s", path, strerror(errno));
    struct stat st;
    if (fstat(fd, &st) != 0 || offset > (uint64_t)st.st_size || bytes > (uint64_t)st.st_size - offset) {
        close(fd);
        return set_err(ctx, XH_E_INVALID, "%s: %zu bytes at offset %llu run past the end of the file", path, bytes,
                       (unsigned long long)offset);
    }
    const uint64_t a0 = offset & ~(uint64_t)(sysconf(_SC_PAGESIZE) - 1);
    const size_t len = bytes + (size_t)(offset - a0);
    void* map = mmap(nullptr, len, PROT_READ, MAP_SHARED | MAP_POPULATE, fd, (off_t)a0);
    const int map_errno = errno;
    close(fd);
    if (map == MAP_FAILED) return set_err(ctx, XH_E_INVALID, "%s: mmap: %s", path, strerror(map_errno));
    Slot s;
    rc = check_mx_host(ctx, kind, dtype, (const char*)map + (offset - a0), bytes);
    if (!rc) rc = tensor_slot(ctx, kind, layer, dtype, &s);
    if (!rc && gq_dt(dtype)) {
        // gguf blocks: repacked on the host from the mapping (planar device rows)
        const size_t rb = dev_row_bytes(dtype, s.cols);
        std::vector<uint8_t> tmp(s.rows * rb);
        gq_repack(dtype, (const uint8_t*)map + (offset - a0), s.rows, s.cols, tmp.data());
        const hipError_t e = copy2d_sync(ctx, s.base, s.pitch, tmp.data(), rb, rb, s.rows);
        if (e != hipSuccess) rc = set_err(ctx, XH_E_HIP, "%s: copy to the device: %s", path, hipGetErrorString(e));
    } else if (!rc) {
        const size_t row_bytes = s.cols * dtype_size(dtype);
        // unregistered (e.g. a mapping the driver cannot pin) the same copy runs pageable
        const bool reg = hipHostRegister(map, len, hipHostRegisterReadOnly) == hipSuccess;
        const hipError_t e = copy2d_sync(ctx, s.base, s.pitch, (const char*)map + (offset - a0), row_bytes,
                                         row_bytes, s.rows);
        if (reg) hipHostUnregister(map);
        if (e != hipSuccess) rc = set_err(ctx, XH_E_HIP, "%s: copy to the device: %s", path, hipGetErrorString(e));
    }
    munmap(map, len);
    if (!rc) rc = scan_mx(ctx, kind, layer, dtype, s);
    return rc ? rc : scan_f8(ctx, kind, layer, dtype, s);
}

int xh_upload_synthetic(xh_ctx* ctx, int kind, int layer, int dtype, uint64_t seed, float mean, float std) {
    if (!ctx) return XH_E_INVALID;
    if (dtype == XH_Q8) return set_err(ctx, XH_E_INVALID, "no synthetic Q8");
    HIP_TRY(ctx, hipSetDevice(ctx->dev));
    Slot s;
    int rc = tensor_slot(ctx, kind, layer, dtype, &s);
    if (rc) return rc;
    if (gq_k(dtype))
        hipLaunchKernelGGL(synth_kq_kernel, dim3(1024), dim3(64), 0, ctx->stream, s.base, s.pitch, s.rows, s.cols, dtype,
                           seed, mean, std);
    else if (gq_dt(dtype))
        hipLaunchKernelGGL(synth_gq_kernel, dim3(4096), dim3(256), 0, ctx->stream, s.base, s.pitch, s.rows, s.cols, dtype,
                           seed, mean, std);
    else
        hipLaunchKernelGGL(synth_fill_kernel, dim3(4096), dim3(256), 0, ctx->stream, s.base, s.pitch, s.rows, s.cols,
                           dtype, seed, mean, std);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if ((rc = scan_mx(ctx, kind, layer, dtype, s))) return rc;
    return scan_f8(ctx, kind, layer, dtype, s);
}

int xh_quantize_blocks(int dtype, const float* values, size_t n_blocks, void* out) {
    if (!gq_dt(dtype) || !values || !out) return set_err(nullptr, XH_E_INVALID, "quantize_blocks: dtype %d is no block type, or a null pointer", dtype);
    const size_t bs = gq_block_bytes(dtype);
    if (gq_mx(dtype) || gq_k(dtype))
        for (size_t i = 0; i < gq_group(dtype) * n_blocks; i++)
            if (!std::isfinite(values[i])) return set_err(nullptr, XH_E_INVALID, "quantize_blocks: value %zu is not finite", i);
    if (gq_k(dtype)) {  // n_blocks super-blocks
        for (size_t b = 0; b < n_blocks; b++) {
            if (dtype == XH_Q4_K) xs_quant_q4_k(values + 256 * b, (uint8_t*)out + b * bs);
            else xs_quant_q6_k(values + 256 * b, (uint8_t*)out + b * bs);
        }
        return 0;
    }
    for (size_t b = 0; b < n_blocks; b++) xs_quant_block(dtype, values + 32 * b, (uint8_t*)out + b * bs);
    return 0;
}

int xh_dequantize_blocks(int dtype, const void* blocks, size_t n_blocks, float* out) {
    if (!gq_dt(dtype) || !blocks || !out) return set_err(nullptr, XH_E_INVALID, "dequantize_blocks: dtype %d is no block type, or a null pointer", dtype);
    static const float E2M1[8] = {0.f, 0.5f, 1.f, 1.5f, 2.f, 3.f, 4.f, 6.f};
    const size_t bs = gq_block_bytes(dtype);
    auto f16 = [](const uint8_t* p) { return (float)__builtin_bit_cast(_Float16, (uint16_t)(p[0] | p[1] << 8)); };
    if (gq_k(dtype)) {  // n_blocks super-blocks
        for (size_t b = 0; b < n_blocks; b++) {
            if (dtype == XH_Q4_K) xs_dequant_q4_k((const uint8_t*)blocks + b * bs, out + 256 * b);
            else xs_dequant_q6_k((const uint8_t*)blocks + b * bs, out + 256 * b);
        }
        return 0;
    }
    for (size_t b = 0; b < n_blocks; b++) {
        const uint8_t* in = (const uint8_t*)blocks + b * bs;
        float* o = out + 32 * b;
        if (gq_mx(dtype)) {
            if (in[0] == 255) return set_err(nullptr, XH_E_INVALID, "dequantize_blocks: block %zu has e = 255 (NaN)", b);
            for (int j = 0; j < 32; j++) {
                const unsigned c = j < 16 ? in[1 + j] & 15u : in[1 + j - 16] >> 4;
                o[j] = ldexpf((c & 8u) ? -E2M1[c & 7u] : E2M1[c & 7u], (int)in[0] - 127);
            }
            continue;
        }
        const float d = f16(in), m = gq_has_m(dtype) ? f16(in + 2) : 0.f;
        const uint8_t* qs = in + gq_head_bytes(dtype);
        if (dtype == XH_Q8_0) {
            for (int j = 0; j < 32; j++) o[j] = d * (float)(int8_t)qs[j];
            continue;
        }
        uint32_t qh = 0;
        if (gq_has_qh(dtype)) memcpy(&qh, in + 2 + (gq_has_m(dtype) ? 2 : 0), 4);
        for (int j = 0; j < 32; j++) {
            const int q = (int)(j < 16 ? qs[j] & 15u : qs[j - 16] >> 4) + (int)(((qh >> j) & 1u) << 4) - gq_bias(dtype);
            o[j] = gq_has_m(dtype) ? fmaf(d, (float)q, m) : d * (float)q;  // d * q is exact
        }
    }
    return 0;
}

int xh_kv_fill_synthetic(xh_ctx* ctx, int layer, int which, int slot0, int n_slots, uint64_t seed, float std) {
    if (!ctx || layer < 0 || layer >= ctx->c.n_layers || (which != 0 && which != 1) || slot0 < 0 || n_slots < 0 ||
        slot0 + n_slots > ctx->c.max_seq_len)
        return set_err(ctx, XH_E_INVALID, "bad kv_fill_synthetic arguments");
    HIP_TRY(ctx, hipSetDevice(ctx->dev));
    if (ctx->kv8()) {
        uint8_t* base8 = (uint8_t*)(which ? ctx->vcache(layer) : ctx->kcache(layer)) + (size_t)slot0 * ctx->kv_dim;
        hipLaunchKernelGGL(synth_fill_kv8_kernel, dim3(2048), dim3(256), 0, ctx->stream, base8, (size_t)n_slots,
                           (size_t)ctx->kv_dim, slot0, which ? (uint16_t*)nullptr : ctx->master(layer), seed, std);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return 0;
    }
    char* base = (char*)((which ? ctx->vcache(layer) : ctx->kcache(layer)) + (size_t)slot0 * ctx->kv_dim);
    hipLaunchKernelGGL(synth_fill_kernel, dim3(2048), dim3(256), 0, ctx->stream, base, (size_t)ctx->kv_dim * 2,
                       (size_t)n_slots, (size_t)ctx->kv_dim, (int)XH_F16, seed, 0.0f, std);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

int xh_kv_write(xh_ctx* ctx, int layer, int which, int slot0, int n_slots, const uint16_t* host) {
    if (!ctx || !host || layer < 0 || layer >= ctx->c.n_layers || (which != 0 && which != 1) || slot0 < 0 ||
        n_slots < 0 || slot0 + n_slots > ctx->c.max_seq_len)
        return set_err(ctx, XH_E_INVALID, "bad kv_write arguments");
    if (ctx->kv8()) return set_err(ctx, XH_E_INVALID, "kv_write: the context's KV ring is fp8 (xh_kv_write8)");
    HIP_TRY(ctx, hipSetDevice(ctx->dev));
    uint16_t* base = (which ? ctx->vcache(layer) : ctx->kcache(layer)) + (size_t)slot0 * ctx->kv_dim;
    HIP_TRY(ctx, copy_sync(ctx, base, host, (size_t)n_slots * ctx->kv_dim * 2, hipMemcpyHostToDevice));
    return 0;
}

int xh_kv_read(xh_ctx* ctx, int layer, int which, int slot0, int n_slots, uint16_t* host) {
    if (!ctx || !host || layer < 0 || layer >= ctx->c.n_layers || (which != 0 && which != 1) || slot0 < 0 ||
        n_slots < 0 || slot0 + n_slots > ctx->c.max_seq_len)
        return set_err(ctx, XH_E_INVALID, "bad kv_read arguments");
    if (ctx->kv8()) return set_err(ctx, XH_E_INVALID, "kv_read: the context's KV ring is fp8 (xh_kv_read8)");
    HIP_TRY(ctx, hipSetDevice(ctx->dev));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const uint16_t* base = (which ? ctx->vcache(layer) : ctx->kcache(layer)) + (size_t)slot0 * ctx->kv_dim;
    HIP_TRY(ctx, copy_sync(ctx, host, base, (size_t)n_slots * ctx->kv_dim * 2, hipMemcpyDeviceToHost));
    return 0;
}

int xh_kv_write8(xh_ctx* ctx, int layer, int which, int slot0, int n_slots, const uint8_t* host) {
    if (!ctx || !host || layer < 0 || layer >= ctx->c.n_layers || (which != 0 && which != 1) || slot0 < 0 ||
        n_slots < 0 || slot0 + n_slots > ctx->c.max_seq_len)
        return set_err(ctx, XH_E_INVALID, "bad kv_write8 arguments");
    if (!ctx->kv8()) return set_err(ctx, XH_E_INVALID, "kv_write8: the context's KV ring is fp16 (xh_kv_write)");
    const size_t kd = (size_t)ctx->kv_dim, n = (size_t)n_slots * kd;
    for (size_t i = 0; i < n; i++)
        if (f8_special(host[i], false)) return set_err(ctx, XH_E_INVALID, "kv_write8: element %zu is the NaN code", i);
    HIP_TRY(ctx, hipSetDevice(ctx->dev));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    uint8_t* base = (uint8_t*)(which ? ctx->vcache(layer) : ctx->kcache(layer)) + (size_t)slot0 * kd;
    HIP_TRY(ctx, copy_sync(ctx, base, host, n, hipMemcpyHostToDevice));
    if (which == 0 && slot0 < 2 && n_slots > 0) {  // the sinks' master: the exact fp16 image
        const size_t rows = std::min<size_t>((size_t)n_slots, (size_t)(2 - slot0));
        std::vector<uint16_t> img(rows * kd);
        for (size_t i = 0; i < img.size(); i++) img[i] = f8_e4m3_f16_bits(host[i]);
        HIP_TRY(ctx, copy_sync(ctx, ctx->master(layer) + (size_t)slot0 * kd, img.data(), img.size() * 2, hipMemcpyHostToDevice));
    }
    return 0;
}

int xh_kv_read8(xh_ctx* ctx, int layer, int which, int slot0, int n_slots, uint8_t* host) {
    if (!ctx || !host || layer < 0 || layer >= ctx->c.n_layers || (which != 0 && which != 1) || slot0 < 0 ||
        n_slots < 0 || slot0 + n_slots > ctx->c.max_seq_len)
        return set_err(ctx, XH_E_INVALID, "bad kv_read8 arguments");
    if (!ctx->kv8()) return set_err(ctx, XH_E_INVALID, "kv_read8: the context's KV ring is fp16 (xh_kv_read)");
    HIP_TRY(ctx, hipSetDevice(ctx->dev));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const uint8_t* base = (const uint8_t*)(which ? ctx->vcache(layer) : ctx->kcache(layer)) + (size_t)slot0 * ctx->kv_dim;
    HIP_TRY(ctx, copy_sync(ctx, host, base, (size_t)n_slots * ctx->kv_dim, hipMemcpyDeviceToHost));
    return 0;
}

int xh_kv_sink_read(xh_ctx* ctx, int layer, uint16_t* out) {
    if (!ctx || !out || layer < 0 || layer >= ctx->c.n_layers) return set_err(ctx, XH_E_INVALID, "bad kv_sink_read arguments");
    if (!ctx->kv8()) return set_err(ctx, XH_E_INVALID, "kv_sink_read: the context's KV ring is fp16 (no sink master)");
    HIP_TRY(ctx, hipSetDevice(ctx->dev));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, copy_sync(ctx, out, ctx->master(layer), (size_t)2 * ctx->kv_dim * 2, hipMemcpyDeviceToHost));
    return 0;
}
}  // extern "C"
