// ops.hip — single ops on host pointers for the tests (xh_op_*) and the per-kernel timing hooks
// of bench.py (xh_time_kernel, xh_kernel_bytes).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "ctx.h"
#include "standalone.h"

using namespace xalm;

extern "C" {

// ---------------------------------------------------------------------------------------
// exposed-for-tests ops (host pointers).  They run the same kernels as the forward pass.
// ---------------------------------------------------------------------------------------
namespace {
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) hipFree(p); }
};
int op_alloc(DevBuf& b, size_t bytes, const void* src) {
    if (hipMalloc(&b.p, bytes ? bytes : 16) != hipSuccess) return set_err(nullptr, XH_E_HIP, "hipMalloc failed");
    if (src && hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice) != hipSuccess)
        return set_err(nullptr, XH_E_HIP, "hipMemcpy failed");
    return 0;
}
int op_finish(void* dst, const DevBuf& b, size_t bytes) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_err(nullptr, XH_E_HIP, "kernel launch failed: %s", hipGetErrorString(e));
    if (hipDeviceSynchronize() != hipSuccess) return set_err(nullptr, XH_E_HIP, "kernel failed");
    if (hipMemcpy(dst, b.p, bytes, hipMemcpyDeviceToHost) != hipSuccess)
        return set_err(nullptr, XH_E_HIP, "hipMemcpy D2H failed");
    return 0;
}
}  // namespace

int xh_op_matmul(float* xout, const float* x, const void* w, int dtype, int n, int d) {
    if (!xout || !x || !w || n <= 0 || d <= 0 || n % 16) return set_err(nullptr, XH_E_INVALID, "bad matmul args");
    if (!matrix_dtype_ok(dtype)) return set_err(nullptr, XH_E_INVALID, "unsupported dtype %d", dtype);
    DevBuf bw, bx, bo;
    int rc;
    if (gq_dt(dtype) && n % 32) return set_err(nullptr, XH_E_INVALID, "bad matmul args: n %% 32");
    // gguf blocks: w in the file layout, repacked to the planar device rows
    std::vector<uint8_t> gq_tmp;
    if (gq_mx(dtype)) {
        uint8_t lo, hi;
        mx_e_range((const uint8_t*)w, (size_t)d * (n / 32), &lo, &hi);
        if (hi == 255) return set_err(nullptr, XH_E_INVALID, "bad matmul args: an MXFP4 block with e = 255 (NaN)");
    }
    if (gq_dt(dtype)) {
        gq_tmp.resize((size_t)d * dev_row_bytes(dtype, n));
        gq_repack(dtype, (const uint8_t*)w, d, n, gq_tmp.data());
        w = gq_tmp.data();
    }
    const size_t wbytes = (size_t)d * dev_row_bytes(dtype, n);
    if ((rc = op_alloc(bw, wbytes, w)) || (rc = op_alloc(bx, (size_t)n * 4, x)) || (rc = op_alloc(bo, (size_t)d * 4, nullptr)))
        return rc;
    GemvArgs a{};
    a.w = bw.p; a.row_bytes = dev_row_bytes(dtype, n); a.n = n; a.rows = d;
    a.x = (const float*)bx.p; a.out = (float*)bo.p;
    bool special = false;
    if (dtype == XH_F8_E4M3 || dtype == XH_F8_E5M2)
        for (size_t i = 0; i < wbytes && !special; i++) special = f8_special(((const uint8_t*)w)[i], dtype == XH_F8_E5M2);
    launch_gemv(GEMV_STORE, kdt(dtype, special), a, nullptr, 4096);
    return op_finish(xout, bo, (size_t)d * 4);
}

int xh_op_rmsnorm(float* o, const float* x, const void* weight, int dtype, int size, float eps) {
    if (!o || !x || !weight || size <= 0 || size % 4 || !(dtype == XH_F32 || dtype == XH_BF16))
        return set_err(nullptr, XH_E_INVALID, "bad rmsnorm args");
    DevBuf bw, bx, bo;
    int rc;
    if ((rc = op_alloc(bw, (size_t)size * dtype_size(dtype), weight)) || (rc = op_alloc(bx, (size_t)size * 4, x)) ||
        (rc = op_alloc(bo, (size_t)size * 4, nullptr)))
        return rc;
    hipLaunchKernelGGL(rmsnorm_kernel, dim3(1), dim3(256), 0, nullptr, (float*)bo.p, (const float*)bx.p,
                       (const void*)bw.p, dtype, size, eps);
    return op_finish(o, bo, (size_t)size * 4);
}

int xh_op_rope(float* vec, int d, int head_dim, int pos, float theta, int rotary_dim) {
    if (!vec || d <= 0 || d % 2 || head_dim <= 0 || head_dim % 2) return set_err(nullptr, XH_E_INVALID, "bad rope args");
    std::vector<float> fr(head_dim / 2);
    for (int j = 0; j < head_dim; j += 2)
        fr[j / 2] = j >= rotary_dim ? 0.f : 1.0f / powf(theta, (float)j / (float)rotary_dim);
    DevBuf bv, bf;
    int rc;
    if ((rc = op_alloc(bv, (size_t)d * 4, vec)) || (rc = op_alloc(bf, fr.size() * 4, fr.data()))) return rc;
    hipLaunchKernelGGL(rope_kernel, dim3((d / 2 + 255) / 256), dim3(256), 0, nullptr, (float*)bv.p, d, head_dim, pos,
                       (const float*)bf.p);
    return op_finish(vec, bv, (size_t)d * 4);
}

int xh_op_mha(float* xout, const uint16_t* kb, const uint16_t* vb, const float* q, int head_dim, int kv_len,
              int max_seq_len, int n_heads, int n_kv_heads) {
    if (!xout || !kb || !vb || !q || kv_len <= 0 || kv_len > max_seq_len || n_kv_heads <= 0 || n_heads % n_kv_heads)
        return set_err(nullptr, XH_E_INVALID, "bad mha args");
    const int qpk = n_heads / n_kv_heads, kv_dim = n_kv_heads * head_dim;
    const int nsplit = attn_nsplit(n_kv_heads, max_seq_len);
    const int t_max = attn_split_len(max_seq_len, nsplit);
    DevBuf bk, bv, bq, bo, bpo, bpm, bsp, bcnt;
    std::vector<int> zeros((size_t)n_kv_heads, 0);
    StepParams sp{};
    sp.kv_len = kv_len;
    sp.max_seq_len = max_seq_len;
    int rc;
    const size_t kvb = (size_t)max_seq_len * kv_dim * 2;
    if ((rc = op_alloc(bk, kvb, kb)) || (rc = op_alloc(bv, kvb, vb)) || (rc = op_alloc(bq, (size_t)n_heads * head_dim * 4, q)) ||
        (rc = op_alloc(bo, (size_t)n_heads * head_dim * 4, nullptr)) ||
        (rc = op_alloc(bpo, (size_t)nsplit * n_heads * head_dim * 4, nullptr)) ||
        (rc = op_alloc(bpm, (size_t)nsplit * n_heads * 2 * 4, nullptr)) || (rc = op_alloc(bsp, sizeof sp, &sp)) ||
        (rc = op_alloc(bcnt, zeros.size() * sizeof(int), zeros.data())))
        return rc;
    AttnArgs a{};
    a.q = (const float*)bq.p; a.kc = (const uint16_t*)bk.p; a.vc = (const uint16_t*)bv.p; a.kv_dim = kv_dim;
    a.n_heads = n_heads; a.nsplit = nsplit; a.out = (float*)bo.p; a.part_o = (float*)bpo.p;
    a.part_ml = (float*)bpm.p; a.counters = (int*)bcnt.p; a.sp = (const StepParams*)bsp.p;
    if (!launch_attn(a, head_dim, qpk, n_kv_heads, t_max, nullptr))
        return set_err(nullptr, XH_E_INVALID, "unsupported head_dim %d / qpk %d", head_dim, qpk);
    return op_finish(xout, bo, (size_t)n_heads * head_dim * 4);
}

int xh_op_prompt_gemm(float* y, const uint16_t* w, const uint16_t* xh, const uint16_t* xl, int rows, int K, int n,
                      int ks) {
    const bool args_ok = y && w && xh && xl && rows > 0 && n > 0 && K > 0 && ks >= 0 && ks <= 64;
    const int bad = args_ok ? mm_op_ks(rows, K, n, &ks) : 1;  // 1: K % MM_KMULT too
    if (bad == 1) return set_err(nullptr, XH_E_INVALID, "bad prompt_gemm args");
    if (bad) return set_err(nullptr, XH_E_INVALID, "K %d not in %d slices of 64", K, ks);
    DevBuf bw, bx, bo;
    int rc;
    const size_t xe = (size_t)n * K;
    if ((rc = op_alloc(bw, (size_t)rows * K * 2, w)) || (rc = op_alloc(bx, 2 * xe * 2, nullptr)) ||
        (rc = op_alloc(bo, (size_t)ks * n * rows * 4, nullptr)))
        return rc;
    if (hipMemcpy(bx.p, xh, xe * 2, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy((uint16_t*)bx.p + xe, xl, xe * 2, hipMemcpyHostToDevice) != hipSuccess)
        return set_err(nullptr, XH_E_HIP, "hipMemcpy failed");
    int dev = 0, n_cu = 256;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        return set_err(nullptr, XH_E_HIP, "no device");
    mm_op_launch((const uint16_t*)bw.p, (const uint16_t*)bx.p, (const uint16_t*)bx.p + xe, (float*)bo.p, rows, K, n, ks, n_cu);
    std::vector<float> part((size_t)ks * n * rows);
    if ((rc = op_finish(part.data(), bo, part.size() * 4))) return rc;
    for (size_t i = 0; i < (size_t)n * rows; i++) {
        float v = 0.f;
        for (int s = 0; s < ks; s++) v += part[(size_t)s * n * rows + i];  // slice order, as prefill_epi_kernel
        y[i] = v;
    }
    return 0;
}

namespace {
int op_n_cu(int* n_cu) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(n_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        return set_err(nullptr, XH_E_HIP, "no device");
    return 0;
}
// a forced split count against the bound the passes obey over pos0 slots of history
// (and the grid's z extent)
bool op_split_ok(int nsplit, int pos0) { return nsplit <= std::min(pf_fa_split_max(pos0), 65535); }
}  // namespace

int xh_op_prompt_attn(float* out, const float* q, const uint16_t* k, const uint16_t* v, int n, int pos0, int head_dim,
                      int n_heads, int n_kv_heads, int mode, int nsplit) {
    if (!out || !q || !k || !v || n <= 0 || pos0 < 0 || pos0 > (1 << 28) || n > (1 << 20) || nsplit < 0)
        return set_err(nullptr, XH_E_INVALID, "bad prompt_attn args");
    if (n_kv_heads <= 0 || n_heads <= 0 || n_heads > 1024 || n_heads % n_kv_heads ||
        !pf_attn_shape_ok(head_dim, n_heads / n_kv_heads))
        return set_err(nullptr, XH_E_INVALID, "prompt_attn: no prompt attention for head_dim %d, %d / %d heads", head_dim,
                       n_heads, n_kv_heads);
    if (mode != 1 && mode != 2) return set_err(nullptr, XH_E_INVALID, "prompt_attn: mode %d (1 or 2)", mode);
    const bool shared = mode == 1 && head_dim == 128;
    if (nsplit > 0 && !shared)
        return set_err(nullptr, XH_E_INVALID, "prompt_attn: splits are forced under mode 1 at head_dim 128 only");
    if (nsplit > 0 && !op_split_ok(nsplit, pos0))
        return set_err(nullptr, XH_E_INVALID, "prompt_attn: %d splits over %d slots (at most %d)", nsplit, pos0,
                       pf_fa_split_max(pos0));
    const PfAttnDims d{head_dim, n_heads, n_kv_heads};
    int rc, n_cu = 0;
    if ((rc = op_n_cu(&n_cu))) return rc;
    if (nsplit == 0) nsplit = shared ? pf_fa_pick_nsplit(d, n_cu, n, pos0, SIZE_MAX) : 1;
    DevBuf bq, bk, bv, bo, bp;
    const size_t qe = (size_t)n * n_heads * head_dim, kve = (size_t)(pos0 + n) * n_kv_heads * head_dim;
    if ((rc = op_alloc(bq, qe * 4, q)) || (rc = op_alloc(bk, kve * 2, k)) || (rc = op_alloc(bv, kve * 2, v)) ||
        (rc = op_alloc(bo, qe * 4, nullptr)) || (rc = op_alloc(bp, nsplit > 1 ? pf_fa_part_floats(d, nsplit, n) * 4 : 0, nullptr)))
        return rc;
    if (pf_fa_launch(d, shared, (const float*)bq.p, (const uint16_t*)bk.p, (const uint16_t*)bv.p, (float*)bo.p, n, pos0, nsplit,
                     (float*)bp.p, nullptr) < 0)
        return set_err(nullptr, XH_E_INVALID, "prompt_attn: head shape not instantiated");
    return op_finish(out, bo, qe * 4);
}

int xh_op_prompt_attn_ring(float* out, uint16_t* k_ring, uint16_t* v_ring, const float* q, const uint16_t* ks,
                           const uint16_t* vs, const uint16_t* sink_ver, int m, int p0, int max_seq_len, int n_heads,
                           int n_kv_heads, int nsplit) {
    if (!out || !k_ring || !v_ring || !q || !ks || !vs || !sink_ver || nsplit < 0)
        return set_err(nullptr, XH_E_INVALID, "bad prompt_attn_ring args");
    if (n_kv_heads <= 0 || n_heads <= 0 || n_heads > 1024 || n_heads % n_kv_heads || !pf_attn_shape_ok(128, n_heads / n_kv_heads))
        return set_err(nullptr, XH_E_INVALID, "prompt_attn_ring: no ring attention for %d / %d heads", n_heads, n_kv_heads);
    const int W = max_seq_len - 2;
    if (max_seq_len > (1 << 24) || W < 2 || p0 < max_seq_len || m < 3 || m > W)
        return set_err(nullptr, XH_E_INVALID, "prompt_attn_ring: m %d at p0 %d over a ring of %d (3 <= m <= %d, p0 >= %d)", m,
                       p0, max_seq_len, W, max_seq_len);
    if (nsplit > 0 && !op_split_ok(nsplit, W))
        return set_err(nullptr, XH_E_INVALID, "prompt_attn_ring: %d splits over %d slots (at most %d)", nsplit, W,
                       pf_fa_split_max(W));
    const PfAttnDims d{128, n_heads, n_kv_heads};
    int rc, n_cu = 0;
    if ((rc = op_n_cu(&n_cu))) return rc;
    if (nsplit == 0) nsplit = pf_fa_pick_nsplit(d, n_cu, m, W, SIZE_MAX);
    DevBuf bq, bk, bv, bks, bvs, bsv, bo, bp;
    const size_t kv_dim = (size_t)n_kv_heads * 128, qe = (size_t)m * n_heads * 128, ring = (size_t)max_seq_len * kv_dim;
    if ((rc = op_alloc(bq, qe * 4, q)) || (rc = op_alloc(bk, ring * 2, k_ring)) || (rc = op_alloc(bv, ring * 2, v_ring)) ||
        (rc = op_alloc(bks, m * kv_dim * 2, ks)) || (rc = op_alloc(bvs, m * kv_dim * 2, vs)) ||
        (rc = op_alloc(bsv, 2 * m * kv_dim * 2, sink_ver)) || (rc = op_alloc(bo, qe * 4, nullptr)) ||
        (rc = op_alloc(bp, pf_fa_part_floats(d, nsplit, m) * 4, nullptr)))
        return rc;
    if (pf_ring_launch(d, (const float*)bq.p, (uint16_t*)bk.p, (uint16_t*)bv.p, (const uint16_t*)bks.p, (const uint16_t*)bvs.p,
                       (const uint16_t*)bsv.p, (float*)bo.p, m, p0, max_seq_len, nsplit, (float*)bp.p, nullptr) < 0)
        return set_err(nullptr, XH_E_INVALID, "prompt_attn_ring: head shape not instantiated");
    if ((rc = op_finish(out, bo, qe * 4))) return rc;
    if (hipMemcpy(k_ring, bk.p, ring * 2, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(v_ring, bv.p, ring * 2, hipMemcpyDeviceToHost) != hipSuccess)
        return set_err(nullptr, XH_E_HIP, "hipMemcpy D2H failed");
    return 0;
}

// ---------------------------------------------------------------------------------------
// timing hooks for bench.py
// ---------------------------------------------------------------------------------------
int xh_time_kernel(xh_ctx* ctx, int which, int iters, float* avg_us) {
    if (!ctx || !avg_us || iters <= 0 || which < 0 || which > 11) return XH_E_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->dev));
    int rc = check_ready(ctx);
    if (rc) return rc;
    // the constrained head reads its tables through the block xh_decode_sample_dfa writes
    if (which == 8 && !(ctx->dfa_vocab_set && ctx->dfa_n_states && ctx->dfa_block_valid))
        return set_err(ctx, XH_E_STATE, "xh_time_kernel 8: no xh_decode_sample_dfa call under the current constraint");
    // likewise the adaptive head, its constraint included when the last call had one
    if (which == 10 && !(ctx->adapt_valid && (!ctx->adapt_constrain ||
                                              (ctx->dfa_vocab_set && ctx->dfa_n_states && ctx->dfa_block_valid))))
        return set_err(ctx, XH_E_STATE, "xh_time_kernel 10: no xh_decode_sample_adapt call under the current constraint");
    // the sequence-aware head reads ctx->adapt and ctx->dfa too: the constraint that counts is the one
    // last written to ctx->adapt, by either loop
    if (which == 11 && !(ctx->seq_valid && (!(ctx->seq_constrain || ctx->adapt_constrain) ||
                                            (ctx->dfa_vocab_set && ctx->dfa_n_states && ctx->dfa_block_valid))))
        return set_err(ctx, XH_E_STATE, "xh_time_kernel 11: no xh_decode_sample_seq call under the current constraint");
    if (which == 9 && ctx->top_n <= 0) return set_err(ctx, XH_E_STATE, "xh_time_kernel 9: xh_set_top_logprobs is 0");
    const int mb = ctx->max_gemv_waves;
    // launches rotate over the layers, so a repeat never finds its weights in the 256 MB
    // Infinity Cache (a decode step streams every layer once)
    int rot = 0;
    auto launch = [&]() -> bool {
        const int l = rot++ % ctx->c.n_layers;
        switch (which) {
            case 0: return launch_gemv(GEMV_GLU, kdt(ctx->L[l].w13_dt, ctx->L[l].w13_x), w13_args(ctx, l), ctx->stream, mb);
            case 1: return launch_gemv(GEMV_QKV, kdt(ctx->L[l].qkv_dt, ctx->L[l].qkv_x), qkv_args(ctx, l), ctx->stream,
                                                             qkv_launch_waves(ctx, l));
            case 2: return launch_gemv(GEMV_RESID, kdt(ctx->L[l].wo_dt, ctx->L[l].wo_x), wo_args(ctx, l), ctx->stream, mb);
            case 3: return launch_gemv(GEMV_RESID, kdt(ctx->L[l].w2_dt, ctx->L[l].w2_x), w2_args(ctx, l), ctx->stream, mb);
            case 4: return launch_gemv(GEMV_LOGITS, kdt(ctx->wcls_dt, ctx->wcls_x), cls_args(ctx), ctx->stream, mb);
            case 6: time_sample_head(ctx); return true;
            case 7: time_sample_ext_head(ctx); return true;
            case 8: time_sample_dfa_head(ctx); return true;
            case 9: time_top_logprobs(ctx); return true;
            case 10: time_sample_adapt_head(ctx); return true;
            case 11: time_sample_seq_head(ctx); return true;
            default:
                return launch_attn(attn_args(ctx, l), ctx->c.head_dim, ctx->qpk, ctx->c.n_kv_heads, ctx->t_max,
                                   ctx->stream);
        }
    };
    hipEvent_t e0, e1;
    HIP_TRY(ctx, hipEventCreate(&e0));
    HIP_TRY(ctx, hipEventCreate(&e1));
    for (int i = 0; i < 3; i++) launch();
    HIP_TRY(ctx, hipEventRecord(e0, ctx->stream));
    for (int i = 0; i < iters; i++) launch();
    HIP_TRY(ctx, hipEventRecord(e1, ctx->stream));
    HIP_TRY(ctx, hipEventSynchronize(e1));
    float ms = 0.f;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, e0, e1));
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    HIP_TRY(ctx, hipGetLastError());
    *avg_us = ms * 1000.f / (float)iters;
    return 0;
}

size_t xh_kernel_bytes(const xh_ctx* ctx, int which, int kv_len) {
    if (!ctx) return 0;
    const xh_config& c = ctx->c;
    const LayerW& w = ctx->L[0];
    const size_t vec = 4;
    switch (which) {
        case 0: return (size_t)2 * c.hidden_dim * file_row_bytes(w.w13_dt, c.dim) + c.dim * (vec + dtype_size(w.fn_dt)) +
                       (size_t)c.hidden_dim * vec;
        case 1: return (size_t)(ctx->q_dim + 2 * ctx->kv_dim) * file_row_bytes(w.qkv_dt, c.dim) +
                       c.dim * (vec + dtype_size(w.an_dt)) + (size_t)ctx->q_dim * vec + 2 * ctx->kv_dim * 2;
        case 2: return (size_t)c.dim * file_row_bytes(w.wo_dt, ctx->q_dim) + ctx->q_dim * vec + 2 * c.dim * vec;
        case 3: return (size_t)c.dim * file_row_bytes(w.w2_dt, c.hidden_dim) + c.hidden_dim * vec + 2 * c.dim * vec;
        case 4: return (size_t)c.vocab_size * file_row_bytes(ctx->wcls ? ctx->wcls_dt : ctx->embed_dt, c.dim) +
                       c.dim * (vec + dtype_size(ctx->final_norm_dt)) + (size_t)c.vocab_size * vec;
        case 6: return (size_t)c.vocab_size * vec + file_row_bytes(ctx->embed_dt, c.dim) + c.dim * vec;
        case 7: return (size_t)2 * c.vocab_size * vec + file_row_bytes(ctx->embed_dt, c.dim) + c.dim * vec;
        case 9: return (size_t)c.vocab_size * vec + (size_t)2 * ctx->top_n * vec;
        default: return (size_t)2 * kv_len * ctx->kv_dim * 2 + 2 * (size_t)ctx->q_dim * vec;
    }
}

}  // extern "C"
