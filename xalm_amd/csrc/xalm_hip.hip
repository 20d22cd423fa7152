// xalm_hip.hip — the device context of the C ABI (include/xalm_hip.h): create, destroy, reset,
// options.  The rest of the ABI: launch.hip (kernel dispatch), decode.hip (the per-token step),
// prefill.hip / prefill_blas.hip (prompt passes), upload.hip (weights), ops.hip (test ops, timing).
//
// Replaces the device branch under Xalm's `-d` switch: Model::forward -> _forward_cpu
// (jubruckne/Xalm src/model.cpp:120-122, src/infer.cpp:604-638) and the host weight/KV
// ownership of Model::from_xalm (src/model.cpp:48-118).
//
// Per token the stream runs (all launches captured once into a hipGraph and replayed; the
// token/position scalars live in device memory, StepParams). Default, fuse level 1:
//   embed_kernel (argmax_embed_kernel in the greedy graph)          x = embed[token]
//   per layer:
//     gemv<PRO_RMSNORM, EPI_QKV>    [Wq;Wk;Wv] (one fused matrix) + rmsnorm + clip + rope +
//                                   fp16 K/V ring write + sink re-rotation
//     attn_wo_kernel (attn_wo.h)    split-KV GQA attention; the last split of a KV head merges
//                                   the partials, then Wo rows (x += .) in the same launch
//     gemv<PRO_RMSNORM, EPI_GLU>    [W1;W3] rows interleaved + rmsnorm + silu(g)*u
//     gemv<PRO_PLAIN, EPI_RESID>    W2, x += .
//   gemv<PRO_RMSNORM, EPI_STORE>    final rmsnorm + lm_head -> logits   (OUTPUT_LOGITS)
//   gemv<PRO_RMSNORM, EPI_LOGITS>   ... + per-workgroup argmax candidates (greedy graph)
// fuse_level 0 launches attention and Wo separately.  Prompts go through prefill.h unless
// XH_OPT_PREFILL is 0: passes of up to PF_TOK_MM tokens whose GEMMs run on the LDS-tiled MFMA GEMM
// of gemm16.h (f16 weights, fp8 through their exact f16 image; split-f16 activations), else
// passes of 64 tokens on the register-streaming MFMA GEMMs of prefill.h.  (Round 2's one-launch engines — persistent,
// LDS-DMA stream, qkv+attention+Wo, column-form attention — measured slower and were removed;
// DESIGN.md §4.5 / §4.9 keep the measurements.)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "ctx.h"
#include "dt_launch.h"

using namespace xalm;

namespace {
thread_local std::string g_create_error;
}

int xalm::set_err(xh_ctx* ctx, int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf; else g_create_error = buf;
    return code;
}

// =======================================================================================
// C ABI
// =======================================================================================
extern "C" {

const char* xh_last_error(const xh_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int xh_create(const xh_config* cfg, int device_ordinal, xh_ctx** out) {
    return xh_create_kv(cfg, device_ordinal, XH_F16, out);
}

int xh_kv_dtype(const xh_ctx* ctx) { return ctx ? ctx->kv_dt : XH_E_INVALID; }

int xh_create_kv(const xh_config* cfg, int device_ordinal, int kv_dtype, xh_ctx** out) {
    if (!cfg || !out) return set_err(nullptr, XH_E_INVALID, "null argument");
    *out = nullptr;
    const xh_config& c = *cfg;
    if (kv_dtype != XH_F16 && kv_dtype != XH_F8_E4M3)
        return set_err(nullptr, XH_E_INVALID, "kv_dtype %d is neither XH_F16 nor XH_F8_E4M3", kv_dtype);
    if (kv_dtype == XH_F8_E4M3 && (c.head_dim <= 0 || c.head_dim % 16))
        return set_err(nullptr, XH_E_INVALID, "an fp8 KV ring needs head_dim %% 16 == 0 (got %d)", c.head_dim);
    if (c.dim <= 0 || c.hidden_dim <= 0 || c.head_dim <= 0 || c.n_layers <= 0 || c.n_heads <= 0 ||
        c.n_kv_heads <= 0 || c.vocab_size <= 0 || c.max_seq_len <= 2)
        return set_err(nullptr, XH_E_INVALID, "bad config dims");
    if (c.dim % 32 || c.hidden_dim % 32 || c.head_dim % 16 || (c.n_heads * c.head_dim) % 32)
        return set_err(nullptr, XH_E_INVALID, "dims must be multiples of 32 (head_dim of 16), as the reference asserts");
    if (c.n_heads % c.n_kv_heads) return set_err(nullptr, XH_E_INVALID, "n_heads %% n_kv_heads != 0");
    const int qpk = c.n_heads / c.n_kv_heads;
    if (!(qpk == 1 || qpk == 2 || qpk == 4 || qpk == 8))
        return set_err(nullptr, XH_E_INVALID, "q heads per kv head must be 1, 2, 4 or 8 (got %d)", qpk);
    if (!(c.head_dim == 16 || c.head_dim == 32 || c.head_dim == 64 || c.head_dim == 128 || c.head_dim == 256))
        return set_err(nullptr, XH_E_INVALID, "head_dim must be 16..256 power of two (got %d)", c.head_dim);
    if (c.rotary_dim > c.head_dim || c.rotary_dim < 0) return set_err(nullptr, XH_E_INVALID, "bad rotary_dim");
    {
        const int ns = attn_nsplit(c.n_kv_heads, c.max_seq_len);
        if (attn_smem_bytes(c.head_dim, qpk, attn_split_len(c.max_seq_len, ns), ns) > 160 * 1024)
            return set_err(nullptr, XH_E_INVALID, "attention tile of head_dim %d x %d q heads per kv head exceeds LDS",
                           c.head_dim, qpk);
    }
    if (c.act != XH_ACT_GELU && c.act != XH_ACT_SILU) return set_err(nullptr, XH_E_INVALID, "bad act");
    {
        // the matvecs stage their whole input in LDS: dim (qkv, W1/W3, lm_head), hidden_dim (W2) and
        // n_heads * head_dim (Wo) must fit under the smallest image any weight dtype gives (F32's;
        // xh_upload checks the dtype's own)
        const long long widest = std::max({(long long)c.dim, (long long)c.hidden_dim, (long long)c.n_heads * c.head_dim});
        if (widest > INT32_MAX || matrix_lds_bytes(XH_F32, (int)widest) > GEMV_LDS_MAX)
            return set_err(nullptr, XH_E_INVALID,
                           "a matvec input of %lld elements (the widest of dim, hidden_dim, n_heads * head_dim) does not "
                           "fit the %zu bytes of LDS a workgroup stages it in",
                           widest, GEMV_LDS_MAX);
    }

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return set_err(nullptr, XH_E_HIP, "no HIP device available");
    if (device_ordinal < 0 || device_ordinal >= ndev)
        return set_err(nullptr, XH_E_INVALID, "device %d out of range (%d devices)", device_ordinal, ndev);

    xh_ctx* ctx = new xh_ctx();
    ctx->c = c;
    ctx->dev = device_ordinal;
    ctx->L.resize(c.n_layers);
    ctx->q_dim = c.n_heads * c.head_dim;
    ctx->kv_dim = c.n_kv_heads * c.head_dim;
    ctx->qpk = qpk;
    ctx->kv_dt = kv_dtype;
    ctx->nsplit = attn_nsplit(c.n_kv_heads, c.max_seq_len);
    ctx->t_max = attn_split_len(c.max_seq_len, ctx->nsplit);
    ctx->t_max_aw = attn_split_len(c.max_seq_len, ctx->nsplit, aw_min_t(c.head_dim));
    int rc = 0;
#define CREATE_TRY(expr) do { rc = (expr); if (rc) { g_create_error = ctx->err; xh_destroy(ctx); return rc; } } while (0)
    if (hipSetDevice(device_ordinal) != hipSuccess) { delete ctx; return set_err(nullptr, XH_E_HIP, "hipSetDevice failed"); }
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
        delete ctx;
        return set_err(nullptr, XH_E_HIP, "stream create failed");
    }
    // (dmalloc counts uint16_t: an fp8 ring is half of them; kv_dim is even)
    CREATE_TRY(dmalloc(ctx, &ctx->kv, ctx->kv_bytes() / 2));
    if (ctx->kv8()) CREATE_TRY(dmalloc(ctx, &ctx->sink_master, (size_t)c.n_layers * 2 * ctx->kv_dim));
    CREATE_TRY(dmalloc(ctx, &ctx->x, (size_t)c.dim));
    CREATE_TRY(dmalloc(ctx, &ctx->q, (size_t)ctx->q_dim));
    CREATE_TRY(dmalloc(ctx, &ctx->attn_out, (size_t)ctx->q_dim));
    CREATE_TRY(dmalloc(ctx, &ctx->hb, (size_t)c.hidden_dim));
    CREATE_TRY(dmalloc(ctx, &ctx->logits, (size_t)c.vocab_size));
    CREATE_TRY(dmalloc(ctx, &ctx->part_o, (size_t)ctx->nsplit * ctx->q_dim));
    CREATE_TRY(dmalloc(ctx, &ctx->part_ml, (size_t)ctx->nsplit * c.n_heads * 2));
    CREATE_TRY(dmalloc(ctx, &ctx->attn_cnt, (size_t)c.n_kv_heads));
    CREATE_TRY(dmalloc(ctx, &ctx->aw_sync, (size_t)c.n_layers * AW_SYNC_WORDS));
    CREATE_TRY(dmalloc(ctx, &ctx->cand, (size_t)ARGMAX_CANDS));
    CREATE_TRY(dmalloc(ctx, &ctx->scan_flag, (size_t)2));  // fp8: one flag; MXFP4: (min e, max e)
    CREATE_TRY(dmalloc(ctx, &ctx->samp, (size_t)1));
    CREATE_TRY(dmalloc(ctx, &ctx->ext, (size_t)1));
    CREATE_TRY(dmalloc(ctx, &ctx->ext_ring, (size_t)XH_CTL_MAX_WINDOW));
    CREATE_TRY(dmalloc(ctx, &ctx->ext_btok, (size_t)XH_CTL_MAX_BIAS));
    CREATE_TRY(dmalloc(ctx, &ctx->ext_bval, (size_t)XH_CTL_MAX_BIAS));
    CREATE_TRY(dmalloc(ctx, &ctx->ext_adj, (size_t)c.vocab_size));
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device_ordinal) != hipSuccess) {
            g_create_error = "hipGetDeviceProperties failed";
            xh_destroy(ctx);
            return XH_E_HIP;
        }
        ctx->n_cu = prop.multiProcessorCount;
    }
    ctx->aw_trace_len = (size_t)8 * ((size_t)c.n_kv_heads * ctx->nsplit + 4096);
    CREATE_TRY(dmalloc(ctx, &ctx->aw_trace, ctx->aw_trace_len));
    CREATE_TRY(dmalloc(ctx, &ctx->rope_freq, (size_t)c.head_dim / 2));
    CREATE_TRY(dmalloc(ctx, &ctx->rope_cs, (size_t)c.head_dim));
    CREATE_TRY(dmalloc(ctx, &ctx->sink_cos, (size_t)c.head_dim / 2));
    CREATE_TRY(dmalloc(ctx, &ctx->sink_sin, (size_t)c.head_dim / 2));
    CREATE_TRY(dmalloc(ctx, &ctx->sp, 1));
    ctx->dec_cap = 1 << 16;
    CREATE_TRY(dmalloc(ctx, &ctx->dec_tokens, (size_t)ctx->dec_cap));
    CREATE_TRY(dmalloc(ctx, &ctx->dec_logprobs, (size_t)ctx->dec_cap));
    CREATE_TRY(dmalloc(ctx, &ctx->dfa, (size_t)1));
    CREATE_TRY(dmalloc(ctx, &ctx->dec_states, (size_t)ctx->dec_cap));
    CREATE_TRY(dmalloc(ctx, &ctx->adapt, (size_t)1));
    CREATE_TRY(dmalloc(ctx, &ctx->adapt_negd, (size_t)c.vocab_size));
    CREATE_TRY(dmalloc(ctx, &ctx->seq, (size_t)1));
    CREATE_TRY(dmalloc(ctx, &ctx->seq_brk, (size_t)XH_SEQ_MAX_BREAKERS));
    CREATE_TRY(dmalloc(ctx, &ctx->seq_tail, (size_t)1));
    if (hipHostMalloc((void**)&ctx->sp_host, sizeof(StepParams), hipHostMallocDefault) != hipSuccess) {
        g_create_error = "hipHostMalloc failed";
        xh_destroy(ctx);
        return XH_E_HIP;
    }
    memset(ctx->sp_host, 0, sizeof(StepParams));
    ctx->sp_host->max_seq_len = c.max_seq_len;
    // rope frequencies with the host libm, exactly the reference expression (src/infer.cpp:310-312)
    std::vector<float> fr(c.head_dim / 2), sc(c.head_dim / 2), sn(c.head_dim / 2);
    for (int j = 0; j < c.head_dim; j += 2) {
        const float freq = j >= c.rotary_dim ? 0.f : 1.0f / powf(c.rope_theta, (float)j / (float)c.rotary_dim);
        fr[j / 2] = freq;
        const float val = 1 * freq;  // sink re-rotation: rope at pos = 1 (src/infer.cpp:426)
        sc[j / 2] = cosf(val);
        sn[j / 2] = sinf(val);
    }
    if (copy_sync(ctx, ctx->rope_freq, fr.data(), fr.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
        copy_sync(ctx, ctx->sink_cos, sc.data(), sc.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
        copy_sync(ctx, ctx->sink_sin, sn.data(), sn.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
        copy_sync(ctx, ctx->sp, ctx->sp_host, sizeof(StepParams), hipMemcpyHostToDevice) != hipSuccess) {
        g_create_error = "initial copies failed";
        xh_destroy(ctx);
        return XH_E_HIP;
    }
#undef CREATE_TRY
    *out = ctx;
    return 0;
}

void xh_destroy(xh_ctx* ctx) {
    if (!ctx) return;
    hipSetDevice(ctx->dev);
    if (ctx->stream) hipStreamSynchronize(ctx->stream);
    drop_graphs(ctx);
    for (auto& w : ctx->L) {
        hipFree(w.wqkv); hipFree(w.w13); hipFree(w.wo); hipFree(w.w2); hipFree(w.attn_norm); hipFree(w.ffn_norm);
    }
    if (ctx->wcls && ctx->wcls != ctx->embed) hipFree(ctx->wcls);
    hipFree(ctx->embed); hipFree(ctx->final_norm);
    hipFree(ctx->kv); hipFree(ctx->sink_master); hipFree(ctx->x); hipFree(ctx->q); hipFree(ctx->attn_out); hipFree(ctx->hb);
    hipFree(ctx->logits); hipFree(ctx->part_o); hipFree(ctx->part_ml); hipFree(ctx->attn_cnt); hipFree(ctx->aw_sync); hipFree(ctx->cand); hipFree(ctx->scan_flag);
    hipFree(ctx->samp);
    hipFree(ctx->ext); hipFree(ctx->ext_ring); hipFree(ctx->ext_btok); hipFree(ctx->ext_bval); hipFree(ctx->ext_adj);
    hipFree(ctx->dec_logprobs);
    hipFree(ctx->dfa); hipFree(ctx->dfa_bytes); hipFree(ctx->dfa_offsets); hipFree(ctx->dfa_next); hipFree(ctx->dfa_accept);
    hipFree(ctx->dec_states);
    hipFree(ctx->adapt); hipFree(ctx->adapt_negd);
    hipFree(ctx->seq); hipFree(ctx->seq_brk); hipFree(ctx->seq_tail);
    hipFree(ctx->top_n_dev); hipFree(ctx->top_ids); hipFree(ctx->top_lps); hipFree(ctx->top_rank); hipFree(ctx->top_tlp);
    pf_free(ctx);
    hipFree(ctx->pf_wdq); hipFree(ctx->ppl_tgt); hipFree(ctx->ppl_prob); hipFree(ctx->rope_freq); hipFree(ctx->rope_cs);
    hipFree(ctx->aw_trace);
    blas_free(ctx);
    hipFree(ctx->sink_cos); hipFree(ctx->sink_sin); hipFree(ctx->sp); hipFree(ctx->dec_tokens);
    if (ctx->sp_host) hipHostFree(ctx->sp_host);
    if (ctx->stream) hipStreamDestroy(ctx->stream);
    delete ctx;
}

int xh_reset(xh_ctx* ctx) {
    if (!ctx) return XH_E_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->dev));
    const xh_config& c = ctx->c;
    HIP_TRY(ctx, hipMemsetAsync(ctx->kv, 0, ctx->kv_bytes(), ctx->stream));
    if (ctx->kv8()) HIP_TRY(ctx, hipMemsetAsync(ctx->sink_master, 0, (size_t)c.n_layers * 2 * ctx->kv_dim * 2, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(ctx->x, 0, (size_t)c.dim * 4, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(ctx->logits, 0, (size_t)c.vocab_size * 4, ctx->stream));
    // the attention + Wo hand-off words (normally zeroed by each layer's W1/W3 launch): a step
    // that failed between the two launches must not leave a stale arrival count
    HIP_TRY(ctx, hipMemsetAsync(ctx->aw_sync, 0, (size_t)c.n_layers * AW_SYNC_WORDS * 4, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(ctx->cand, 0, ARGMAX_CANDS * 8, ctx->stream));
    ctx->cand_valid = true;  // all-zero candidates = zero logits (argmax token 0)
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

size_t xh_active_bytes(const xh_ctx* ctx, size_t pos) {
    // Model::active_bytes, src/model.cpp:12-35
    if (!ctx) return 0;
    const xh_config& c = ctx->c;
    size_t bytes = file_row_bytes(ctx->embed_dt, c.dim);
    bytes += (size_t)c.dim * dtype_size(ctx->final_norm_dt);
    const int wdt = ctx->wcls ? ctx->wcls_dt : ctx->embed_dt;
    bytes += (size_t)c.vocab_size * file_row_bytes(wdt, c.dim);
    const size_t kv_len = (size_t)c.max_seq_len < pos + 1 ? (size_t)c.max_seq_len : pos + 1;
    for (int l = 0; l < c.n_layers; ++l) {
        const LayerW& w = ctx->L[l];
        bytes += (size_t)c.dim * dtype_size(w.an_dt) + (size_t)c.dim * dtype_size(w.fn_dt);
        bytes += (size_t)(ctx->q_dim + 2 * ctx->kv_dim) * file_row_bytes(w.qkv_dt, c.dim);
        bytes += (size_t)c.dim * file_row_bytes(w.wo_dt, ctx->q_dim);
        bytes += (size_t)2 * c.hidden_dim * file_row_bytes(w.w13_dt, c.dim);
        bytes += (size_t)c.dim * file_row_bytes(w.w2_dt, c.hidden_dim);
        bytes += 2 * kv_len * ctx->kv_dim * ctx->kv_esz();
    }
    return bytes;
}

int xh_debug_trace(xh_ctx* ctx, int enable, uint64_t* out, int cap, int* len) {
    if (!ctx) return XH_E_INVALID;
    const int n = (int)ctx->aw_trace_len;
    if (len) *len = n;
    if (out && cap > 0) {
        HIP_TRY(ctx, hipSetDevice(ctx->dev));
        HIP_TRY(ctx, copy_sync(ctx, out, ctx->aw_trace, (size_t)std::min(cap, n) * sizeof(uint64_t), hipMemcpyDeviceToHost));
    }
    if (enable >= 0) {
        ctx->aw_trace_on = (enable & 2) != 0;
        ctx->w13_trace_on = (enable & 8) != 0;
        ctx->layer_trace_on = (enable & 16) != 0 && ctx->aw_trace_len >= LT_WORDS;
        drop_graphs(ctx);
        HIP_TRY(ctx, fill_sync(ctx, ctx->aw_trace, 0, (size_t)n * sizeof(uint64_t)));
    }
    return 0;
}

int xh_debug_read(xh_ctx* ctx, int which, float* out, size_t cap) {
    if (!ctx || !out) return set_err(ctx, XH_E_INVALID, "null argument");
    const float* src = nullptr;
    size_t n = 0;
    switch (which) {
        case XH_READ_X: src = ctx->x; n = (size_t)ctx->c.dim; break;
        case XH_READ_Q: src = ctx->q; n = (size_t)ctx->q_dim; break;
        case XH_READ_HB: src = ctx->hb; n = (size_t)ctx->c.hidden_dim; break;
        default: return set_err(ctx, XH_E_INVALID, "xh_debug_read: unknown buffer %d", which);
    }
    if (cap < n) return set_err(ctx, XH_E_INVALID, "xh_debug_read: %zu floats do not hold the buffer's %zu", cap, n);
    HIP_TRY(ctx, hipSetDevice(ctx->dev));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, copy_sync(ctx, out, src, n * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

int xh_gemv_shape(int role, int dtype, int n) { return gemv_shape(role, dtype, n); }

// The values attn_block and attn_wo_kernel form on the device from kv_len, through the functions
// they form them with (attention.h, attn_wo.h): the split launch is attn_block<HD, QPK,
// ATTN_THREADS, false, 0>; the fused launch attn_block<.., AW_THREADS, aw_partials(stage),
// aw_mint(hd, stage)> with T from aw_min_t, as attn_wo_kernel instantiates and computes them.
int xh_attn_plan(int head_dim, int n_heads, int n_kv_heads, int max_seq_len, int kv_dtype, int fused, int kv_len,
                 xh_attn_plan_t* out) {
    if (!out || n_kv_heads <= 0 || n_heads <= 0 || n_heads % n_kv_heads || kv_len <= 0 || kv_len > max_seq_len)
        return set_err(nullptr, XH_E_INVALID, "bad attn_plan args");
    if (kv_dtype != XH_F16 && kv_dtype != XH_F8_E4M3) return set_err(nullptr, XH_E_INVALID, "attn_plan: bad kv_dtype %d", kv_dtype);
    const int hd = head_dim, qpk = n_heads / n_kv_heads;
    if (!(qpk == 1 || qpk == 2 || qpk == 4 || qpk == 8) || !(hd == 16 || hd == 32 || hd == 64 || hd == 128 || hd == 256))
        return set_err(nullptr, XH_E_INVALID, "attn_plan: no attention kernel for head_dim %d x %d q heads per kv head", hd, qpk);
    if (fused && (kv_dtype != XH_F16 || !aw_instantiated(hd, qpk)))
        return set_err(nullptr, XH_E_INVALID, "attn_plan: no fused attention + Wo launch for head_dim %d x %d, kv dtype %d", hd,
                       qpk, kv_dtype);
    xh_attn_plan_t p{};
    p.fused = fused ? 1 : 0;
    p.nsplit = attn_nsplit(n_kv_heads, max_seq_len);
    const int threads = fused ? AW_THREADS : ATTN_THREADS;
    // T: the kernels take it from their block's floor (attn_block_min_t; the fused kernel from
    // aw_min_t, which both of its forms' floors equal)
    p.T = attn_split_len(kv_len, p.nsplit, fused ? aw_min_t(hd) : attn_block_min_t(hd, kv_dtype, qpk, threads, false, 0));
    p.n_active = (kv_len + p.T - 1) / p.T;
    p.stage = fused ? aw_stage_form(p.n_active) : 0;
    const bool partials = fused && aw_partials(p.stage);
    if (fused && attn_block_min_t(hd, kv_dtype, qpk, threads, partials, aw_mint(hd, p.stage)) != aw_min_t(hd))
        return set_err(nullptr, XH_E_INVALID, "attn_plan: the fused launch's block floor differs from aw_min_t");
    p.step = attn_step(hd, kv_dtype, qpk, threads, partials);
    const int full = kv_len < p.T ? kv_len : p.T, last = kv_len - (p.n_active - 1) * p.T;
    p.rounds_full = (full + p.step - 1) / p.step;
    p.rounds_last = (last + p.step - 1) / p.step;
    p.wph = attn_wph(qpk, threads, partials);
    if (!partials && p.n_active > 1) {
        p.merge_mb = attn_merge_mb(p.n_active, attn_merge_groups(qpk * hd, threads));
        p.merge_nc = attn_merge_nc(p.merge_mb);
    }
    *out = p;
    return 0;
}

int xh_get_option(const xh_ctx* ctx, int option, int* value) {
    if (!ctx || !value) return XH_E_INVALID;
    switch (option) {
        case XH_OPT_FUSE_ATTN_WO: *value = ctx->fuse_attn_wo ? 1 : 0; return 0;
        case XH_OPT_PREFILL: *value = ctx->prefill_batched ? ctx->prefill_gemm : 0; return 0;
        case XH_OPT_PREFILL_GLU_SPLIT: *value = ctx->pf_glu_split ? 1 : 0; return 0;
        case XH_OPT_PREFILL_ATTN: *value = ctx->pf_attn_mode; return 0;
        case XH_OPT_PREFILL_ATTN_SPLIT: *value = ctx->pf_fa_split; return 0;
        case XH_OPT_PREFILL_RING: *value = ctx->pf_ring ? 1 : 0; return 0;
        case XH_OPT_PREFILL_ATTN_KV8: *value = ctx->pf_attn_kv8 ? 1 : 0; return 0;
        case XH_OPT_PREFILL_RING_KV8: *value = ctx->pf_ring_kv8 ? 1 : 0; return 0;
        default: return XH_E_INVALID;
    }
}

int xh_set_option(xh_ctx* ctx, int option, int value) {
    if (!ctx) return XH_E_INVALID;
    switch (option) {
        case XH_OPT_FUSE_ATTN_WO:
            if (value < 0 || value > 1) return set_err(ctx, XH_E_INVALID, "fuse level %d not in 0..1", value);
            ctx->fuse_attn_wo = value != 0;
            drop_graphs(ctx);
            return 0;
        case XH_OPT_PREFILL:
            if (value < 0 || value > 4) return set_err(ctx, XH_E_INVALID, "XH_OPT_PREFILL: 0 ... 4");
            ctx->prefill_batched = value != 0;
            if (value) ctx->prefill_gemm = value;
            return 0;
        case XH_OPT_PREFILL_GLU_SPLIT:
            if (value < 0 || value > 1) return set_err(ctx, XH_E_INVALID, "XH_OPT_PREFILL_GLU_SPLIT: 0 or 1");
            ctx->pf_glu_split = value != 0;
            ctx->pf_resid_norm = value != 0;
            return 0;
        case XH_OPT_PREFILL_ATTN:
            if (value < 0 || value > 2) return set_err(ctx, XH_E_INVALID, "XH_OPT_PREFILL_ATTN: 0, 1 or 2");
            ctx->pf_attn_mode = value;
            return 0;
        case XH_OPT_PREFILL_ATTN_SPLIT:
            if (value < 0 || value > 1) return set_err(ctx, XH_E_INVALID, "XH_OPT_PREFILL_ATTN_SPLIT: 0 or 1");
            ctx->pf_fa_split = value;
            return 0;
        case XH_OPT_PREFILL_RING:
            if (value < 0 || value > 1) return set_err(ctx, XH_E_INVALID, "XH_OPT_PREFILL_RING: 0 or 1");
            ctx->pf_ring = value != 0;
            return 0;
        case XH_OPT_PREFILL_ATTN_KV8:
            if (value < 0 || value > 1) return set_err(ctx, XH_E_INVALID, "XH_OPT_PREFILL_ATTN_KV8: 0 or 1");
            ctx->pf_attn_kv8 = value != 0;
            return 0;
        case XH_OPT_PREFILL_RING_KV8:
            if (value < 0 || value > 1) return set_err(ctx, XH_E_INVALID, "XH_OPT_PREFILL_RING_KV8: 0 or 1");
            ctx->pf_ring_kv8 = value != 0;
            return 0;
        default: return set_err(ctx, XH_E_INVALID, "unknown option %d", option);
    }
}

int xh_set_graphs(xh_ctx* ctx, int enable) {
    if (!ctx) return XH_E_INVALID;
    ctx->use_graphs = enable != 0;
    if (!ctx->use_graphs) drop_graphs(ctx);
    return 0;
}
}  // extern "C"
