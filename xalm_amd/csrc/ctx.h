// ctx.h — the device context and what the host translation units share (internal, not installed).
// Functions that cross units live in namespace xalm; each is defined in the unit named above it.
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <type_traits>
#include <vector>

#include "attention.h"
#include "gemv.h"

namespace xalm {

inline size_t dtype_size(int dt) {
    switch (dt) {
        case XH_F32: return 4;
        case XH_F16: case XH_BF16: return 2;
        case XH_F8_E4M3: case XH_F8_E5M2: case XH_Q8: case XH_U8: return 1;
        default: return 0;
    }
}
inline bool matrix_dtype_ok(int dt) {
    return dt == XH_F32 || dt == XH_F16 || dt == XH_BF16 || dt == XH_F8_E4M3 || dt == XH_F8_E5M2 || dt == XH_Q8 ||
           gq_dt(dt);
}
// bytes of one [n]-element row: in the device layout (gguf blocks: planar, gq_pitch) and in
// the .xalm file / host upload (gguf blocks: n/32 blocks, or n/256 super-blocks, of gq_block_bytes)
inline size_t dev_row_bytes(int dt, size_t n) { return gq_dt(dt) ? gq_pitch(dt, n) : n * dtype_size(dt); }
inline size_t file_row_bytes(int dt, size_t n) { return gq_dt(dt) ? n / gq_group(dt) * gq_block_bytes(dt) : n * dtype_size(dt); }
inline int elems_per_16b(int dt) { return 16 / (int)dtype_size(dt); }
// LDS bytes of the decode matvec's x image for an n-column matrix of dt (gemv_smem_bytes); the
// f32 image is the smallest of any dtype
inline size_t matrix_lds_bytes(int dt, int n) {
    const bool nib = gq_dt(dt) && dt != XH_Q8_0 && !gq_mx(dt) && dt != XH_Q6_K;  // gq4_image
    return gemv_lds_bytes(nib || gq_mx(dt) || dt == XH_Q6_K ? 32 : gq_dt(dt) ? 16 : elems_per_16b(dt), nib, n);
}
// the kernel's decode form for a matrix: fp8 with NaN/Inf codes -> the exact bit decoder
inline int kdt(int dt, bool special) {
    if (!special) return dt;
    return dt == XH_F8_E4M3 ? XH_F8_E4M3_EXACT : dt == XH_F8_E5M2 ? XH_F8_E5M2_EXACT : dt;
}

struct LayerW {
    void* wqkv = nullptr; int qkv_dt = 0; unsigned qkv_have = 0;  // bit0 q, bit1 k, bit2 v
    void* w13 = nullptr; int w13_dt = 0; unsigned w13_have = 0;   // bit0 w1, bit1 w3
    void* wo = nullptr; int wo_dt = 0;
    void* w2 = nullptr; int w2_dt = 0;
    // fp8 matrices holding NaN/Inf codes (decoded with the exact bit form, no fused kernels);
    // MXFP4 matrices with a scale byte outside [MX_E_F16_LO, MX_E_F16_HI] (no exact f16 image:
    // the prompt passes decode them in registers)
    bool qkv_x = false, w13_x = false, wo_x = false, w2_x = false;
    // MXFP4: the least and greatest scale byte e uploaded into each matrix (255, 0: none yet)
    uint8_t qkv_e[2] = {255, 0}, w13_e[2] = {255, 0}, wo_e[2] = {255, 0}, w2_e[2] = {255, 0};
    void* attn_norm = nullptr; int an_dt = 0;
    void* ffn_norm = nullptr; int fn_dt = 0;
};

struct BlasState;  // hipBLASLt handle, workspace, plans (prefill_blas.hip)

// xh_decode_sample_ext's device parameter block (sample_ext.h): xh_sampling, the scalars of
// xh_logit_ctl, and the number of tokens the window ring has received (history, then one per step:
// the step head itself appends)
struct ExtCtl {
    xh_sampling samp;
    float repeat_penalty, presence_penalty, frequency_penalty;
    int last_n;
    float min_p;
    int n_bias;
    int count;
};

// xh_decode_sample_dfa's device block (sample_dfa.h): the tables of xh_byte_dfa and the pieces
// (device pointers: a new DFA changes the block, not the graph), the current state, which the step
// head advances, and the call's end tokens
struct DfaCtl {
    const uint16_t* next;
    const uint8_t* accept;
    const uint8_t* bytes;
    const uint32_t* offsets;
    int n_states;
    uint32_t state;
    int stop_a, stop_b;
};

// xh_decode_sample_adapt's device block (sample_adapt.h): the fields of xh_trunc_ctl, Mirostat's mu,
// which the step head reads and writes every step, and whether the DFA mask runs
struct AdaptCtl {
    float typical_p, top_n_sigma, tau, eta;
    float mu;
    int constrain;
};

// xh_decode_sample_seq's device block (sample_seq.h): the scalars of xh_seq_ctl (the breakers sit,
// sorted, in a buffer of their own)
struct SeqCtl {
    float dry_multiplier, dry_base;
    int dry_allowed, ngram, last_n, n_breakers;
    float xtc_p, xtc_thr;
};

// What sample_seq_embed_kernel's tail needs (the outputs, the embedding, the rope table), in a device
// block instead of eleven kernel arguments.  As arguments they sit in SGPRs from the kernel's first
// instruction; with the sequence stage's scalars on top the head ran out of SGPRs, and the spill slots
// the register allocator made then stayed in the frame as a 68-byte private segment even where it
// spilled nothing in the end.  The block is read behind the draw, when the stages' scalars are dead.
struct SeqTail {
    int* tokens;
    float* logprobs;
    uint32_t* states;
    const void* emb;
    float* x;
    const float* rope_freq;
    float* rope_cs;
    int cap, dtype, dim, half;
};

constexpr int ARGMAX_CANDS = 1024;  // the lm_head workgroups' argmax keys (argmax_embed_kernel's block size)

// The kinds of per-token step (decode.hip).  A kind names the step's head, the launch that puts its
// token in place, and with it the captured graph in xh_ctx::g_step: STEP_LOGITS and STEP_HYDRATE run a
// token the host gave, with and without the lm_head; the others are the decode loop's steps, the token
// chosen on the device under the greedy, sampled, extended, constrained, adaptive or sequence-aware
// head.  The sampled heads are cumulative: each takes the parameter blocks of the one before it.
enum StepKind { STEP_LOGITS, STEP_HYDRATE, STEP_GREEDY, STEP_SAMPLE, STEP_SAMPLE_EXT, STEP_SAMPLE_DFA, STEP_SAMPLE_ADAPT,
                STEP_SAMPLE_SEQ, N_STEP_KINDS };

// The batched prefill's device buffers (prefill.hip), in growth groups.  T = cap[PASS] tokens, the
// pass length in use: a longer pass frees every group and reallocates PASS; the others are
// allocated on their first use and sized to T.
struct PfBufs {
    enum Group { PASS, ATTN0, RING, LOGITS, N_GROUPS };
    int cap[N_GROUPS] = {};                // tokens each group holds
    // PASS
    uint16_t* xh = nullptr;                // [2T][max K] f16 halves of a GEMM input
    uint16_t* xl = nullptr;                // [PF_TOK][max K] the split kernel's lo fragments
    float* xs = nullptr;                   // [T] 1 / row scale
    int* tok = nullptr;                    // [T]
    float *x = nullptr, *xn = nullptr;     // [T][dim]
    float *q = nullptr, *att = nullptr;    // [T][q_dim]
    float* h = nullptr;                    // [T][hidden]
    float* part = nullptr;                 // split-K partials [ks][n][rows] (pf_part_floats)
    StepParams* sp = nullptr;              // [T] per-token attention scalars
    // ATTN0: the per-token split attention (XH_OPT_PREFILL_ATTN 0 only)
    float *po = nullptr, *pml = nullptr;   // [T][nsplit][q_dim], [T][nsplit][n_heads][2]
    int* cnt = nullptr;                    // [T][n_kv_heads] split tickets
    // RING: ring passes (positions >= max_seq_len, XH_OPT_PREFILL_RING); elements of the ring's type
    // (an fp8 ring: one code each, rows of kv_dim bytes)
    uint16_t *ks = nullptr, *vs = nullptr; // [T][kv_dim] the pass's K / V rows until its attention ran
    uint16_t* sinkv = nullptr;             // [T][2][kv_dim] sink K rows after 1 .. T re-rotations (one layer's)
    uint16_t* sinkm = nullptr;             // fp8 only: [2][kv_dim] fp16, the master after the pass's last rotation
    // LOGITS: xh_perplexity's per-token logits of a pass and their targets
    float* logits = nullptr;               // [T][vocab]
    int* tgt = nullptr;                    // [T]

    // every pointer a group owns: what pf_free and the group allocators walk
    std::vector<void**> owned(int g) {
        switch (g) {
            case PASS: return {(void**)&xh, (void**)&xl, (void**)&xs, (void**)&tok, (void**)&x, (void**)&xn,
                               (void**)&q, (void**)&att, (void**)&h, (void**)&part, (void**)&sp};
            case ATTN0: return {(void**)&po, (void**)&pml, (void**)&cnt};
            case RING: return {(void**)&ks, (void**)&vs, (void**)&sinkv, (void**)&sinkm};
            case LOGITS: return {(void**)&logits, (void**)&tgt};
            default: return {};
        }
    }
    void free_group(int g) {
        for (void** p : owned(g)) { hipFree(*p); *p = nullptr; }
        cap[g] = 0;
    }
};

}  // namespace xalm

struct xh_ctx {
    xh_config c{};
    int dev = 0;
    hipStream_t stream = nullptr;
    std::string err;
    std::vector<xalm::LayerW> L;
    void* embed = nullptr; int embed_dt = 0;
    void* final_norm = nullptr; int final_norm_dt = 0;
    void* wcls = nullptr; int wcls_dt = 0; bool wcls_x = false;
    uint8_t wcls_e[2] = {255, 0};  // MXFP4: its scale bytes' range, as LayerW's
    int* scan_flag = nullptr;  // device word for the fp8 special-code scan
    int q_dim = 0, kv_dim = 0, qpk = 0;
    uint16_t* kv = nullptr;  // [n_layers][2][max_seq_len][kv_dim]: fp16 bits, or one e4m3 code each (kv_dt)
    int kv_dt = XH_F16;      // xh_create_kv: XH_F16 or XH_F8_E4M3
    // fp8 KV only: the fp16 master of K slots 0 and 1 [n_layers][2][kv_dim] (what rotate_sinks
    // rotates; ring K slot r is its e4m3 rounding at all times)
    uint16_t* sink_master = nullptr;
    bool kv8() const { return kv_dt == XH_F8_E4M3; }
    size_t kv_esz() const { return kv8() ? 1 : 2; }
    size_t kv_bytes() const { return (size_t)c.n_layers * 2 * c.max_seq_len * kv_dim * kv_esz(); }
    uint16_t* master(int l) { return sink_master + (size_t)l * 2 * kv_dim; }
    float *x = nullptr, *q = nullptr, *attn_out = nullptr, *hb = nullptr, *logits = nullptr;
    float *part_o = nullptr, *part_ml = nullptr;
    int* attn_cnt = nullptr;        // [n_kv_heads] split arrival tickets
    float *rope_freq = nullptr, *sink_cos = nullptr, *sink_sin = nullptr;
    float* rope_cs = nullptr;  // [head_dim]: this step's rotations (rope_table, gemv.h)
    xalm::StepParams* sp = nullptr;       // device
    xalm::StepParams* sp_host = nullptr;  // pinned
    int* dec_tokens = nullptr;      // device, decode loop output
    unsigned long long* cand = nullptr;  // device [ARGMAX_CANDS]: lm_head workgroups' argmax keys
    bool cand_valid = false;        // cand describes the logits on the device
    xh_sampling* samp = nullptr;    // device: xh_decode_sample's parameter block (read by its graph)
    // xh_decode_sample_ext (sample_ext.h): parameter block, window ring [XH_CTL_MAX_WINDOW], bias
    // table [XH_CTL_MAX_BIAS] each, adjusted logits [vocab], per-step log-probabilities [dec_cap]
    xalm::ExtCtl* ext = nullptr;
    int* ext_ring = nullptr;
    int* ext_btok = nullptr;
    float* ext_bval = nullptr;
    float* ext_adj = nullptr;
    float* dec_logprobs = nullptr;
    // xh_decode_sample_dfa (sample_dfa.h): parameter block, the pieces (xh_constraint_set_vocab), the
    // DFA (xh_constraint_set; dfa_n_states 0 = none), per-step successor states [dec_cap]
    xalm::DfaCtl* dfa = nullptr;
    uint8_t* dfa_bytes = nullptr;
    uint32_t* dfa_offsets = nullptr;
    bool dfa_vocab_set = false;
    uint16_t* dfa_next = nullptr;
    uint8_t* dfa_accept = nullptr;
    int dfa_n_states = 0;
    bool dfa_block_valid = false;  // the block's pointers are the current tables' (a decode call wrote it since)
    uint32_t* dec_states = nullptr;
    // xh_decode_sample_adapt (sample_adapt.h): parameter block, the typical stage's keys [vocab];
    // adapt_valid: a call has written the block (with adapt_constrain under the current constraint)
    xalm::AdaptCtl* adapt = nullptr;
    float* adapt_negd = nullptr;
    bool adapt_valid = false, adapt_constrain = false;
    // xh_decode_sample_seq (sample_seq.h): parameter block, the sorted breakers [XH_SEQ_MAX_BREAKERS];
    // seq_valid / seq_constrain as adapt_valid / adapt_constrain
    xalm::SeqCtl* seq = nullptr;
    int* seq_brk = nullptr;
    xalm::SeqTail* seq_tail = nullptr;  // written by every xh_decode_sample_seq call
    bool seq_valid = false, seq_constrain = false;
    int dec_cap = 0;
    // xh_set_top_logprobs (top_logprobs.h): the width on the host and in a device word the row
    // kernel reads, per-step top lists [dec_cap][XH_TOP_MAX] and ranks / log-probabilities of the
    // emitted tokens [dec_cap] (allocated by the first positive width), and the steps the last
    // decode call completed under the current width (-1: none yet)
    int top_n = 0;
    int* top_n_dev = nullptr;
    int* top_ids = nullptr;
    float* top_lps = nullptr;
    int* top_rank = nullptr;
    float* top_tlp = nullptr;
    int top_steps = -1;
    int nsplit = 1, t_max = 16;
    // fused attention + Wo launch (attn_wo.h): per-layer hand-off words [n_layers][4]
    bool fuse_attn_wo = true;
    unsigned* aw_sync = nullptr;
    // batched prefill (prefill.h), buffers allocated on first use
    bool prefill_batched = true;
    // XH_OPT_PREFILL: 1 = the LDS-tiled f16 MFMA GEMM (gemm16.h) for f16 / e4m3 / e5m2 weights (fp8
    // as an exact f16 image), f32 MFMA otherwise; 2 = split-f16 register-streaming MFMA wherever the
    // weights convert exactly; 3 = f32 MFMA only; 4 = as 1 with hipBLASLt in place of gemm16.h
    int prefill_gemm = 1;
    xalm::BlasState* blas = nullptr;             // XH_OPT_PREFILL 4, created on the first prompt that uses it
    uint16_t* pf_wdq = nullptr;                  // f16 image of one fp8 matrix for the f16 GEMMs (pf_prepare)
    size_t pf_wdq_elems = 0;
    bool pf_resid_norm = true;                   // residual + rmsnorm split in one launch (XH_OPT_PREFILL_GLU_SPLIT 0: off)
    bool pf_glu_split = true;                    // XH_OPT_PREFILL_GLU_SPLIT: fused GLU -> split input
    int pf_fa_split = 1;                         // XH_OPT_PREFILL_ATTN_SPLIT: history splits for short passes
    int pf_attn_mode = 1;                        // XH_OPT_PREFILL_ATTN: 1 shared-tile MFMA (v1 for head_dim != 128),
                                                 // 2 per-wave MFMA tiles, 0 per-token split kernel
    bool pf_ring = true;                         // XH_OPT_PREFILL_RING: ring passes at positions >= max_seq_len
    bool pf_attn_kv8 = false;                    // XH_OPT_PREFILL_ATTN_KV8: an fp8 KV ring follows pf_attn_mode too
    bool pf_ring_kv8 = false;                    // XH_OPT_PREFILL_RING_KV8: ... and runs ring passes (under pf_attn_kv8)
    xalm::PfBufs pf;                             // the pass buffers
    // xh_perplexity: targets and probabilities of the whole run (allocated on first use)
    int* ppl_tgt = nullptr;                      // [ppl_cap] targets (per-token path)
    float* ppl_prob = nullptr;                   // [ppl_cap]
    int ppl_cap = 0;
    int t_max_aw = 16;
    bool use_graphs = true;
    hipGraphExec_t g_step[xalm::N_STEP_KINDS] = {};  // the captured step of each kind (null: not captured yet)
    int max_gemv_waves = 4096;  // 16 waves per CU
    // the qkv launch: its whole matrix is one round at 16 waves per CU (every wave one group,
    // requested at once); at 8 waves per CU each wave streams two groups back to back
    // (tools/gemv_bench GB_T1K: 10.95 -> 10.12 us f16, 7.93 -> 7.34 us fp8)
    int qkv_waves = 2048;
    int n_cu = 0;
    // debug timelines (xh_debug_trace): device-clock stamps per workgroup
    unsigned long long* aw_trace = nullptr;
    size_t aw_trace_len = 0;
    bool aw_trace_on = false;   // attn_wo launches ([workgroup][8])
    bool w13_trace_on = false;  // plain W1/W3 launches ([workgroup][4]: tools/balance_trace.py)
    // the last layer's launches and the lm_head each write their own region (LT_*): the step's
    // timeline, kernel boundaries included (tools/layer_trace.py)
    bool layer_trace_on = false;
    // (typed as the fp16 ring; an fp8 ring's rows are kv_dim bytes: address it through kv_esz())
    uint16_t* kcache(int l) { return (uint16_t*)((char*)kv + (size_t)l * 2 * c.max_seq_len * kv_dim * kv_esz()); }
    uint16_t* vcache(int l) { return (uint16_t*)((char*)kcache(l) + (size_t)c.max_seq_len * kv_dim * kv_esz()); }
};

namespace xalm {

// xalm_hip.hip: the message goes to ctx, or to the creating thread when there is none
int set_err(xh_ctx* ctx, int code, const char* fmt, ...);

#define HIP_TRY(ctx, expr)                                                                     \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess)                                                                  \
            return xalm::set_err((ctx), XH_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                                 __FILE__, __LINE__);                                          \
    } while (0)

// Host <-> device copies and fills go on ctx->stream and wait for it.  ctx->stream is
// non-blocking, so null-stream work (hipMemcpy, hipMemset, hipMemcpy2D) is not ordered with
// its kernels: a fill can land after a kernel wrote the buffer, and a pageable upload can
// return before its DMA does.
inline hipError_t copy_sync(xh_ctx* ctx, void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    const hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, ctx->stream);
    return e != hipSuccess ? e : hipStreamSynchronize(ctx->stream);
}
inline hipError_t copy2d_sync(xh_ctx* ctx, void* dst, size_t dpitch, const void* src, size_t spitch, size_t width,
                              size_t height) {
    const hipError_t e = hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, hipMemcpyHostToDevice, ctx->stream);
    return e != hipSuccess ? e : hipStreamSynchronize(ctx->stream);
}
inline hipError_t fill_sync(xh_ctx* ctx, void* dst, int value, size_t bytes) {
    const hipError_t e = hipMemsetAsync(dst, value, bytes, ctx->stream);
    return e != hipSuccess ? e : hipStreamSynchronize(ctx->stream);
}
template <typename T>
int dmalloc(xh_ctx* ctx, T** p, size_t n) {
    HIP_TRY(ctx, hipMalloc((void**)p, n ? n * sizeof(T) : 16));
    HIP_TRY(ctx, fill_sync(ctx, *p, 0, n ? n * sizeof(T) : 16));
    return 0;
}

// debug layer timeline: regions of aw_trace (words) per launch of the traced (last) layer
constexpr size_t LT_QKV = 0, LT_AW = 8192, LT_W13 = 16384, LT_W2 = 20480, LT_CLS = 24576, LT_WORDS = 28672;

// launch.hip: the only unit that instantiates gemv_kernel and attn_split_kernel.  A role is one
// (prologue, epilogue) pair of gemv.h; false = no instantiation for the dtype / head shape.
// GEMV_QKV8: GEMV_QKV writing an fp8 KV ring (EPI_QKV8).
enum GemvRole { GEMV_QKV, GEMV_GLU, GEMV_RESID, GEMV_LOGITS, GEMV_STORE, GEMV_QKV8 };
inline GemvRole qkv_role(const xh_ctx* ctx) { return ctx->kv8() ? GEMV_QKV8 : GEMV_QKV; }
bool launch_gemv(GemvRole role, int dt, const GemvArgs& a, hipStream_t s, int max_waves);
// the shape launch_gemv takes for (role, dt) at input length n (xh_gemv_shape), -1 = none
int gemv_shape(int role, int dt, int n);
// kv_dt: the rings' element type behind a.kc / a.vc (XH_F16, XH_F8_E4M3)
bool launch_attn(const AttnArgs& a, int hd, int qpk, int n_kv_heads, int t_max, hipStream_t s, int kv_dt = XH_F16);
int attn_nsplit(int n_kv_heads, int max_seq_len);
// The dynamic-LDS limit of a kernel above 64 KiB (up to the CU's 160 KiB), set once per (kernel,
// device); false when it could not be set.
bool ensure_lds(const void* fn, int bytes = 160 * 1024);

// Runtime value -> template argument, for the units that instantiate kernels.  for_dt: f.run<DT>()
// for a weight dtype; for_qpk: f(std::integral_constant<int, QPK>) for the q heads per KV head.
// -1: no instantiation for the value (f returns >= 0).
template <class F>
int for_dt(int dt, const F& f) {
    switch (dt) {
        case XH_F32: return f.template run<XH_F32>();
        case XH_F16: return f.template run<XH_F16>();
        case XH_BF16: return f.template run<XH_BF16>();
        case XH_F8_E4M3: return f.template run<XH_F8_E4M3>();
        case XH_F8_E5M2: return f.template run<XH_F8_E5M2>();
        case XH_Q8: return f.template run<XH_Q8>();
        case XH_F8_E4M3_EXACT: return f.template run<XH_F8_E4M3_EXACT>();
        case XH_F8_E5M2_EXACT: return f.template run<XH_F8_E5M2_EXACT>();
        case XH_Q8_0: return f.template run<XH_Q8_0>();
        case XH_Q4_0: return f.template run<XH_Q4_0>();
        case XH_Q4_1: return f.template run<XH_Q4_1>();
        case XH_Q5_0: return f.template run<XH_Q5_0>();
        case XH_Q5_1: return f.template run<XH_Q5_1>();
        case XH_MXFP4: return f.template run<XH_MXFP4>();
        case XH_Q4_K: return f.template run<XH_Q4_K>();
        case XH_Q6_K: return f.template run<XH_Q6_K>();
        default: return -1;
    }
}
template <class F>
int for_qpk(int qpk, const F& f) {
    switch (qpk) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 4: return f(std::integral_constant<int, 4>{});
        case 8: return f(std::integral_constant<int, 8>{});
        default: return -1;
    }
}

// decode.hip
GemvArgs qkv_args(xh_ctx* ctx, int l);
GemvArgs wo_args(xh_ctx* ctx, int l);
GemvArgs w13_args(xh_ctx* ctx, int l);
GemvArgs w2_args(xh_ctx* ctx, int l);
GemvArgs cls_args(xh_ctx* ctx);
AttnArgs attn_args(xh_ctx* ctx, int l);
int qkv_launch_waves(const xh_ctx* ctx, int l);
int check_ready(xh_ctx* ctx);
int check_aw(xh_ctx* ctx);
void drop_graphs(xh_ctx* ctx);
int host_step_params(xh_ctx* ctx, int token, int pos);
int run_step(xh_ctx* ctx, bool with_logits);
void time_head(xh_ctx* ctx, StepKind head);  // one launch of the head's kernel on ctx->stream (xh_time_kernel 6 .. 8, 10, 11)
// top_logprobs_kernel (top_logprobs.h; defined in decode.hip) over n_rows rows on stream s: the
// kernel's arguments in its order
void launch_top_logprobs(const float* logits, int vocab, size_t stride, int n_rows, const int* n_top_dev, int n_top,
                         const StepParams* sp, int cap, const int* targets, int out_stride, int* ids, float* lps,
                         float* target_lp, int* target_rank, hipStream_t s);
void time_top_logprobs(xh_ctx* ctx);  // one row-kernel launch on ctx->logits (xh_time_kernel 9)

// prefill.hip: the pass buffers, and gemm16.h for xh_op_prompt_gemm (device pointers).  mm_op_ks:
// *ks = 0 picks the K slicing; 0, 1 when K is no multiple of MM_KMULT, 2 when *ks slices do not divide it
void pf_free(xh_ctx* ctx);
int mm_op_ks(int rows, int K, int n, int* ks);
void mm_op_launch(const uint16_t* w, const uint16_t* xh, const uint16_t* xl, float* out, int rows, int K, int n, int ks,
                  int n_cu);
// prefill.hip: the prompt attention's launch bodies on device pointers, shared by the passes and
// by xh_op_prompt_attn / xh_op_prompt_attn_ring.  -1: no instantiation for the head shape.
struct PfAttnDims { int head_dim, n_heads, n_kv_heads; };
// floats of the split partials of n rows: O [nsplit][n][q_dim], then (m, l) [nsplit][n][n_heads]
inline size_t pf_fa_part_floats(const PfAttnDims& d, int nsplit, int n) {
    return (size_t)nsplit * n * ((size_t)d.n_heads * d.head_dim + 2 * d.n_heads);
}
bool pf_attn_shape_ok(int hd, int qpk);
// history splits: the most a walk over pos0 slots may take, and the passes' choice for n rows at
// n_cu CUs within part_floats of partials
int pf_fa_split_max(int pos0);
int pf_fa_pick_nsplit(const PfAttnDims& d, int n_cu, int n, int pos0, size_t part_floats);
// causal rows [pos0, pos0 + n) over kc / vc of element type kv_dt (XH_F16; XH_F8_E4M3: one code per
// element); shared: the shared-tile kernel (head_dim 128) over nsplit >= 1 splits, part
// (pf_fa_part_floats) when nsplit > 1; else the per-wave kernel
int pf_fa_launch(const PfAttnDims& d, int kv_dt, bool shared, const float* q, const uint16_t* kc, const uint16_t* vc,
                 float* out, int n, int pos0, int nsplit, float* part, hipStream_t s);
// a ring pass's walk, merge with the sinks (sinkv [m][2][kv_dim]) and commit; part always.  kv_dt: the
// element type behind kc / vc / ks / vs / sinkv (XH_F8_E4M3: one code each); an fp8 commit also moves
// the last master version sinkm [2][kv_dim] (fp16) to `master` when there is one (null: neither)
int pf_ring_launch(const PfAttnDims& d, int kv_dt, const float* q, uint16_t* kc, uint16_t* vc, const uint16_t* ks,
                   const uint16_t* vs, const uint16_t* sinkv, float* out, int m, int p0, int max_seq_len, int nsplit,
                   float* part, hipStream_t s, const uint16_t* sinkm = nullptr, uint16_t* master = nullptr);

// prefill.hip: the prompt GEMM's launch bodies on device pointers, shared by the passes (pf_gemm) and
// by xh_op_prompt_matmul / xh_op_prompt_weight_image / xh_op_prompt_stage.  Nothing here reads a context.
// One GEMM Y[n][rows] = X[n][K] . W[rows][K]^T of decode form dt under XH_OPT_PREFILL `mode` (blas: mode 4
// with a hipBLASLt plan for every shape of the model).  wide: an MXFP4 matrix with no f16 image.
// ks 0: the route's own K slicing, else that many slices (pf_gemm_ks_ok).  max_groups 0: the image
// kernels' cap of PF_IMAGE_GROUPS workgroups.
constexpr int PF_IMAGE_GROUPS = 8192;
struct PfGemmPlan {
    int mode; bool blas;
    int dt, K, rows; bool wide;
    int n, n_cu;
    size_t part_floats;  // capacity of `part`
    int ks, max_groups;
};
struct PfGemmIo {
    const void* w;        // device rows of dt
    const float* x;       // [n][K] (the f32-input route reads it; the others their split halves)
    uint16_t *xh, *xl;    // split halves: row-major hi rows then lo rows in xh (route 0), fragments in xh / xl (E > 0)
    float* xs;            // [n] 1 / row scale
    uint16_t* wdq;        // f16 image(s) of w (route 0), wdq_elems f16
    size_t wdq_elems;
    float* part;          // [ks][n][rows]
};
enum { PF_GEMM_OK = 0, PF_GEMM_E_IMAGE = -1, PF_GEMM_E_FIT = -2, PF_GEMM_E_SHAPE = -3, PF_GEMM_E_DTYPE = -4 };
// weights per 16-byte chunk of the f32-input kernel's decoder of dt (WDec<DT>::E)
int pf_elems(int dt);
// the route: 0 = row-major split input (gemm16.h or hipBLASLt), E > 0 = the fragment kernel, -1 = f32 input
int pf_gemm_route(const PfGemmPlan& p);
// rows per wave (routes -1 and E > 0) or per workgroup (route 0): the launch's row tile
int pf_gemm_row_tile(int route);
// may the GEMM of p run in p.ks > 0 slices on `route`: the divisibility and capacity rules of its picker
bool pf_gemm_ks_ok(const PfGemmPlan& p, int route);
// the split halves of x [n][K] in layout lay (0 or E): hi, lo and 1 / s_t
void pf_split_launch(const float* x, int K, int n, int lay, uint16_t* xh, uint16_t* xl, float* inv_s, hipStream_t s);
uint16_t* pf_split_lo(int lay, int n, int K, uint16_t* xh, uint16_t* xl);  // where lay's lo halves go
size_t pf_split_index(int t, int k, int K, int lay);                      // split_off on the host
// route 0: the f16 image(s) of w into io.wdq (none for f16: *w_hi = io.w); *w_lo: the gguf blocks' lo image
int pf_gemm_images(const PfGemmPlan& p, const PfGemmIo& io, const uint16_t** w_hi, const uint16_t** w_lo, hipStream_t s);
// route 0 on gemm16.h over w_hi (and w_lo into partials [ks, 2 ks)); *ks_out = slices the epilogue sums
int pf_gemm_rowmajor(const PfGemmPlan& p, const PfGemmIo& io, const uint16_t* w_hi, const uint16_t* w_lo, int* ks_out,
                     hipStream_t s);
int pf_gemm_frag(const PfGemmPlan& p, const PfGemmIo& io, int lay, int* ks_out, hipStream_t s);
int pf_gemm_f32(const PfGemmPlan& p, const PfGemmIo& io, int* ks_out, hipStream_t s);
// the producers and the epilogue (prefill.h) on plain arguments
void pf_norm_split_launch(const float* x, int dim, const void* nw, int ndt, float eps, int n, int lay, uint16_t* xh,
                          uint16_t* xl, float* inv_s, hipStream_t s);
void pf_norm_launch(const float* x, int dim, const void* nw, int ndt, float eps, int n, float* o, hipStream_t s);
void pf_resid_norm_split_launch(const float* part, int ks, const float* part_s, float* x, int dim, const void* nw, int ndt,
                                float eps, int n, int lay, uint16_t* xh, uint16_t* xl, float* inv_s, hipStream_t s);
void pf_glu_split_launch(const float* part, int ks, const float* part_s, int n, int hidden, int act, int lay, uint16_t* xh,
                         uint16_t* xl, float* inv_s, hipStream_t s);
// prefill_epi_kernel with EPI_STORE / EPI_RESID / EPI_GLU (no K/V arguments)
void pf_epi_plain_launch(const float* part, const float* part_s, int ks, int n, int rows, int epi, float* out,
                         size_t out_stride, int act, hipStream_t s);

// prefill_blas.hip (XH_OPT_PREFILL 4).  blas_ok: 0 unprobed, 1 every GEMM shape of the model has
// an f16 plan, -1 not.  blas_has_plan: *have = hipBLASLt has an algorithm for the shape.
int blas_ok(const xh_ctx* ctx);
void blas_set_ok(xh_ctx* ctx, int ok);
int blas_has_plan(xh_ctx* ctx, int rows, int K, int n, bool* have);
int blas_gemm(xh_ctx* ctx, const void* w, int K, int rows, const uint16_t* x, int n, float* y);
void blas_free(xh_ctx* ctx);

// upload.hip
void gq_repack(int dt, const uint8_t* src, size_t rows, size_t cols, uint8_t* dst);
// MXFP4 blocks in the file layout: the least and greatest scale byte (lo > hi: no block)
void mx_e_range(const uint8_t* src, size_t n_blocks, uint8_t* lo, uint8_t* hi);

}  // namespace xalm
