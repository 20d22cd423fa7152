// decode.hip — the per-token step: its kernels, argument builders, the fused attention + Wo launch,
// and one graph per StepKind (ctx.h), captured on first use and replayed.  The decode ABI entries
// (xh_decode_greedy, xh_decode_sample, _ext, _dfa, _adapt, _seq) fill a DecodeCall and run the one
// driver, decode_run; the xh_op_sample* entries share their argument checks, device staging and
// copy-back.  Also here: xh_forward, xh_get_logits, the constraint and top-logprobs entries.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <vector>

#include "constraint.h"
#include "ctx.h"
#include "dt_launch.h"
#include "sample.h"
#include "sample_adapt.h"
#include "sample_seq.h"
#include "sample_dfa.h"
#include "sample_ext.h"
#include "top_logprobs.h"
#include "top_logprobs_host.h"

using namespace xalm;

// The step's own kernels.  Non-template kernels are defined in one translation unit: this one.
namespace xalm {

// Model::_copy_embedding (src/infer.cpp:553-602): x = dec(embed[token, :])
__global__ void embed_kernel(const void* emb, int dtype, int dim, float* x, const StepParams* sp,
                             const float* rope_freq, float* rope_cs, int half) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < dim) x[i] = dec_row(dtype, emb, (size_t)sp->token, dim, i);
    if (blockIdx.x == 0) rope_table(rope_cs, rope_freq, half, sp->pos, threadIdx.x);
}

// Greedy decode step head: argmax over the lm_head workgroups' candidates (Sampler::
// sample_argmax, src/sampler.cpp:19-30: the first maximum among logits > FLT_MIN, else token
// 0), the decode-loop bookkeeping of argmax_advance (tokens[step], step, token, positions,
// src/infer.cpp:611-613) and x = embed[token] (Model::_copy_embedding,
// src/infer.cpp:553-602), in one 1024-thread workgroup.
__global__ __launch_bounds__(1024) void argmax_embed_kernel(const unsigned long long* cand, StepParams* sp,
                                                            int* tokens, int cap, const void* emb, int dtype,
                                                            int dim, float* x, const float* rope_freq,
                                                            float* rope_cs, int half) {
    __shared__ unsigned long long kb[16];
    __shared__ int tok_s, pos_s;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    unsigned long long best = cand[tid];  // ARGMAX_CANDS == blockDim.x
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(best, o, 64);
        best = other > best ? other : best;
    }
    if (lane == 0) kb[wid] = best;
    __syncthreads();
    if (tid == 0) {
        unsigned long long bb = 0;
#pragma unroll
        for (int w = 0; w < 16; w++) bb = kb[w] > bb ? kb[w] : bb;
        const int tok = argmax_key_index(bb);
        if (sp->step < cap) tokens[sp->step] = tok;
        sp->step += 1;
        sp->token = tok;
        step_positions(sp, sp->pos_next);
        sp->pos_next += 1;
        tok_s = tok;
        pos_s = sp->pos;
    }
    __syncthreads();
    rope_table(rope_cs, rope_freq, half, pos_s, tid);
    for (int i = tid; i < dim; i += 1024) x[i] = dec_row(dtype, emb, (size_t)tok_s, dim, i);
}

// Sampled decode step head: the token is drawn from the logits of the previous step
// (sample_token, sample.h; the definition is in include/xalm_hip.h) at counter sp->pos_next, the
// position it will occupy; then the bookkeeping and the embedding exactly as argmax_embed_kernel.
__global__ __launch_bounds__(SMP_THREADS) void sample_embed_kernel(const float* logits, int vocab,
                                                                   const xh_sampling* samp, StepParams* sp, int* tokens,
                                                                   int cap, const void* emb, int dtype, int dim, float* x,
                                                                   const float* rope_freq, float* rope_cs, int half) {
    __shared__ SampleShared sh;
    __shared__ int pos_s;
    const int tid = threadIdx.x;
    int n_kept;
    const int tok = sample_token(sh, logits, vocab, *samp, (uint32_t)sp->pos_next, &n_kept);
    __syncthreads();  // every thread has read pos_next
    if (tid == 0) {
        if (sp->step < cap) tokens[sp->step] = tok;
        sp->step += 1;
        sp->token = tok;
        step_positions(sp, sp->pos_next);
        sp->pos_next += 1;
        pos_s = sp->pos;
    }
    __syncthreads();
    rope_table(rope_cs, rope_freq, half, pos_s, tid);
    for (int i = tid; i < dim; i += SMP_THREADS) x[i] = dec_row(dtype, emb, (size_t)tok, dim, i);
}

// xh_op_sample: workgroup d draws at counter pos0 + d
__global__ __launch_bounds__(SMP_THREADS) void sample_op_kernel(const float* logits, int vocab, const xh_sampling* samp,
                                                                uint32_t pos0, int* tokens, int* n_kept_out) {
    __shared__ SampleShared sh;
    int n_kept;
    const int tok = sample_token(sh, logits, vocab, *samp, pos0 + blockIdx.x, &n_kept);
    if (threadIdx.x == 0) {
        tokens[blockIdx.x] = tok;
        n_kept_out[blockIdx.x] = n_kept;
    }
}

// Extended sampled decode step head (xh_decode_sample_ext): the adjusted logits l' go to `adj`
// (ext_prepare, sample_ext.h; `logits` stay raw), the token is drawn from them by sample_token
// under the effective top-k, its log-probability comes from the raw logits, the token joins the
// window ring, and then the bookkeeping and the embedding exactly as sample_embed_kernel.
__global__ __launch_bounds__(SMP_THREADS) void sample_ext_embed_kernel(
    const float* logits, int vocab, ExtCtl* ctl, int* ring, const int* btok, const float* bval, float* adj,
    StepParams* sp, int* tokens, float* logprobs, int cap, const void* emb, int dtype, int dim, float* x,
    const float* rope_freq, float* rope_cs, int half) {
    __shared__ SampleShared sh;
    __shared__ ExtShared es;
    __shared__ int pos_s;
    const int tid = threadIdx.x;
    const ExtCtl c = *ctl;
    const ExtPrep pr = ext_prepare(es, logits, adj, vocab, c, ring, btok, bval);
    xh_sampling p = c.samp;
    p.top_k = pr.top_k;
    int n_kept;
    const int tok = sample_token(sh, adj, vocab, p, (uint32_t)sp->pos_next, &n_kept);
    __syncthreads();  // every thread has read pos_next, the block and the ring
    if (tid == 0) {
        if (sp->step < cap) {
            tokens[sp->step] = tok;
            logprobs[sp->step] = (logits[tok] - pr.M) - pr.lse;
        }
        ring[c.count & (EXT_RING - 1)] = tok;
        ctl->count = c.count + 1;
        sp->step += 1;
        sp->token = tok;
        step_positions(sp, sp->pos_next);
        sp->pos_next += 1;
        pos_s = sp->pos;
    }
    __syncthreads();
    rope_table(rope_cs, rope_freq, half, pos_s, tid);
    for (int i = tid; i < dim; i += SMP_THREADS) x[i] = dec_row(dtype, emb, (size_t)tok, dim, i);
}

// xh_op_sample_ext: one workgroup prepares l' and the scalars of the draw ...
__global__ __launch_bounds__(SMP_THREADS) void sample_ext_prep_kernel(const float* logits, int vocab, const ExtCtl* ctl,
                                                                      const int* ring, const int* btok,
                                                                      const float* bval, float* adj, ExtPrep* prep) {
    __shared__ ExtShared es;
    const ExtPrep pr = ext_prepare(es, logits, adj, vocab, *ctl, ring, btok, bval);
    if (threadIdx.x == 0) *prep = pr;
}
// ... and workgroup d draws at counter pos0 + d from l'
__global__ __launch_bounds__(SMP_THREADS) void sample_ext_op_kernel(const float* logits, const float* adj, int vocab,
                                                                    const ExtCtl* ctl, const ExtPrep* prep,
                                                                    uint32_t pos0, int* tokens, int* n_kept_out,
                                                                    float* logprobs) {
    __shared__ SampleShared sh;
    const ExtPrep pr = *prep;
    xh_sampling p = ctl->samp;
    p.top_k = pr.top_k;
    int n_kept;
    const int tok = sample_token(sh, adj, vocab, p, pos0 + blockIdx.x, &n_kept);
    if (threadIdx.x == 0) {
        tokens[blockIdx.x] = tok;
        n_kept_out[blockIdx.x] = n_kept;
        logprobs[blockIdx.x] = (logits[tok] - pr.M) - pr.lse;
    }
}

// Constrained sampled decode step head (xh_decode_sample_dfa): sample_ext_embed_kernel's work with
// the byte-DFA mask written over l' before anything is computed from it (DfaMask, sample_dfa.h), the
// draw of dfa_draw, and the successor state stored in the block and in the per-step log.
__global__ __launch_bounds__(SMP_THREADS) void sample_dfa_embed_kernel(
    const float* logits, int vocab, ExtCtl* ctl, DfaCtl* dfa, int* ring, const int* btok, const float* bval, float* adj,
    StepParams* sp, int* tokens, float* logprobs, uint32_t* states, int cap, const void* emb, int dtype, int dim,
    float* x, const float* rope_freq, float* rope_cs, int half) {
    __shared__ SampleShared sh;
    __shared__ ExtShared es;
    __shared__ DfaShared ds;
    __shared__ int pos_s;
    const int tid = threadIdx.x;
    const ExtCtl c = *ctl;
    const DfaCtl d = *dfa;
    const ExtPrep pr = ext_prepare(es, logits, adj, vocab, c, ring, btok, bval, DfaMask{&ds, d});
    const DfaDraw dr = dfa_draw(sh, ds, adj, vocab, c, pr, d, (uint32_t)sp->pos_next);
    const int tok = dr.token;
    __syncthreads();  // every thread has read pos_next, the blocks and the ring
    if (tid == 0) {
        if (sp->step < cap) {
            tokens[sp->step] = tok;
            logprobs[sp->step] = (logits[tok] - pr.M) - pr.lse;
            states[sp->step] = dr.state;
        }
        dfa->state = dr.state;
        ring[c.count & (EXT_RING - 1)] = tok;
        ctl->count = c.count + 1;
        sp->step += 1;
        sp->token = tok;
        step_positions(sp, sp->pos_next);
        sp->pos_next += 1;
        pos_s = sp->pos;
    }
    __syncthreads();
    rope_table(rope_cs, rope_freq, half, pos_s, tid);
    for (int i = tid; i < dim; i += SMP_THREADS) x[i] = dec_row(dtype, emb, (size_t)tok, dim, i);
}

// xh_op_sample_dfa: one workgroup prepares the masked l', the scalars of the draw, the allowed count
// and the constrained greedy key ...
struct DfaPrep {
    ExtPrep ext;
    unsigned long long best;
    unsigned n_allowed;
};
__global__ __launch_bounds__(SMP_THREADS) void sample_dfa_prep_kernel(const float* logits, int vocab, const ExtCtl* ctl,
                                                                      const DfaCtl* dfa, const int* ring, const int* btok,
                                                                      const float* bval, float* adj, DfaPrep* prep) {
    __shared__ ExtShared es;
    __shared__ DfaShared ds;
    const DfaCtl d = *dfa;
    const ExtPrep pr = ext_prepare(es, logits, adj, vocab, *ctl, ring, btok, bval, DfaMask{&ds, d});
    if (threadIdx.x == 0) {
        prep->ext = pr;
        prep->best = d.state == XH_DFA_DEAD ? 0ull : ds.best;
        prep->n_allowed = d.state == XH_DFA_DEAD ? 0u : ds.n_allowed;
    }
}
// ... and workgroup i draws at counter pos0 + i from it, every draw from the same state
__global__ __launch_bounds__(SMP_THREADS) void sample_dfa_op_kernel(const float* logits, const float* adj, int vocab,
                                                                    const ExtCtl* ctl, const DfaCtl* dfa,
                                                                    const DfaPrep* prep, uint32_t pos0, int* tokens,
                                                                    int* n_kept_out, uint32_t* states, float* logprobs) {
    __shared__ SampleShared sh;
    __shared__ DfaShared ds;
    const DfaPrep pp = *prep;
    if (threadIdx.x == 0) {
        ds.best = pp.best;
        ds.n_allowed = pp.n_allowed;
    }
    __syncthreads();
    const DfaDraw dr = dfa_draw(sh, ds, adj, vocab, *ctl, pp.ext, *dfa, pos0 + blockIdx.x);
    if (threadIdx.x == 0) {
        tokens[blockIdx.x] = dr.token;
        n_kept_out[blockIdx.x] = dr.n_kept;
        states[blockIdx.x] = dr.state;
        logprobs[blockIdx.x] = (logits[dr.token] - pp.ext.M) - pp.ext.lse;
    }
}

// Candidates from logits already on the device (the first greedy step after logits that no
// EPI_LOGITS launch produced): cand[0] = best key, the rest 0.
__global__ __launch_bounds__(1024) void logits_cand_kernel(const float* logits, int vocab, unsigned long long* cand) {
    __shared__ unsigned long long kb[16];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    unsigned long long best = 0;
    for (int i = tid; i < vocab; i += 1024) {
        const float v = logits[i];
        if (v > FLT_MIN) {
            const unsigned long long k = argmax_key(v, i);
            best = k > best ? k : best;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(best, o, 64);
        best = other > best ? other : best;
    }
    if (lane == 0) kb[wid] = best;
    __syncthreads();
    unsigned long long bb = 0;
#pragma unroll
    for (int w = 0; w < 16; w++) bb = kb[w] > bb ? kb[w] : bb;
    cand[tid] = tid == 0 ? bb : 0ull;
}

}  // namespace xalm

namespace {

// ---------------------------------------------------------------------------------------
// the per-token step, enqueued on a stream (eager or under graph capture)
// ---------------------------------------------------------------------------------------
bool layer_traced(const xh_ctx* ctx, int l) { return ctx->layer_trace_on && l == ctx->c.n_layers - 1; }

bool use_attn_wo(const xh_ctx* ctx, int l) {
    const int dt = ctx->L[l].wo_dt;
    if (ctx->L[l].wo_x) return false;  // exact fp8 decode: the separate launches
    if (ctx->kv8()) return false;      // fp8 KV ring: attn_wo.h has no instantiation for it
    return ctx->fuse_attn_wo && aw_instantiated(ctx->c.head_dim, ctx->qpk) &&
           (dt == XH_F32 || dt == XH_F16 || dt == XH_BF16 || dt == XH_F8_E4M3 || dt == XH_F8_E5M2 || dt == XH_Q8);
}

int launch_attn_wo(xh_ctx* ctx, int l, hipStream_t s) {
    const AttnArgs aa = attn_args(ctx, l);
    const GemvArgs ga = wo_args(ctx, l);
    unsigned* sync = ctx->aw_sync + (size_t)AW_SYNC_WORDS * l;
    const int hd = ctx->c.head_dim, qpk = ctx->qpk, nkv = ctx->c.n_kv_heads, tm = ctx->t_max_aw;
    const int mw = ctx->max_gemv_waves;
    unsigned long long* tr = ctx->aw_trace_on ? ctx->aw_trace : layer_traced(ctx, l) ? ctx->aw_trace + LT_AW : nullptr;
    switch (ctx->L[l].wo_dt) {
        case XH_F32: return aw_launch_dt1(aa, ga, hd, qpk, nkv, tm, sync, mw, s, tr);
        case XH_F16: return aw_launch_dt2(aa, ga, hd, qpk, nkv, tm, sync, mw, s, tr);
        case XH_BF16: return aw_launch_dt3(aa, ga, hd, qpk, nkv, tm, sync, mw, s, tr);
        case XH_F8_E4M3: return aw_launch_dt6(aa, ga, hd, qpk, nkv, tm, sync, mw, s, tr);
        case XH_F8_E5M2: return aw_launch_dt7(aa, ga, hd, qpk, nkv, tm, sync, mw, s, tr);
        case XH_Q8: return aw_launch_dt9(aa, ga, hd, qpk, nkv, tm, sync, mw, s, tr);
        default: return XH_E_INVALID;
    }
}

// The head of a step of `kind` (StepKind, ctx.h), the launch that puts the step's token, positions and
// x = embed[token] in place:
//   STEP_LOGITS, STEP_HYDRATE  the token host_step_params gave (embed_kernel)
//   STEP_GREEDY                the argmax of the previous step's logits (argmax_embed_kernel)
//   STEP_SAMPLE                drawn from them under ctx->samp (sample_embed_kernel)
//   STEP_SAMPLE_EXT            drawn from their adjusted copy under ctx->ext (sample_ext_embed_kernel)
//   STEP_SAMPLE_DFA            ... adjusted and masked under ctx->ext and ctx->dfa (sample_dfa_embed_kernel)
//   STEP_SAMPLE_ADAPT          the same under ctx->adapt's truncation stages (sample_adapt_embed_kernel)
//   STEP_SAMPLE_SEQ            the same with ctx->seq's sequence stage and XTC (sample_seq_embed_kernel)
void launch_head(xh_ctx* ctx, StepKind kind, hipStream_t s) {
    const xh_config& c = ctx->c;
    const float* logits = ctx->logits;
    const void* emb = ctx->embed;
    const float* rope_freq = ctx->rope_freq;
    const int* btok = ctx->ext_btok;
    const float* bval = ctx->ext_bval;
    const int half = c.head_dim / 2;
    switch (kind) {
        case STEP_LOGITS:
        case STEP_HYDRATE:
            hipLaunchKernelGGL(embed_kernel, dim3((c.dim + 255) / 256), dim3(256), 0, s, emb, ctx->embed_dt, c.dim, ctx->x,
                               (const StepParams*)ctx->sp, rope_freq, ctx->rope_cs, half);
            break;
        case STEP_GREEDY:
            hipLaunchKernelGGL(argmax_embed_kernel, dim3(1), dim3(ARGMAX_CANDS), 0, s, (const unsigned long long*)ctx->cand,
                               ctx->sp, ctx->dec_tokens, ctx->dec_cap, emb, ctx->embed_dt, c.dim, ctx->x, rope_freq,
                               ctx->rope_cs, half);
            break;
        case STEP_SAMPLE:
            hipLaunchKernelGGL(sample_embed_kernel, dim3(1), dim3(SMP_THREADS), 0, s, logits, c.vocab_size,
                               (const xh_sampling*)ctx->samp, ctx->sp, ctx->dec_tokens, ctx->dec_cap, emb, ctx->embed_dt,
                               c.dim, ctx->x, rope_freq, ctx->rope_cs, half);
            break;
        case STEP_SAMPLE_EXT:
            hipLaunchKernelGGL(sample_ext_embed_kernel, dim3(1), dim3(SMP_THREADS), 0, s, logits, c.vocab_size, ctx->ext,
                               ctx->ext_ring, btok, bval, ctx->ext_adj, ctx->sp, ctx->dec_tokens, ctx->dec_logprobs,
                               ctx->dec_cap, emb, ctx->embed_dt, c.dim, ctx->x, rope_freq, ctx->rope_cs, half);
            break;
        case STEP_SAMPLE_DFA:
            hipLaunchKernelGGL(sample_dfa_embed_kernel, dim3(1), dim3(SMP_THREADS), 0, s, logits, c.vocab_size, ctx->ext,
                               ctx->dfa, ctx->ext_ring, btok, bval, ctx->ext_adj, ctx->sp, ctx->dec_tokens,
                               ctx->dec_logprobs, ctx->dec_states, ctx->dec_cap, emb, ctx->embed_dt, c.dim, ctx->x,
                               rope_freq, ctx->rope_cs, half);
            break;
        case STEP_SAMPLE_ADAPT:
            hipLaunchKernelGGL(sample_adapt_embed_kernel, dim3(1), dim3(SMP_THREADS), 0, s, logits, c.vocab_size, ctx->ext,
                               ctx->dfa, ctx->adapt, ctx->ext_ring, btok, bval, ctx->ext_adj, ctx->adapt_negd, ctx->sp,
                               ctx->dec_tokens, ctx->dec_logprobs, ctx->dec_states, ctx->dec_cap, emb, ctx->embed_dt, c.dim,
                               ctx->x, rope_freq, ctx->rope_cs, half);
            break;
        case STEP_SAMPLE_SEQ:
            hipLaunchKernelGGL(sample_seq_embed_kernel, dim3(1), dim3(SMP_THREADS), 0, s, logits, c.vocab_size, ctx->ext,
                               ctx->dfa, ctx->adapt, (const SeqCtl*)ctx->seq, ctx->ext_ring, btok, bval,
                               (const int*)ctx->seq_brk, ctx->ext_adj, ctx->adapt_negd, ctx->sp,
                               (const SeqTail*)ctx->seq_tail);
            break;
        case N_STEP_KINDS: break;
    }
}

// one step of `kind`: its head, the layers, and the lm_head unless the step only hydrates the KV ring
int enqueue_step(xh_ctx* ctx, hipStream_t s, StepKind kind) {
    const xh_config& c = ctx->c;
    const int mb = ctx->max_gemv_waves;
    launch_head(ctx, kind, s);
    // xh_set_top_logprobs: the row kernel on the raw logits a decode head chose from (the lm_head at
    // the end of this step is their next writer), as row sp->step - 1 with the head's token as target
    if (kind >= STEP_GREEDY && ctx->top_n > 0)
        launch_top_logprobs(ctx->logits, c.vocab_size, 0, 1, ctx->top_n_dev, 0, ctx->sp, ctx->dec_cap, ctx->dec_tokens,
                            XH_TOP_MAX, ctx->top_ids, ctx->top_lps, ctx->top_tlp, ctx->top_rank, s);
    for (int l = 0; l < c.n_layers; l++) {
        const LayerW& w = ctx->L[l];
        if (!launch_gemv(qkv_role(ctx), kdt(w.qkv_dt, w.qkv_x), qkv_args(ctx, l), s, qkv_launch_waves(ctx, l)))
            return set_err(ctx, XH_E_INVALID, "layer %d: unsupported qkv dtype %d", l, w.qkv_dt);
        GemvArgs a13 = w13_args(ctx, l);
        if (use_attn_wo(ctx, l)) {
            const int rc = launch_attn_wo(ctx, l, s);
            if (rc) return set_err(ctx, rc, "layer %d: fused attention + Wo launch failed", l);
            // W1/W3 right behind it zeroes its hand-off words for the next step
            a13.aw_reset = ctx->aw_sync + (size_t)AW_SYNC_WORDS * l;
        } else {
            if (!launch_attn(attn_args(ctx, l), c.head_dim, ctx->qpk, c.n_kv_heads, ctx->t_max, s, ctx->kv_dt))
                return set_err(ctx, XH_E_INVALID, "unsupported head_dim %d / q-per-kv %d", c.head_dim, ctx->qpk);
            if (!launch_gemv(GEMV_RESID, kdt(w.wo_dt, w.wo_x), wo_args(ctx, l), s, mb))
                return set_err(ctx, XH_E_INVALID, "layer %d: unsupported wo dtype", l);
        }
        if (!launch_gemv(GEMV_GLU, kdt(w.w13_dt, w.w13_x), a13, s, mb))
            return set_err(ctx, XH_E_INVALID, "layer %d: unsupported w1/w3 dtype", l);
        if (!launch_gemv(GEMV_RESID, kdt(w.w2_dt, w.w2_x), w2_args(ctx, l), s, mb))
            return set_err(ctx, XH_E_INVALID, "layer %d: unsupported w2 dtype", l);
    }
    if (kind != STEP_HYDRATE) {
        if (!launch_gemv(GEMV_LOGITS, kdt(ctx->wcls_dt, ctx->wcls_x), cls_args(ctx), s, mb))
            return set_err(ctx, XH_E_INVALID, "unsupported wcls dtype");
    }
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

// the step of `kind` into its slot of ctx->g_step
int capture(xh_ctx* ctx, StepKind kind) {
    hipGraph_t g = nullptr;
    HIP_TRY(ctx, hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
    const int rc = enqueue_step(ctx, ctx->stream, kind);
    hipError_t e = hipStreamEndCapture(ctx->stream, &g);
    if (rc) { if (g) hipGraphDestroy(g); return rc; }
    if (e != hipSuccess) return set_err(ctx, XH_E_HIP, "graph capture failed: %s", hipGetErrorString(e));
    e = hipGraphInstantiate(&ctx->g_step[kind], g, nullptr, nullptr, 0);
    hipGraphDestroy(g);
    if (e != hipSuccess) return set_err(ctx, XH_E_HIP, "graph instantiate failed: %s", hipGetErrorString(e));
    return 0;
}

// an eager step that failed part-way: the attention + Wo hand-off words may hold arrivals that
// the layer's W1/W3 launch never zeroed
int eager_step(xh_ctx* ctx, StepKind kind) {
    const int rc = enqueue_step(ctx, ctx->stream, kind);
    if (rc) hipMemsetAsync(ctx->aw_sync, 0, (size_t)ctx->c.n_layers * AW_SYNC_WORDS * 4, ctx->stream);
    return rc;
}
}  // namespace

GemvArgs xalm::qkv_args(xh_ctx* ctx, int l) {
    const LayerW& w = ctx->L[l];
    GemvArgs a{};
    a.w = w.wqkv; a.row_bytes = dev_row_bytes(w.qkv_dt, ctx->c.dim);
    a.n = ctx->c.dim; a.rows = ctx->q_dim + 2 * ctx->kv_dim; a.x = ctx->x;
    a.norm_w = w.attn_norm; a.norm_dtype = w.an_dt; a.eps = ctx->c.norm_eps;
    a.q = ctx->q; a.kcache = ctx->kcache(l); a.vcache = ctx->vcache(l);
    a.q_dim = ctx->q_dim; a.kv_dim = ctx->kv_dim; a.head_dim = ctx->c.head_dim;
    a.rope_freq = ctx->rope_freq; a.rope_cs = ctx->rope_cs; a.sink_cos = ctx->sink_cos; a.sink_sin = ctx->sink_sin;
    a.qkv_clip = ctx->c.qkv_clip; a.sp = ctx->sp;
    if (ctx->kv8()) a.sink_master = ctx->master(l);
    if (layer_traced(ctx, l)) a.trace = ctx->aw_trace + LT_QKV;
    return a;
}
GemvArgs xalm::wo_args(xh_ctx* ctx, int l) {
    const LayerW& w = ctx->L[l];
    GemvArgs a{};
    a.w = w.wo; a.row_bytes = dev_row_bytes(w.wo_dt, ctx->q_dim);
    a.n = ctx->q_dim; a.rows = ctx->c.dim; a.x = ctx->attn_out; a.out = ctx->x; a.sp = ctx->sp;
    return a;
}
GemvArgs xalm::w13_args(xh_ctx* ctx, int l) {
    const LayerW& w = ctx->L[l];
    GemvArgs a{};
    a.w = w.w13; a.row_bytes = dev_row_bytes(w.w13_dt, ctx->c.dim);
    a.n = ctx->c.dim; a.rows = 2 * ctx->c.hidden_dim; a.x = ctx->x;
    a.norm_w = w.ffn_norm; a.norm_dtype = w.fn_dt; a.eps = ctx->c.norm_eps;
    a.out = ctx->hb; a.act = ctx->c.act; a.sp = ctx->sp;
    if (ctx->w13_trace_on) a.trace = ctx->aw_trace;
    if (layer_traced(ctx, l)) a.trace = ctx->aw_trace + LT_W13;
    return a;
}
GemvArgs xalm::w2_args(xh_ctx* ctx, int l) {
    const LayerW& w = ctx->L[l];
    GemvArgs a{};
    a.w = w.w2; a.row_bytes = dev_row_bytes(w.w2_dt, ctx->c.hidden_dim);
    a.n = ctx->c.hidden_dim; a.rows = ctx->c.dim; a.x = ctx->hb; a.out = ctx->x; a.sp = ctx->sp;
    if (layer_traced(ctx, l)) a.trace = ctx->aw_trace + LT_W2;
    return a;
}
GemvArgs xalm::cls_args(xh_ctx* ctx) {
    GemvArgs a{};
    a.w = ctx->wcls; a.row_bytes = dev_row_bytes(ctx->wcls_dt, ctx->c.dim);
    a.n = ctx->c.dim; a.rows = ctx->c.vocab_size; a.x = ctx->x;
    a.norm_w = ctx->final_norm; a.norm_dtype = ctx->final_norm_dt; a.eps = ctx->c.norm_eps;
    a.out = ctx->logits; a.sp = ctx->sp; a.cand = ctx->cand;
    if (ctx->layer_trace_on) a.trace = ctx->aw_trace + LT_CLS;
    return a;
}
AttnArgs xalm::attn_args(xh_ctx* ctx, int l) {
    AttnArgs a{};
    a.q = ctx->q; a.kc = ctx->kcache(l); a.vc = ctx->vcache(l); a.kv_dim = ctx->kv_dim;
    a.n_heads = ctx->c.n_heads; a.nsplit = ctx->nsplit; a.out = ctx->attn_out;
    a.part_o = ctx->part_o; a.part_ml = ctx->part_ml; a.counters = ctx->attn_cnt; a.sp = ctx->sp;
    return a;
}
// wave cap of layer l's qkv launch: ctx->qkv_waves for the pipelined shape; gguf blocks take the
// unpipelined staged shape, every wave one group at 16 waves per CU
int xalm::qkv_launch_waves(const xh_ctx* ctx, int l) {
    return gq_dt(ctx->L[l].qkv_dt) ? ctx->max_gemv_waves : ctx->qkv_waves;
}

// a fused hand-off that timed out leaves its sticky flag: report it (after the stream sync)
int xalm::check_aw(xh_ctx* ctx) {
    if (!ctx->fuse_attn_wo) return 0;
    std::vector<unsigned> h((size_t)ctx->c.n_layers * AW_SYNC_WORDS);
    HIP_TRY(ctx, copy_sync(ctx, h.data(), ctx->aw_sync, h.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
    for (int l = 0; l < ctx->c.n_layers; l++)
        if (h[(size_t)AW_SYNC_WORDS * l + 2]) {
            // reported once: the sticky words are cleared so the context can be reset and reused
            HIP_TRY(ctx, fill_sync(ctx, ctx->aw_sync, 0, h.size() * sizeof(unsigned)));
            return set_err(ctx, XH_E_HIP, "layer %d: attention -> Wo hand-off timed out", l);
        }
    return 0;
}

int xalm::check_ready(xh_ctx* ctx) {
    if (!ctx->embed) return set_err(ctx, XH_E_STATE, "embed.weight not uploaded");
    if (!ctx->final_norm) return set_err(ctx, XH_E_STATE, "output.norm.weight not uploaded");
    if (!ctx->wcls) {
        if (ctx->c.tie_word_embeddings) { ctx->wcls = ctx->embed; ctx->wcls_dt = ctx->embed_dt; }
        else return set_err(ctx, XH_E_STATE, "output.weight not uploaded");
    }
    for (int l = 0; l < ctx->c.n_layers; l++) {
        const LayerW& w = ctx->L[l];
        if (w.qkv_have != 7 || w.w13_have != 3 || !w.wo || !w.w2 || !w.attn_norm || !w.ffn_norm)
            return set_err(ctx, XH_E_STATE, "layer %d: weights incomplete", l);
    }
    return 0;
}

void xalm::time_head(xh_ctx* ctx, StepKind head) { launch_head(ctx, head, ctx->stream); }

void xalm::launch_top_logprobs(const float* logits, int vocab, size_t stride, int n_rows, const int* n_top_dev, int n_top,
                               const StepParams* sp, int cap, const int* targets, int out_stride, int* ids, float* lps,
                               float* target_lp, int* target_rank, hipStream_t s) {
    hipLaunchKernelGGL(top_logprobs_kernel, dim3(n_rows), dim3(SMP_THREADS), 0, s, logits, vocab, stride, n_top_dev, n_top,
                       sp, cap, targets, out_stride, ids, lps, target_lp, target_rank);
}
// row 0 of the context's buffers, no target
void xalm::time_top_logprobs(xh_ctx* ctx) {
    launch_top_logprobs(ctx->logits, ctx->c.vocab_size, 0, 1, ctx->top_n_dev, 0, nullptr, 0, nullptr, XH_TOP_MAX,
                        ctx->top_ids, ctx->top_lps, nullptr, nullptr, ctx->stream);
}

void xalm::drop_graphs(xh_ctx* ctx) {
    for (hipGraphExec_t& g : ctx->g_step) {
        if (g) hipGraphExecDestroy(g);
        g = nullptr;
    }
}

// the step at host_step_params' position
int xalm::run_step(xh_ctx* ctx, bool with_logits) {
    const StepKind kind = with_logits ? STEP_LOGITS : STEP_HYDRATE;
    if (with_logits) ctx->cand_valid = true;  // the lm_head launch writes candidates
    if (!ctx->use_graphs) return eager_step(ctx, kind);
    if (!ctx->g_step[kind]) {
        int rc = capture(ctx, kind);
        if (rc) return rc;
    }
    HIP_TRY(ctx, hipGraphLaunch(ctx->g_step[kind], ctx->stream));
    return 0;
}

int xalm::host_step_params(xh_ctx* ctx, int token, int pos) {
    StepParams* h = ctx->sp_host;
    const int msl = ctx->c.max_seq_len;
    h->token = token;
    h->pos = pos;
    h->kv_sink = pos >= msl ? 2 : 0;
    h->kv_pos = h->kv_sink + (pos - h->kv_sink) % (msl - h->kv_sink);
    h->kv_len = pos >= msl ? msl : pos + 1;
    h->step = 0;
    h->pos_next = pos + 1;
    h->max_seq_len = msl;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->sp, h, sizeof(StepParams), hipMemcpyHostToDevice, ctx->stream));
    return 0;
}

namespace {
// xh_sampling as the header defines it: temperature >= 0, top_k >= 0, top_p in (0, 1]; NaN fails each
bool sampling_ok(const xh_sampling* s) {
    return s && s->temperature >= 0.f && s->top_k >= 0 && s->top_p > 0.f && s->top_p <= 1.f;
}

// xh_logit_ctl as the header defines it (null = all off), with the token list that feeds the
// window; vocab <= 0: unknown (no context), the ids are only checked for sign.  nullptr = valid.
const char* ctl_error(const xh_logit_ctl* c, const int* toks, int n_toks, int vocab) {
    if (n_toks < 0) return "negative token count";
    if (n_toks > 0 && !toks) return "null token list";
    for (int i = std::max(0, n_toks - XH_CTL_MAX_WINDOW); i < n_toks; i++)
        if (toks[i] < 0 || (vocab > 0 && toks[i] >= vocab)) return "window token out of range";
    if (!c) return nullptr;
    if (!(c->repeat_penalty > 0.f) || !std::isfinite(c->repeat_penalty)) return "repeat_penalty must be > 0 and finite";
    if (!std::isfinite(c->presence_penalty) || !std::isfinite(c->frequency_penalty)) return "penalties must be finite";
    if (c->last_n < 0 || c->last_n > XH_CTL_MAX_WINDOW) return "last_n outside 0 .. XH_CTL_MAX_WINDOW";
    if (!(c->min_p >= 0.f && c->min_p <= 1.f)) return "min_p outside [0, 1]";
    if (c->n_bias < 0 || c->n_bias > XH_CTL_MAX_BIAS) return "n_bias outside 0 .. XH_CTL_MAX_BIAS";
    if (c->n_bias > 0 && (!c->bias_token || !c->bias_value)) return "null bias array";
    std::vector<int> ids(c->bias_token, c->bias_token + c->n_bias);
    std::sort(ids.begin(), ids.end());
    for (int i = 0; i < c->n_bias; i++) {
        if (ids[i] < 0 || (vocab > 0 && ids[i] >= vocab)) return "bias id out of range";
        if (i && ids[i] == ids[i - 1]) return "duplicate bias id";
        const float b = c->bias_value[i];
        if (std::isnan(b) || b == INFINITY) return "bias value must be finite or -inf";
    }
    return nullptr;
}

const xh_logit_ctl CTL_OFF = {1.f, 0.f, 0.f, 0, 0.f, 0, nullptr, nullptr};

// the device block of (sampling, ctl) with `count` tokens in the ring
ExtCtl ext_block(const xh_sampling& s, const xh_logit_ctl& c, int count) {
    ExtCtl e{};
    e.samp = s;
    e.repeat_penalty = c.repeat_penalty;
    e.presence_penalty = c.presence_penalty;
    e.frequency_penalty = c.frequency_penalty;
    e.last_n = c.last_n;
    e.min_p = c.min_p;
    e.n_bias = c.n_bias;
    e.count = count;
    return e;
}

// the device block of a constraint's tables (device pointers) at `state`; a stop token that is off is -1
DfaCtl dfa_block(const void* next, const void* accept, const void* bytes, const void* offsets, int n_states,
                 uint32_t state, int stop_a, int stop_b) {
    return DfaCtl{(const uint16_t*)next, (const uint8_t*)accept, (const uint8_t*)bytes, (const uint32_t*)offsets,
                  n_states, state, stop_a < 0 ? -1 : stop_a, stop_b < 0 ? -1 : stop_b};
}

AdaptCtl adapt_block(const xh_trunc_ctl& t, float mu, bool constrain) {
    return AdaptCtl{t.typical_p, t.top_n_sigma, t.mirostat_tau, t.mirostat_eta, mu, constrain ? 1 : 0};
}

// the device block of xh_seq_ctl and its breakers in ascending order (what the head's binary search needs)
SeqCtl seq_block(const xh_seq_ctl& q, std::vector<int>* sorted) {
    sorted->assign(q.breaker_token, q.breaker_token + q.n_breakers);
    std::sort(sorted->begin(), sorted->end());
    return SeqCtl{q.dry_multiplier, q.dry_base, q.dry_allowed_length, q.no_repeat_ngram, q.seq_last_n, q.n_breakers,
                  q.xtc_probability, q.xtc_threshold};
}

// ---------------------------------------------------------------------------------------
// the decode loop: one driver under the six xh_decode_* entries
// ---------------------------------------------------------------------------------------
// The union of the entries' arguments; an entry leaves what its head does not take at null / 0.
// The heads are cumulative: each one from STEP_SAMPLE_EXT up takes what the one before it takes.
struct DecodeCall {
    StepKind head;  // STEP_GREEDY .. STEP_SAMPLE_SEQ
    int pos, n_steps;
    const xh_sampling* sampling;  // from STEP_SAMPLE
    const xh_logit_ctl* ctl;      // from STEP_SAMPLE_EXT, with the history that fills the window ring
    const xh_trunc_ctl* trunc;    // from STEP_SAMPLE_ADAPT
    const xh_seq_ctl* seq;        // STEP_SAMPLE_SEQ
    const int* history;
    int n_history;
    int constrain;  // the DFA mask runs: always under STEP_SAMPLE_DFA, the caller's choice above it
    uint32_t state_in;
    float mu_in;
    int stop_a, stop_b;
    int* tokens_out;
    float* logprobs_out;
    uint32_t* state_out;
    float* mu_out;
    int* n_done;
};

int decode_run(xh_ctx* ctx, const DecodeCall& k) {
    const StepKind head = k.head;
    const bool sampled = head >= STEP_SAMPLE, ext = head >= STEP_SAMPLE_EXT, adapt = head >= STEP_SAMPLE_ADAPT;
    const bool seq = head == STEP_SAMPLE_SEQ, constrained = k.constrain != 0;
    // the checks, every one before the first HIP call; those on the arguments alone come before
    // those that need the context
    if (k.n_done) *k.n_done = 0;
    if (sampled && !sampling_ok(k.sampling)) return set_err(ctx, XH_E_INVALID, "bad sampling parameters");
    const int vocab = ctx ? ctx->c.vocab_size : 0;
    const char* why = nullptr;
    if (ext) why = ctl_error(k.ctl, k.history, k.n_history, vocab);
    if (!why && adapt) why = trunc_error(k.trunc, k.sampling, k.ctl ? k.ctl->min_p : 0.f, k.mu_in);
    if (!why && seq) why = seq_error(k.seq, k.trunc, vocab);
    if (why) return set_err(ctx, XH_E_INVALID, "%s", why);
    if (!ctx || k.n_steps < 0) return XH_E_INVALID;
    if (sampled) {
        if (k.pos < 0) return set_err(ctx, XH_E_INVALID, "negative pos");
        if (vocab > SMP_MAX_VOCAB) return set_err(ctx, XH_E_INVALID, "vocab_size > %d", SMP_MAX_VOCAB);
    }
    if (k.n_steps > ctx->dec_cap) return set_err(ctx, XH_E_INVALID, "n_steps > %d", ctx->dec_cap);
    if (constrained) {
        if (!ctx->dfa_vocab_set || !ctx->dfa_n_states)
            return set_err(ctx, XH_E_INVALID, "constrained decode before xh_constraint_set_vocab and xh_constraint_set");
        if (k.state_in != XH_DFA_DEAD && k.state_in >= (uint32_t)ctx->dfa_n_states)
            return set_err(ctx, XH_E_INVALID, "state_in %u out of range", k.state_in);
        // an end token is emitted in the stuck state, so it has to be a token
        if (k.stop_a >= vocab || k.stop_b >= vocab) return set_err(ctx, XH_E_INVALID, "stop token out of range");
    }
    HIP_TRY(ctx, hipSetDevice(ctx->dev));
    int rc = check_ready(ctx);
    if (rc) return rc;
    // step counter 0, next position `pos`; the head sets the token and position fields
    StepParams* h = ctx->sp_host;
    h->step = 0;
    h->pos_next = k.pos;
    h->max_seq_len = ctx->c.max_seq_len;
    HIP_TRY(ctx, hipMemcpyAsync(&ctx->sp->step, &h->step, 3 * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    // The head's parameter blocks.  Every source is pageable, so a copy has left it when
    // hipMemcpyAsync returns: the blocks may be locals and the caller's arrays may go after the call.
    const hipStream_t s = ctx->stream;
    if (head == STEP_SAMPLE) HIP_TRY(ctx, hipMemcpyAsync(ctx->samp, k.sampling, sizeof(xh_sampling), hipMemcpyHostToDevice, s));
    if (ext) {
        // the block, the bias table and the history's tail (ring slots 0 .. n_hist - 1)
        const xh_logit_ctl& c = k.ctl ? *k.ctl : CTL_OFF;
        const int n_hist = std::min(k.n_history, XH_CTL_MAX_WINDOW);
        const ExtCtl blk = ext_block(*k.sampling, c, n_hist);
        HIP_TRY(ctx, hipMemcpyAsync(ctx->ext, &blk, sizeof blk, hipMemcpyHostToDevice, s));
        if (c.n_bias > 0) {
            HIP_TRY(ctx, hipMemcpyAsync(ctx->ext_btok, c.bias_token, (size_t)c.n_bias * sizeof(int), hipMemcpyHostToDevice, s));
            HIP_TRY(ctx, hipMemcpyAsync(ctx->ext_bval, c.bias_value, (size_t)c.n_bias * sizeof(float), hipMemcpyHostToDevice, s));
        }
        if (n_hist > 0)
            HIP_TRY(ctx, hipMemcpyAsync(ctx->ext_ring, k.history + (k.n_history - n_hist), (size_t)n_hist * sizeof(int),
                                        hipMemcpyHostToDevice, s));
    }
    if (constrained) {
        const DfaCtl blk = dfa_block(ctx->dfa_next, ctx->dfa_accept, ctx->dfa_bytes, ctx->dfa_offsets, ctx->dfa_n_states,
                                     k.state_in, k.stop_a, k.stop_b);
        HIP_TRY(ctx, hipMemcpyAsync(ctx->dfa, &blk, sizeof blk, hipMemcpyHostToDevice, s));
        ctx->dfa_block_valid = true;
    }
    if (adapt) {
        // mu lives in the block: the head reads and writes it every step
        const AdaptCtl blk = adapt_block(*k.trunc, k.mu_in, k.constrain != 0);
        HIP_TRY(ctx, hipMemcpyAsync(ctx->adapt, &blk, sizeof blk, hipMemcpyHostToDevice, s));
        // the timing hooks of this head and of the ones above read ctx->adapt: it holds this call's parameters now
        ctx->adapt_valid = true;
        ctx->adapt_constrain = k.constrain != 0;
    }
    if (seq) {
        std::vector<int> brk;
        const SeqCtl blk = seq_block(*k.seq, &brk);
        const SeqTail tail = {ctx->dec_tokens, ctx->dec_logprobs, ctx->dec_states, (const void*)ctx->embed, ctx->x,
                              (const float*)ctx->rope_freq, ctx->rope_cs, ctx->dec_cap, ctx->embed_dt, ctx->c.dim,
                              ctx->c.head_dim / 2};
        HIP_TRY(ctx, hipMemcpyAsync(ctx->seq, &blk, sizeof blk, hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->seq_tail, &tail, sizeof tail, hipMemcpyHostToDevice, s));
        if (!brk.empty())
            HIP_TRY(ctx, hipMemcpyAsync(ctx->seq_brk, brk.data(), brk.size() * sizeof(int), hipMemcpyHostToDevice, s));
        ctx->seq_valid = true;
        ctx->seq_constrain = k.constrain != 0;
    }
    if (ext) HIP_TRY(ctx, hipStreamSynchronize(s));
    if (ctx->use_graphs && k.n_steps > 0 && !ctx->g_step[head]) {
        rc = capture(ctx, head);
        if (rc) return rc;
    }
    if (head == STEP_GREEDY) {
        // the first token is the argmax of the logits on the device: candidates from them if the
        // launch that produced them left none (nothing yet)
        if (!ctx->cand_valid)
            hipLaunchKernelGGL(logits_cand_kernel, dim3(1), dim3(ARGMAX_CANDS), 0, s, (const float*)ctx->logits,
                               ctx->c.vocab_size, ctx->cand);
        ctx->cand_valid = true;
    }
    // A sampled head reads the logits themselves, so cand and cand_valid stay as they were until a
    // step has run: every step's lm_head launch rewrites cand for the raw logits it leaves, and a
    // greedy call may follow.
    const bool stops = k.stop_a >= 0 || k.stop_b >= 0;
    int done = 0;
    for (int i = 0; i < k.n_steps; i++) {
        if (ctx->use_graphs) {
            HIP_TRY(ctx, hipGraphLaunch(ctx->g_step[head], s));
        } else {
            rc = eager_step(ctx, head);
            if (rc) return rc;
        }
        ctx->cand_valid = true;
        done = i + 1;
        if (stops) {
            int tok = -1;
            HIP_TRY(ctx, hipMemcpyAsync(&tok, ctx->dec_tokens + i, sizeof(int), hipMemcpyDeviceToHost, s));
            HIP_TRY(ctx, hipStreamSynchronize(s));
            if (tok == k.stop_a || tok == k.stop_b) break;
        }
    }
    if (k.tokens_out && done)
        HIP_TRY(ctx, hipMemcpyAsync(k.tokens_out, ctx->dec_tokens, (size_t)done * sizeof(int), hipMemcpyDeviceToHost, s));
    if (ext && k.logprobs_out && done)
        HIP_TRY(ctx, hipMemcpyAsync(k.logprobs_out, ctx->dec_logprobs, (size_t)done * sizeof(float), hipMemcpyDeviceToHost, s));
    // no step runs past the last emitted token, so the per-step log holds the state and the block mu after it
    uint32_t st = k.state_in;
    float mu = k.mu_in;
    if (constrained && done)
        HIP_TRY(ctx, hipMemcpyAsync(&st, ctx->dec_states + (done - 1), sizeof st, hipMemcpyDeviceToHost, s));
    if (adapt && done) HIP_TRY(ctx, hipMemcpyAsync(&mu, &ctx->adapt->mu, sizeof mu, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    if (k.state_out) *k.state_out = st;
    if (k.mu_out) *k.mu_out = mu;
    if (k.n_done) *k.n_done = done;
    ctx->top_steps = ctx->top_n > 0 ? done : -1;
    return check_aw(ctx);
}

// ---------------------------------------------------------------------------------------
// the xh_op_* entries: the heads' device code on host arrays, without a context
// ---------------------------------------------------------------------------------------
// a device buffer of an op, freed with it: at least 16 bytes, the first src_bytes copied from src
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) hipFree(p); }
    bool alloc(size_t bytes, const void* src = nullptr, size_t src_bytes = 0) {
        if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) return false;
        return !src_bytes || hipMemcpy(p, src, src_bytes, hipMemcpyHostToDevice) == hipSuccess;
    }
};

// The xh_op_sample* entries' argument checks in the order they report them; 0 = valid.  outs: the
// entry's required outputs are all there.  ctl, trunc and seq are checked from the head that takes
// them; STEP_SAMPLE_DFA demands the constraint, the heads above it take one or none (dfa null).
int op_check(StepKind head, const float* logits, int vocab, const xh_sampling* sampling, int n_draws, bool outs,
             const xh_logit_ctl* ctl = nullptr, const int* window = nullptr, int n_window = 0,
             const xh_trunc_ctl* trunc = nullptr, float mu = 0.f, const xh_seq_ctl* seq = nullptr,
             const xh_byte_dfa* dfa = nullptr, const uint8_t* bytes = nullptr, const uint32_t* offsets = nullptr,
             uint32_t state = 0, int stop_a = -1, int stop_b = -1) {
    if (!sampling_ok(sampling)) return set_err(nullptr, XH_E_INVALID, "bad sampling parameters");
    if (!logits || !outs || vocab <= 0 || vocab > SMP_MAX_VOCAB || n_draws <= 0 || n_draws > 65536)
        return set_err(nullptr, XH_E_INVALID, "bad sample args");
    const char* why = nullptr;
    if (head >= STEP_SAMPLE_EXT) why = ctl_error(ctl, window, n_window, vocab);
    if (!why && head >= STEP_SAMPLE_ADAPT) why = trunc_error(trunc, sampling, ctl ? ctl->min_p : 0.f, mu);
    if (!why && head == STEP_SAMPLE_SEQ) why = seq_error(seq, trunc, vocab);
    if (!why && (head == STEP_SAMPLE_DFA || (head > STEP_SAMPLE_DFA && dfa))) {
        why = dfa_error(dfa);
        if (!why) why = pieces_error(bytes, offsets, vocab);
        if (!why) why = dfa_state_error(dfa, state);
        if (!why && (stop_a >= vocab || stop_b >= vocab)) why = "stop token out of range";
    }
    return why ? set_err(nullptr, XH_E_INVALID, "%s", why) : 0;
}

// what every op from xh_op_sample_ext up reads: the logits, room for l', the block of (sampling, ctl)
// with the window's tail in the ring, and the bias table
struct ExtStage {
    DevBuf logits, adj, blk, ring, btok, bval;
    bool stage(const float* h_logits, int vocab, const xh_sampling& s, const xh_logit_ctl* ctl, const int* window,
               int n_window) {
        const xh_logit_ctl& c = ctl ? *ctl : CTL_OFF;
        const int n_win = std::min(n_window, XH_CTL_MAX_WINDOW);
        const ExtCtl b = ext_block(s, c, n_win);
        const size_t V = (size_t)vocab;
        return logits.alloc(V * 4, h_logits, V * 4) && adj.alloc(V * 4) && blk.alloc(sizeof b, &b, sizeof b) &&
               ring.alloc(XH_CTL_MAX_WINDOW * sizeof(int), n_win ? window + (n_window - n_win) : nullptr,
                          (size_t)n_win * sizeof(int)) &&
               btok.alloc(XH_CTL_MAX_BIAS * sizeof(int), c.bias_token, (size_t)c.n_bias * sizeof(int)) &&
               bval.alloc(XH_CTL_MAX_BIAS * sizeof(float), c.bias_value, (size_t)c.n_bias * sizeof(float));
    }
};

// a constraint's four tables and the block that points at them; dfa null: the block alone, its tables null
struct DfaStage {
    DevBuf next, acc, bytes, offs, blk;
    bool stage(const xh_byte_dfa* dfa, const uint8_t* h_bytes, const uint32_t* offsets, int vocab, uint32_t state,
               int stop_a, int stop_b) {
        const size_t ns = dfa ? (size_t)dfa->n_states : 0, V = (size_t)vocab;
        if (dfa && !(next.alloc(ns * 512, dfa->next, ns * 512) && acc.alloc(ns, dfa->accept, ns) &&
                     bytes.alloc(offsets[vocab], h_bytes, offsets[vocab]) && offs.alloc((V + 1) * 4, offsets, (V + 1) * 4)))
            return false;
        const DfaCtl b = dfa_block(next.p, acc.p, bytes.p, offs.p, (int)ns, state, stop_a, stop_b);
        return blk.alloc(sizeof b, &b, sizeof b);
    }
};

int op_stage_failed() { return set_err(nullptr, XH_E_HIP, "hipMalloc / hipMemcpy failed"); }

// behind an op's launches: wait for them ...
hipError_t op_wait() {
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : hipDeviceSynchronize();
}
// ... and copy a result back: a null destination is skipped, the first error is carried forward
void op_out(hipError_t& e, void* dst, const void* src, size_t bytes) {
    if (e == hipSuccess && dst) e = hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);
}
}  // namespace

extern "C" {

int xh_forward(xh_ctx* ctx, int token, int pos, int mode, float* logits_out) {
    if (!ctx) return XH_E_INVALID;
    if (token < 0 || token >= ctx->c.vocab_size) return set_err(ctx, XH_E_INVALID, "token %d out of range", token);
    if (pos < 0) return set_err(ctx, XH_E_INVALID, "negative pos");
    if (mode != XH_HYDRATE_KV_CACHE && mode != XH_OUTPUT_LOGITS) return set_err(ctx, XH_E_INVALID, "bad mode");
    HIP_TRY(ctx, hipSetDevice(ctx->dev));
    int rc = check_ready(ctx);
    if (rc) return rc;
    rc = host_step_params(ctx, token, pos);
    if (!rc) rc = run_step(ctx, mode == XH_OUTPUT_LOGITS);
    if (rc) return rc;
    if (logits_out && mode == XH_OUTPUT_LOGITS)
        HIP_TRY(ctx, hipMemcpyAsync(logits_out, ctx->logits, (size_t)ctx->c.vocab_size * 4, hipMemcpyDeviceToHost,
                                    ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return check_aw(ctx);
}

// The six decode entries: a DecodeCall in its field order (head; pos, n_steps; sampling, ctl, trunc, seq;
// history; constrain, state_in, mu_in; stops; the five outputs) for decode_run.
int xh_decode_greedy(xh_ctx* ctx, int pos, int n_steps, int stop_a, int stop_b, int* tokens_out, int* n_done) {
    if (!ctx || n_steps < 0) return XH_E_INVALID;  // this entry alone leaves *n_done as it was here
    return decode_run(ctx, {STEP_GREEDY, pos, n_steps, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0.f, stop_a,
                            stop_b, tokens_out, nullptr, nullptr, nullptr, n_done});
}

int xh_decode_sample(xh_ctx* ctx, int pos, int n_steps, const xh_sampling* sampling, int stop_a, int stop_b,
                     int* tokens_out, int* n_done) {
    return decode_run(ctx, {STEP_SAMPLE, pos, n_steps, sampling, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0.f, stop_a,
                            stop_b, tokens_out, nullptr, nullptr, nullptr, n_done});
}

int xh_op_sample(const float* logits, int vocab, const xh_sampling* sampling, uint64_t pos0, int n_draws,
                 int* tokens_out, int* n_kept_out) {
    if (int rc = op_check(STEP_SAMPLE, logits, vocab, sampling, n_draws, tokens_out && n_kept_out)) return rc;
    const size_t V = (size_t)vocab, nd = (size_t)n_draws;
    DevBuf d_logits, d_samp, d_out;
    if (!d_logits.alloc(V * 4) || !d_samp.alloc(sizeof(xh_sampling)) || !d_out.alloc(2 * nd * sizeof(int)))
        return set_err(nullptr, XH_E_HIP, "hipMalloc failed");
    if (hipMemcpy(d_logits.p, logits, V * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_samp.p, sampling, sizeof(xh_sampling), hipMemcpyHostToDevice) != hipSuccess)
        return set_err(nullptr, XH_E_HIP, "hipMemcpy failed");
    int* d_tok = (int*)d_out.p;
    hipLaunchKernelGGL(sample_op_kernel, dim3(n_draws), dim3(SMP_THREADS), 0, nullptr, (const float*)d_logits.p, vocab,
                       (const xh_sampling*)d_samp.p, (uint32_t)pos0, d_tok, d_tok + nd);
    hipError_t e = op_wait();
    op_out(e, tokens_out, d_tok, nd * sizeof(int));
    op_out(e, n_kept_out, d_tok + nd, nd * sizeof(int));
    if (e != hipSuccess) return set_err(nullptr, XH_E_HIP, "sample op failed: %s", hipGetErrorString(e));
    return 0;
}


int xh_adjust_logits(const float* logits, int vocab, const xh_logit_ctl* ctl, const int* window, int n_window,
                     float* out) {
    if (!logits || !out || vocab <= 0) return set_err(nullptr, XH_E_INVALID, "bad adjust args");
    if (const char* why = ctl_error(ctl, window, n_window, vocab)) return set_err(nullptr, XH_E_INVALID, "%s", why);
    const xh_logit_ctl& c = ctl ? *ctl : CTL_OFF;
    std::copy(logits, logits + vocab, out);
    // (token, count) of the window's distinct tokens
    const int n_win = std::min(c.last_n, n_window);
    std::vector<int> win(window + (n_window - n_win), window + n_window);
    std::sort(win.begin(), win.end());
    std::vector<char> seen;  // bias entries whose token the window holds
    seen.assign((size_t)c.n_bias, 0);
    for (size_t i = 0; i < win.size();) {
        size_t j = i;
        while (j < win.size() && win[j] == win[i]) j++;
        const int t = win[i];
        bool biased = false;
        float b = 0.f;
        for (int k = 0; k < c.n_bias; k++)
            if (c.bias_token[k] == t) { biased = true; b = c.bias_value[k]; seen[k] = 1; }
        out[t] = ctl_adjust(logits[t], (int)(j - i), biased, b, c.repeat_penalty, c.presence_penalty, c.frequency_penalty);
        i = j;
    }
    for (int k = 0; k < c.n_bias; k++)
        if (!seen[k]) {
            const int t = c.bias_token[k];
            out[t] = ctl_adjust(logits[t], 0, true, c.bias_value[k], c.repeat_penalty, c.presence_penalty, c.frequency_penalty);
        }
    return 0;
}

int xh_decode_sample_ext(xh_ctx* ctx, int pos, int n_steps, const xh_sampling* sampling, const xh_logit_ctl* ctl,
                         const int* history, int n_history, int stop_a, int stop_b, int* tokens_out,
                         float* logprobs_out, int* n_done) {
    return decode_run(ctx, {STEP_SAMPLE_EXT, pos, n_steps, sampling, ctl, nullptr, nullptr, history, n_history, 0, 0, 0.f,
                            stop_a, stop_b, tokens_out, logprobs_out, nullptr, nullptr, n_done});
}

int xh_op_sample_ext(const float* logits, int vocab, const xh_sampling* sampling, const xh_logit_ctl* ctl,
                     const int* window, int n_window, uint64_t pos0, int n_draws, int* tokens_out, int* n_kept_out,
                     float* adjusted_out, float* logprob_out) {
    if (int rc = op_check(STEP_SAMPLE_EXT, logits, vocab, sampling, n_draws, tokens_out && n_kept_out, ctl, window, n_window))
        return rc;
    const size_t V = (size_t)vocab, nd = (size_t)n_draws;
    ExtStage x;
    DevBuf d_prep, d_out, d_lp;
    if (!x.stage(logits, vocab, *sampling, ctl, window, n_window) || !d_prep.alloc(sizeof(ExtPrep)) ||
        !d_out.alloc(2 * nd * sizeof(int)) || !d_lp.alloc(nd * sizeof(float)))
        return op_stage_failed();
    int* d_tok = (int*)d_out.p;
    hipLaunchKernelGGL(sample_ext_prep_kernel, dim3(1), dim3(SMP_THREADS), 0, nullptr, (const float*)x.logits.p, vocab,
                       (const ExtCtl*)x.blk.p, (const int*)x.ring.p, (const int*)x.btok.p, (const float*)x.bval.p,
                       (float*)x.adj.p, (ExtPrep*)d_prep.p);
    hipLaunchKernelGGL(sample_ext_op_kernel, dim3(n_draws), dim3(SMP_THREADS), 0, nullptr, (const float*)x.logits.p,
                       (const float*)x.adj.p, vocab, (const ExtCtl*)x.blk.p, (const ExtPrep*)d_prep.p, (uint32_t)pos0,
                       d_tok, d_tok + nd, (float*)d_lp.p);
    hipError_t e = op_wait();
    op_out(e, tokens_out, d_tok, nd * sizeof(int));
    op_out(e, n_kept_out, d_tok + nd, nd * sizeof(int));
    op_out(e, adjusted_out, x.adj.p, V * 4);
    op_out(e, logprob_out, d_lp.p, nd * sizeof(float));
    if (e != hipSuccess) return set_err(nullptr, XH_E_HIP, "sample_ext op failed: %s", hipGetErrorString(e));
    return 0;
}


int xh_constraint_set_vocab(xh_ctx* ctx, const uint8_t* bytes, const uint32_t* offsets) {
    if (!ctx) return XH_E_INVALID;
    const int V = ctx->c.vocab_size;
    if (const char* why = pieces_error(bytes, offsets, V)) return set_err(ctx, XH_E_INVALID, "%s", why);
    HIP_TRY(ctx, hipSetDevice(ctx->dev));
    // the new tables are whole on the device before the old ones go: a failure keeps the old constraint
    uint8_t* d_bytes = nullptr;
    uint32_t* d_offsets = nullptr;
    int rc = dmalloc(ctx, &d_bytes, (size_t)offsets[V]);
    if (!rc) rc = dmalloc(ctx, &d_offsets, (size_t)V + 1);
    hipError_t e = hipSuccess;
    if (!rc && offsets[V]) e = copy_sync(ctx, d_bytes, bytes, offsets[V], hipMemcpyHostToDevice);
    if (!rc && e == hipSuccess) e = copy_sync(ctx, d_offsets, offsets, ((size_t)V + 1) * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (!rc && e != hipSuccess) rc = set_err(ctx, XH_E_HIP, "piece upload failed: %s", hipGetErrorString(e));
    if (rc) {
        hipFree(d_bytes);
        hipFree(d_offsets);
        return rc;
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // no step reads the old table any more
    hipFree(ctx->dfa_bytes);
    hipFree(ctx->dfa_offsets);
    ctx->dfa_bytes = d_bytes;
    ctx->dfa_offsets = d_offsets;
    ctx->dfa_vocab_set = true;
    ctx->dfa_block_valid = false;  // the device block still points at the freed tables
    return 0;
}

int xh_constraint_set(xh_ctx* ctx, const xh_byte_dfa* dfa) {
    if (!ctx) return XH_E_INVALID;
    if (dfa)
        if (const char* why = dfa_error(dfa)) return set_err(ctx, XH_E_INVALID, "%s", why);
    HIP_TRY(ctx, hipSetDevice(ctx->dev));
    uint16_t* d_next = nullptr;
    uint8_t* d_accept = nullptr;
    if (dfa) {
        const size_t n = (size_t)dfa->n_states;
        int rc = dmalloc(ctx, &d_next, n * 256);
        if (!rc) rc = dmalloc(ctx, &d_accept, n);
        hipError_t e = hipSuccess;
        if (!rc) e = copy_sync(ctx, d_next, dfa->next, n * 256 * sizeof(uint16_t), hipMemcpyHostToDevice);
        if (!rc && e == hipSuccess) e = copy_sync(ctx, d_accept, dfa->accept, n, hipMemcpyHostToDevice);
        if (!rc && e != hipSuccess) rc = set_err(ctx, XH_E_HIP, "dfa upload failed: %s", hipGetErrorString(e));
        if (rc) {
            hipFree(d_next);
            hipFree(d_accept);
            return rc;
        }
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    hipFree(ctx->dfa_next);
    hipFree(ctx->dfa_accept);
    ctx->dfa_next = d_next;
    ctx->dfa_accept = d_accept;
    ctx->dfa_n_states = dfa ? dfa->n_states : 0;
    ctx->dfa_block_valid = false;
    return 0;
}

int xh_decode_sample_dfa(xh_ctx* ctx, int pos, int n_steps, const xh_sampling* sampling, const xh_logit_ctl* ctl,
                         const int* history, int n_history, uint32_t state_in, int stop_a, int stop_b, int* tokens_out,
                         float* logprobs_out, uint32_t* state_out, int* n_done) {
    return decode_run(ctx, {STEP_SAMPLE_DFA, pos, n_steps, sampling, ctl, nullptr, nullptr, history, n_history, 1, state_in,
                            0.f, stop_a, stop_b, tokens_out, logprobs_out, state_out, nullptr, n_done});
}

int xh_op_sample_dfa(const float* logits, int vocab, const xh_sampling* sampling, const xh_logit_ctl* ctl,
                     const int* window, int n_window, const xh_byte_dfa* dfa, const uint8_t* bytes,
                     const uint32_t* offsets, uint32_t state, int stop_a, int stop_b, uint64_t pos0, int n_draws,
                     int* tokens_out, int* n_kept_out, float* masked_out, uint32_t* next_state_out, float* logprob_out) {
    if (int rc = op_check(STEP_SAMPLE_DFA, logits, vocab, sampling, n_draws, tokens_out && n_kept_out && next_state_out, ctl,
                          window, n_window, nullptr, 0.f, nullptr, dfa, bytes, offsets, state, stop_a, stop_b))
        return rc;
    const size_t V = (size_t)vocab, nd = (size_t)n_draws;
    ExtStage x;
    DfaStage d;
    DevBuf d_prep, d_out, d_lp;
    if (!x.stage(logits, vocab, *sampling, ctl, window, n_window) || !d_prep.alloc(sizeof(DfaPrep)) ||
        !d_out.alloc(3 * nd * sizeof(int)) || !d_lp.alloc(nd * sizeof(float)) ||
        !d.stage(dfa, bytes, offsets, vocab, state, stop_a, stop_b))
        return op_stage_failed();
    int* d_tok = (int*)d_out.p;
    hipLaunchKernelGGL(sample_dfa_prep_kernel, dim3(1), dim3(SMP_THREADS), 0, nullptr, (const float*)x.logits.p, vocab,
                       (const ExtCtl*)x.blk.p, (const DfaCtl*)d.blk.p, (const int*)x.ring.p, (const int*)x.btok.p,
                       (const float*)x.bval.p, (float*)x.adj.p, (DfaPrep*)d_prep.p);
    hipLaunchKernelGGL(sample_dfa_op_kernel, dim3(n_draws), dim3(SMP_THREADS), 0, nullptr, (const float*)x.logits.p,
                       (const float*)x.adj.p, vocab, (const ExtCtl*)x.blk.p, (const DfaCtl*)d.blk.p,
                       (const DfaPrep*)d_prep.p, (uint32_t)pos0, d_tok, d_tok + nd, (uint32_t*)d_tok + 2 * nd,
                       (float*)d_lp.p);
    hipError_t e = op_wait();
    op_out(e, tokens_out, d_tok, nd * sizeof(int));
    op_out(e, n_kept_out, d_tok + nd, nd * sizeof(int));
    op_out(e, next_state_out, d_tok + 2 * nd, nd * sizeof(uint32_t));
    op_out(e, masked_out, x.adj.p, V * 4);
    op_out(e, logprob_out, d_lp.p, nd * sizeof(float));
    if (e != hipSuccess) return set_err(nullptr, XH_E_HIP, "sample_dfa op failed: %s", hipGetErrorString(e));
    return 0;
}

int xh_decode_sample_adapt(xh_ctx* ctx, int pos, int n_steps, const xh_sampling* sampling, const xh_logit_ctl* ctl,
                           const xh_trunc_ctl* trunc, const int* history, int n_history, int constrain, uint32_t state_in,
                           float mu_in, int stop_a, int stop_b, int* tokens_out, float* logprobs_out, uint32_t* state_out,
                           float* mu_out, int* n_done) {
    return decode_run(ctx, {STEP_SAMPLE_ADAPT, pos, n_steps, sampling, ctl, trunc, nullptr, history, n_history, constrain,
                            state_in, mu_in, stop_a, stop_b, tokens_out, logprobs_out, state_out, mu_out, n_done});
}

int xh_op_sample_adapt(const float* logits, int vocab, const xh_sampling* sampling, const xh_logit_ctl* ctl,
                       const xh_trunc_ctl* trunc, const int* window, int n_window, const xh_byte_dfa* dfa,
                       const uint8_t* bytes, const uint32_t* offsets, uint32_t state, float mu, int stop_a, int stop_b,
                       uint64_t pos0, int n_draws, int* tokens_out, int* n_kept_out, uint32_t* next_state_out,
                       float* mu_out, uint8_t* kept_out, float* thr_out) {
    if (int rc = op_check(STEP_SAMPLE_ADAPT, logits, vocab, sampling, n_draws,
                          tokens_out && n_kept_out && next_state_out && mu_out, ctl, window, n_window, trunc, mu, nullptr, dfa,
                          bytes, offsets, state, stop_a, stop_b))
        return rc;
    const AdaptCtl ablk = adapt_block(*trunc, mu, dfa != nullptr);
    const size_t V = (size_t)vocab, nd = (size_t)n_draws;
    ExtStage x;
    DfaStage d;
    DevBuf d_negd, d_kept, d_ablk, d_prep, d_out, d_mu;
    if (!x.stage(logits, vocab, *sampling, ctl, window, n_window) || !d_negd.alloc(V * 4) || !d_kept.alloc(V) ||
        !d_ablk.alloc(sizeof ablk, &ablk, sizeof ablk) || !d_prep.alloc(sizeof(AdaptOpPrep)) ||
        !d_out.alloc(3 * nd * sizeof(int)) || !d_mu.alloc(nd * sizeof(float)) ||
        !d.stage(dfa, bytes, offsets, vocab, state, stop_a, stop_b))
        return op_stage_failed();
    int* d_tok = (int*)d_out.p;
    hipLaunchKernelGGL(sample_adapt_prep_kernel, dim3(1), dim3(SMP_THREADS), 0, nullptr, (const float*)x.logits.p, vocab,
                       (const ExtCtl*)x.blk.p, (const DfaCtl*)d.blk.p, (const AdaptCtl*)d_ablk.p, (const int*)x.ring.p,
                       (const int*)x.btok.p, (const float*)x.bval.p, (float*)x.adj.p, (float*)d_negd.p, (uint8_t*)d_kept.p,
                       (AdaptOpPrep*)d_prep.p);
    hipLaunchKernelGGL(sample_adapt_op_kernel, dim3(n_draws), dim3(SMP_THREADS), 0, nullptr, (const float*)x.adj.p, vocab,
                       (const ExtCtl*)x.blk.p, (const DfaCtl*)d.blk.p, (const AdaptCtl*)d_ablk.p,
                       (const AdaptOpPrep*)d_prep.p, (uint32_t)pos0, d_tok, d_tok + nd, (uint32_t*)d_tok + 2 * nd,
                       (float*)d_mu.p);
    AdaptOpPrep hp;
    hipError_t e = op_wait();
    op_out(e, tokens_out, d_tok, nd * sizeof(int));
    op_out(e, n_kept_out, d_tok + nd, nd * sizeof(int));
    op_out(e, next_state_out, d_tok + 2 * nd, nd * sizeof(uint32_t));
    op_out(e, mu_out, d_mu.p, nd * sizeof(float));
    op_out(e, kept_out, d_kept.p, V);
    op_out(e, thr_out ? &hp : nullptr, d_prep.p, sizeof hp);
    if (e != hipSuccess) return set_err(nullptr, XH_E_HIP, "sample_adapt op failed: %s", hipGetErrorString(e));
    if (thr_out) *thr_out = hp.ap.thr;
    return 0;
}

int xh_decode_sample_seq(xh_ctx* ctx, int pos, int n_steps, const xh_sampling* sampling, const xh_logit_ctl* ctl,
                         const xh_trunc_ctl* trunc, const xh_seq_ctl* seq, const int* history, int n_history, int constrain,
                         uint32_t state_in, float mu_in, int stop_a, int stop_b, int* tokens_out, float* logprobs_out,
                         uint32_t* state_out, float* mu_out, int* n_done) {
    return decode_run(ctx, {STEP_SAMPLE_SEQ, pos, n_steps, sampling, ctl, trunc, seq, history, n_history, constrain, state_in,
                            mu_in, stop_a, stop_b, tokens_out, logprobs_out, state_out, mu_out, n_done});
}

int xh_op_sample_seq(const float* logits, int vocab, const xh_sampling* sampling, const xh_logit_ctl* ctl,
                     const xh_trunc_ctl* trunc, const xh_seq_ctl* seq, const int* window, int n_window,
                     const xh_byte_dfa* dfa, const uint8_t* bytes, const uint32_t* offsets, uint32_t state, float mu,
                     int stop_a, int stop_b, uint64_t pos0, int n_draws, int* tokens_out, int* n_kept_out,
                     uint32_t* next_state_out, float* mu_out, float* adjusted_out, int* rep_out, int* ng_out,
                     uint8_t* kept_out, int* xtc_fired_out) {
    if (int rc = op_check(STEP_SAMPLE_SEQ, logits, vocab, sampling, n_draws,
                          tokens_out && n_kept_out && next_state_out && mu_out, ctl, window, n_window, trunc, mu, seq, dfa,
                          bytes, offsets, state, stop_a, stop_b))
        return rc;
    const AdaptCtl ablk = adapt_block(*trunc, mu, dfa != nullptr);
    std::vector<int> brk;
    const SeqCtl sblk = seq_block(*seq, &brk);
    const size_t V = (size_t)vocab, nd = (size_t)n_draws;
    ExtStage x;
    DfaStage d;
    DevBuf d_negd, d_snap, d_rep, d_kept, d_rows, d_krows, d_ablk, d_sblk, d_brk, d_prep, d_out, d_mu;
    if (!x.stage(logits, vocab, *sampling, ctl, window, n_window) || !d_negd.alloc(V * 4) || !d_snap.alloc(V * 4) ||
        !d_rep.alloc(2 * V * sizeof(int)) || !d_kept.alloc(V) || !d_rows.alloc(nd * V * 4) || !d_krows.alloc(nd * V) ||
        !d_ablk.alloc(sizeof ablk, &ablk, sizeof ablk) || !d_sblk.alloc(sizeof sblk, &sblk, sizeof sblk) ||
        !d_brk.alloc(XH_SEQ_MAX_BREAKERS * sizeof(int), brk.data(), brk.size() * sizeof(int)) ||
        !d_prep.alloc(sizeof(AdaptOpPrep)) || !d_out.alloc(4 * nd * sizeof(int)) || !d_mu.alloc(nd * sizeof(float)) ||
        !d.stage(dfa, bytes, offsets, vocab, state, stop_a, stop_b))
        return op_stage_failed();
    if (hipMemset(d_rep.p, 0, 2 * V * sizeof(int)) != hipSuccess) return set_err(nullptr, XH_E_HIP, "hipMemset failed");
    int* d_tok = (int*)d_out.p;
    hipLaunchKernelGGL(sample_seq_prep_kernel, dim3(1), dim3(SMP_THREADS), 0, nullptr, (const float*)x.logits.p, vocab,
                       (const ExtCtl*)x.blk.p, (const DfaCtl*)d.blk.p, (const AdaptCtl*)d_ablk.p, (const SeqCtl*)d_sblk.p,
                       (const int*)x.ring.p, (const int*)x.btok.p, (const float*)x.bval.p, (const int*)d_brk.p,
                       (float*)x.adj.p, (float*)d_negd.p, (float*)d_snap.p, (int*)d_rep.p, (int*)d_rep.p + V,
                       (uint8_t*)d_kept.p, (AdaptOpPrep*)d_prep.p);
    hipLaunchKernelGGL(sample_seq_op_kernel, dim3(n_draws), dim3(SMP_THREADS), 0, nullptr, (const float*)x.adj.p,
                       (const uint8_t*)d_kept.p, (float*)d_rows.p, (uint8_t*)d_krows.p, vocab, (const ExtCtl*)x.blk.p,
                       (const DfaCtl*)d.blk.p, (const AdaptCtl*)d_ablk.p, (const SeqCtl*)d_sblk.p,
                       (const AdaptOpPrep*)d_prep.p, (uint32_t)pos0, d_tok, d_tok + nd, (uint32_t*)d_tok + 2 * nd,
                       (float*)d_mu.p, d_tok + 3 * nd);
    hipError_t e = op_wait();
    op_out(e, tokens_out, d_tok, nd * sizeof(int));
    op_out(e, n_kept_out, d_tok + nd, nd * sizeof(int));
    op_out(e, next_state_out, d_tok + 2 * nd, nd * sizeof(uint32_t));
    op_out(e, mu_out, d_mu.p, nd * sizeof(float));
    op_out(e, xtc_fired_out, d_tok + 3 * nd, nd * sizeof(int));
    op_out(e, adjusted_out, d_snap.p, V * 4);
    op_out(e, rep_out, d_rep.p, V * sizeof(int));
    op_out(e, ng_out, (int*)d_rep.p + V, V * sizeof(int));
    op_out(e, kept_out, d_krows.p, nd * V);
    if (e != hipSuccess) return set_err(nullptr, XH_E_HIP, "sample_seq op failed: %s", hipGetErrorString(e));
    return 0;
}


int xh_op_top_logprobs(const float* logits, int vocab, int n_rows, int n_top, const int* targets, int* ids_out,
                       float* lps_out, float* target_lp_out, int* target_rank_out) {
    if (const char* why = top_args_error(logits, vocab, n_rows, n_top, 1, targets, ids_out, lps_out, target_lp_out,
                                         target_rank_out))
        return set_err(nullptr, XH_E_INVALID, "%s", why);
    DevBuf d_logits, d_tgt, d_ids, d_lps, d_tlp, d_rank;
    const size_t rows = (size_t)n_rows, top = rows * (size_t)n_top;
    if (!d_logits.alloc(rows * vocab * 4, logits, rows * vocab * 4) || !d_ids.alloc(top * sizeof(int)) ||
        !d_lps.alloc(top * sizeof(float)) ||
        (targets && (!d_tgt.alloc(rows * sizeof(int), targets, rows * sizeof(int)) || !d_tlp.alloc(rows * sizeof(float)) ||
                     !d_rank.alloc(rows * sizeof(int)))))
        return op_stage_failed();
    launch_top_logprobs((const float*)d_logits.p, vocab, (size_t)vocab, n_rows, nullptr, n_top, nullptr, 0,
                        (const int*)d_tgt.p, n_top, (int*)d_ids.p, (float*)d_lps.p, (float*)d_tlp.p, (int*)d_rank.p, nullptr);
    hipError_t e = op_wait();
    op_out(e, ids_out, d_ids.p, top * sizeof(int));
    op_out(e, lps_out, d_lps.p, top * sizeof(float));
    op_out(e, targets ? target_lp_out : nullptr, d_tlp.p, rows * sizeof(float));
    op_out(e, targets ? target_rank_out : nullptr, d_rank.p, rows * sizeof(int));
    if (e != hipSuccess) return set_err(nullptr, XH_E_HIP, "top_logprobs op failed: %s", hipGetErrorString(e));
    return 0;
}


int xh_set_top_logprobs(xh_ctx* ctx, int n_top) {
    if (!ctx) return XH_E_INVALID;
    if (n_top < 0 || n_top > XH_TOP_MAX || n_top > ctx->c.vocab_size)
        return set_err(ctx, XH_E_INVALID, "n_top %d outside 0 .. min(%d, vocab)", n_top, XH_TOP_MAX);
    if (n_top > 0 && ctx->c.vocab_size > SMP_MAX_VOCAB) return set_err(ctx, XH_E_INVALID, "vocab_size > %d", SMP_MAX_VOCAB);
    HIP_TRY(ctx, hipSetDevice(ctx->dev));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (n_top > 0 && !ctx->top_ids) {
        const size_t cap = (size_t)ctx->dec_cap;
        int rc;
        if ((rc = dmalloc(ctx, &ctx->top_n_dev, (size_t)1)) || (rc = dmalloc(ctx, &ctx->top_lps, cap * XH_TOP_MAX)) ||
            (rc = dmalloc(ctx, &ctx->top_rank, cap)) || (rc = dmalloc(ctx, &ctx->top_tlp, cap)) ||
            (rc = dmalloc(ctx, &ctx->top_ids, cap * XH_TOP_MAX)))  // top_ids last: it marks the set as whole
            return rc;
    }
    if (n_top > 0) HIP_TRY(ctx, copy_sync(ctx, ctx->top_n_dev, &n_top, sizeof(int), hipMemcpyHostToDevice));
    // the decode graphs hold the row kernel's launch or do not: 0 <-> positive captures anew
    if ((ctx->top_n > 0) != (n_top > 0)) drop_graphs(ctx);
    ctx->top_n = n_top;
    ctx->top_steps = -1;
    return 0;
}

int xh_get_top_logprobs(xh_ctx* ctx, int n_steps, int* ids_out, float* lps_out, int* rank_out) {
    if (!ctx || n_steps < 0) return XH_E_INVALID;
    if (ctx->top_n <= 0 || ctx->top_steps < 0)
        return set_err(ctx, XH_E_STATE, "no decode call since xh_set_top_logprobs set a positive n_top");
    if (n_steps > ctx->top_steps)
        return set_err(ctx, XH_E_INVALID, "n_steps %d exceeds the %d steps of the last decode call", n_steps, ctx->top_steps);
    if (n_steps == 0) return 0;
    HIP_TRY(ctx, hipSetDevice(ctx->dev));
    const size_t rows = (size_t)n_steps, n = (size_t)ctx->top_n;
    std::vector<int> ids(ids_out ? rows * XH_TOP_MAX : 0);
    std::vector<float> lps(lps_out ? rows * XH_TOP_MAX : 0);
    if (ids_out) HIP_TRY(ctx, hipMemcpyAsync(ids.data(), ctx->top_ids, ids.size() * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    if (lps_out) HIP_TRY(ctx, hipMemcpyAsync(lps.data(), ctx->top_lps, lps.size() * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    if (rank_out) HIP_TRY(ctx, hipMemcpyAsync(rank_out, ctx->top_rank, rows * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t r = 0; r < rows; r++) {
        if (ids_out) std::copy_n(ids.begin() + r * XH_TOP_MAX, n, ids_out + r * n);
        if (lps_out) std::copy_n(lps.begin() + r * XH_TOP_MAX, n, lps_out + r * n);
    }
    return 0;
}

int xh_philox4x32(uint64_t seed, uint64_t pos, uint32_t out[4]) {
    if (!out) return set_err(nullptr, XH_E_INVALID, "null argument");
    out[0] = (uint32_t)pos;  // the counter's first word is pos mod 2^32, the other three are 0
    out[1] = out[2] = out[3] = 0;
    philox4x32_10((uint32_t)seed, (uint32_t)(seed >> 32), out);
    return 0;
}

int xh_get_logits(xh_ctx* ctx, float* logits_out) {
    if (!ctx || !logits_out) return XH_E_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->dev));
    HIP_TRY(ctx, hipMemcpyAsync(logits_out, ctx->logits, (size_t)ctx->c.vocab_size * 4, hipMemcpyDeviceToHost,
                                ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

}  // extern "C"
