/*
 * xalm_hip.h — C ABI of the MI355X (gfx950) single-batch decode path.
 *
 * This is the drop-in boundary for Xalm's per-token forward pass.  The reference C++ API it
 * replaces (all paths under jubruckne/Xalm @ 2025-03-21):
 *
 *   void Model::forward(const InferenceState& s, int token, int pos,
 *                       InferenceMode mode = OUTPUT_LOGITS) const;      src/model.h:272
 *     -> Model::_forward_cpu                                             src/infer.cpp:604-638
 *     -> Block::block / _block_cpu                                       src/model.cpp:37-46,
 *                                                                        src/infer.cpp:365-496
 *   struct InferenceState { x, xb, xb2, hb, hb2, q, k, v, att, logits }  src/model.h:96-156
 *   Model::from_xalm (host Tensor buffers, per-layer KV caches)          src/model.cpp:48-118
 *   enum class Device { CPU }  (the `-d` switch)                         src/model.h:21-23
 *   Exposed-for-tests ops: attn / mha_cpu / mha_cuda / matmul            src/model.h:286-316
 *
 * Conventions: plain pointers and sizes only; every call returns 0 on success or a
 * nonzero XH_E* code; xh_last_error() gives a message.  One host thread per context; a
 * context is one live sequence (as the reference Model: KV and scratch are shared).
 * Weights are COPIED into device memory by xh_upload (the caller keeps ownership).
 */
#ifndef XALM_HIP_H
#define XALM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- element types: the reference `Type` ids (src/types.h:505-514) ------------------ */
enum xh_dtype {
    XH_F32 = 1,
    XH_F16 = 2,
    XH_BF16 = 3,
    XH_F8_E4M3 = 6,
    XH_F8_E5M2 = 7,
    XH_U8 = 8,
    XH_Q8 = 9, /* int8 * 0.01f, src/types.h:423-424 */
    /* The converter's gguf blocks (convert.py:176-187 `--type q8_0 / q4_0`, quants.py): 32
     * elements per block, an f16 scale d first.  Q8_0 (quants.py:441-463): 34 B = d + 32
     * int8, value d*q.  Q4_0 (quants.py:281-311): 18 B = d + 16 bytes, byte j holding element
     * j (low nibble) and j+16 (high nibble), value d*(nibble-8).  Tensors are uploaded in that
     * file layout ([rows][cols/32 blocks], header shape = bytes per row); the reference C++
     * runtime cannot parse them (src/types.h:468-499), so the ids are this build's.
     * The affine and 5-bit blocks (`--type q4_1 / q5_0 / q5_1`), nibbles as Q4_0, bit j of the
     * little-endian u32 qh the fifth bit of element j, every value ONE f32 rounding
     * fmaf(d, q, m) (quants.py evaluates (d*q) + m in float32 and d*q is exact):
     *   Q4_1 (quants.py:316-350): 20 B = d, f16 m, 16 bytes;          value d*q + m, q = 0..15
     *   Q5_0 (quants.py:353-393): 22 B = d, u32 qh, 16 bytes;         value d*(q-16), q = 0..31
     *   Q5_1 (quants.py:396-438): 24 B = d, f16 m, u32 qh, 16 bytes;  value d*q + m, q = 0..31
     * XH_OPT_FUSE_ATTN_WO 1: the fused attention + Wo kernel has no block instantiation; a
     * layer whose Wo is any of the block types takes the two-launch route.
     * MXFP4: OCP microscaling FP4, the 4-bit format gfx950 decodes in hardware
     * (v_cvt_scalef32_pk_f32_fp4).  17 B = e (E8M0), 16 bytes of e2m1 codes in Q4_0's nibble order
     * (ggml's block_mxfp4).  Code c has sign c >> 3 and magnitude {0, 0.5, 1, 1.5, 2, 3, 4, 6}[c & 7]
     * (code 8 is -0); a weight is exactly value(c) * 2^(e - 127).  e = 255 (NaN) is invalid: every
     * upload route answers XH_E_INVALID for a tensor that holds one; every other e, 0 and 254
     * included, is valid (a product that overflows f32 is outside the contract).  Columns in whole
     * 32-element blocks, header shape = bytes per row, as for the other blocks.
     * gguf K-quants: super-blocks of 256 consecutive elements of a row (little-endian; columns in
     * whole super-blocks, header shape = bytes per row).
     *   Q4_K (quants.py Q4_K.dequantize_blocks): 144 B = f16 d, f16 dmin, s[12], qs[128].  Sub-block
     *     j (0..7, elements 32j..32j+31) has the 6-bit fields
     *       j < 4:  sc = s[j] & 63,                           mn = s[j+4] & 63
     *       j >= 4: sc = (s[j+4] & 15) | (s[j-4] >> 6) << 4,  mn = (s[j+4] >> 4) | (s[j] >> 6) << 4
     *     element 64g + l (l 0..31) the low nibble q of qs[32g + l], element 64g + 32 + l the high
     *     one; a weight is fmaf(d*sc, q, -(dmin*mn)): both products exact, ONE f32 rounding.
     *   Q6_K (quants.py Q6_K.dequantize_blocks): 210 B = ql[128], qh[64], int8 sc[16], f16 d.
     *     Element e = 128h + 32k + l (h 0..1, k 0..3, l 0..31) has the code q = nibble k >> 1 of
     *     ql[64h + 32(k & 1) + l] | (bits 2k..2k+1 of qh[32h + l]) << 4; a weight is
     *     (d*sc[e / 16]) * (q - 32), exact in f32.
     * The decode matvecs, the embedding gather and the prompt passes (the f32-input MFMA kernel, as
     * Q4_1 / Q5_1) run both; a Wo of either takes the two-launch route like every block type. */
    XH_Q8_0 = 20,
    XH_Q4_0 = 21,
    XH_Q4_1 = 22,
    XH_Q5_0 = 23,
    XH_Q5_1 = 24,
    XH_MXFP4 = 25,
    XH_Q4_K = 26,
    XH_Q6_K = 27
};

/* ---- tensor kinds (names as in .xalm, src/model.cpp:83-114) ------------------------ */
enum xh_tensor_kind {
    XH_EMBED = 0,      /* embed.weight          [vocab, dim]              */
    XH_ATTN_NORM = 1,  /* l.N.attn.norm.weight  [dim]                     */
    XH_FFN_NORM = 2,   /* l.N.mlp.norm.weight   [dim]                     */
    XH_WQ = 3,         /* l.N.attn.q.weight     [n_heads*head_dim, dim]   */
    XH_WK = 4,         /* l.N.attn.k.weight     [n_kv_heads*head_dim, dim]*/
    XH_WV = 5,         /* l.N.attn.v.weight     [n_kv_heads*head_dim, dim]*/
    XH_WO = 6,         /* l.N.attn.down.weight  [dim, n_heads*head_dim]   */
    XH_W1 = 7,         /* l.N.mlp.gate.weight   [hidden_dim, dim]         */
    XH_W2 = 8,         /* l.N.mlp.down.weight   [dim, hidden_dim]         */
    XH_W3 = 9,         /* l.N.mlp.up.weight     [hidden_dim, dim]         */
    XH_FINAL_NORM = 10,/* output.norm.weight    [dim]                     */
    XH_WCLS = 11,      /* output.weight (or embed.weight if tied) [vocab, dim] */
    XH_NUM_KINDS = 12
};

/* InferenceMode, src/model.h:249-252 */
enum xh_mode { XH_HYDRATE_KV_CACHE = 0, XH_OUTPUT_LOGITS = 1 };
/* ActivationType, src/model.h:12-15 */
enum xh_act { XH_ACT_GELU = 0, XH_ACT_SILU = 1 };

enum xh_status {
    XH_OK = 0,
    XH_E_INVALID = 1,   /* bad argument / shape / dtype mismatch (reference: throw invalid_argument) */
    XH_E_HIP = 2,       /* HIP runtime error */
    XH_E_STATE = 3,     /* call out of order, e.g. forward before all weights uploaded */
    XH_E_NOMEM = 4
};

/* POD mirror of `Config` (src/model.h:25-91); max_seq_len already resolved (cap 4096 or -T). */
typedef struct xh_config {
    int32_t dim;
    int32_t hidden_dim;
    int32_t head_dim;
    int32_t n_layers;
    int32_t n_heads;
    int32_t n_kv_heads;
    int32_t vocab_size;
    int32_t max_seq_len;
    float rope_theta;
    int32_t rotary_dim;
    float norm_eps;
    int32_t act;            /* enum xh_act */
    float qkv_clip;         /* FLT_MAX when absent (src/model.h:84-85) */
    int32_t tie_word_embeddings;
} xh_config;

typedef struct xh_ctx xh_ctx;

/* Create a device context on HIP device `device_ordinal`: allocates the fp16 KV rings
 * (2 * n_layers * max_seq_len * n_kv_heads*head_dim) and the device InferenceState. */
int xh_create(const xh_config* cfg, int device_ordinal, xh_ctx** out);

/* xh_create with the KV rings' element type: XH_F16 (exactly xh_create) or XH_F8_E4M3, anything else
 * XH_E_INVALID.  An fp8 (e4m3) context keeps one byte per element in rings of the same
 * [slot][kv_dim] shape: half the bytes the attention streams per step, twice the context in the
 * same memory.  head_dim must be a multiple of 16.  Every K/V writer stores
 * xh_f8_e4m3_from_f32 of the value the fp16 ring would round to fp16; the attention decodes the
 * codes with the gfx950 converter and computes in f32 as ever.
 * The two sink rows of K (slots 0 and 1), which the reference re-rotates every step past the ring
 * wrap, are kept per layer in an fp16 master [2][kv_dim]: the rotation reads and writes the master
 * (the fp16 ring's arithmetic exactly) and ring slot r is rewritten as the e4m3 rounding of master
 * row r, so the fp8 rounding does not accumulate over the rotations.  At all times ring K slot r
 * equals f8(master[r]).
 * Routing on an fp8 context (the stored xh_option values are untouched and read back as set):
 *   decode:  every layer takes the two-launch route (attention, then Wo), as a layer with a
 *            block-type Wo does; the fused attention + Wo launch has no fp8 instantiation.
 *   prompts: the GEMMs as ever; the attention as under XH_OPT_PREFILL_ATTN 0 (the per-token
 *            split kernel) unless XH_OPT_PREFILL_ATTN_KV8 is 1, under which it follows
 *            XH_OPT_PREFILL_ATTN and XH_OPT_PREFILL_ATTN_SPLIT as on an fp16 context (the MFMA
 *            kernels' fp8 form); either way no ring passes unless XH_OPT_PREFILL_RING_KV8: a
 *            prompt that reaches past the ring is batched below max_seq_len and takes the
 *            per-token loop from the cut (xh_prefill_route answers accordingly, the same under
 *            both values). */
int xh_create_kv(const xh_config* cfg, int device_ordinal, int kv_dtype, xh_ctx** out);
/* The context's KV element type: XH_F16 or XH_F8_E4M3. */
int xh_kv_dtype(const xh_ctx* ctx);
void xh_destroy(xh_ctx* ctx);
const char* xh_last_error(const xh_ctx* ctx); /* ctx may be NULL: last create error */

/* Copy one host tensor (`bytes` must equal shape*elem size) to the device.  `layer` is
 * ignored for embed/final_norm/wcls.  Shape and dtype are validated against the config
 * (mirrors the load_tensor checks, src/model.cpp:62-81).  Matrices of one layer that
 * the kernels fuse (q/k/v, gate/up) must share one dtype. */
int xh_upload(xh_ctx* ctx, int tensor_kind, int layer, int dtype, const void* host, size_t bytes);

/* The same upload read straight from a file: `bytes` at absolute `offset` of `path` (a
 * .xalm tensor, convert.py:248-321; the reference reads it into a host Tensor first,
 * src/xalm.h:90-192, src/model.cpp:48-118).  The range is memory-mapped, pinned for the
 * copy and moved by one DMA; no host copy of the tensor is made.  Same validation as
 * xh_upload, plus the range must lie inside the file.  Synchronous. */
int xh_upload_file(xh_ctx* ctx, int tensor_kind, int layer, int dtype, const char* path, uint64_t offset,
                   size_t bytes);

/* Benchmark weights without a checkpoint: fill the tensor slot on the device with the
 * deterministic values of include/xalm_synth.h (element i of the logical [rows][cols]
 * tensor = xs_value(seed, i, mean, std) rounded to `dtype`).  The CPU baseline builds the
 * bit-identical host copy from the same header.  Q8 is not supported. */
int xh_upload_synthetic(xh_ctx* ctx, int tensor_kind, int layer, int dtype, uint64_t seed, float mean, float std);
/* The converter's block quantizer on the host (no context, no device): n_blocks * 32 floats ->
 * n_blocks blocks of `dtype` (any of the five XH_Q*_* block types) in the file layout, the bytes
 * quants.py `quantize` writes.  It is the quantizer of the synthetic weights
 * (include/xalm_synth.h).  XH_E_INVALID for another dtype or a null pointer.
 * XH_MXFP4: per block amax = max|v|; amax == 0 gives e = 0 and all codes 0; else
 * E = clamp(floor(log2(amax)) - 2, -127, 127) from the f32 exponent bits (a subnormal amax exactly),
 * e = E + 127, each code the sign plus the e2m1 magnitude nearest to |v| * 2^-E (an exact product),
 * ties to the even code, above 6 saturating at 6.  A non-finite input: XH_E_INVALID.
 * XH_Q4_K / XH_Q6_K: n_blocks counts SUPER-blocks (256 floats in, 144 / 210 bytes out each).  The
 * reference ships no quantizer for them; this one (xs_quant_q4_k / xs_quant_q6_k, xalm_synth.h) is a
 * plain min / max quantizer, every f32 operation rounded on its own, f16 by round-to-nearest-even
 * saturating at 65504, rnd(t) = floorf(t + 0.5f):
 *   Q4_K: per sub-block j  lo_j = min(0, min v), a_j = (max v - lo_j) / 15, b_j = 0 - lo_j;
 *         d = f16(max_j a_j / 63), dmin = f16(max_j b_j / 63);  sc_j = min(63, rnd(a_j / d)) (0 when
 *         d == 0), mn_j = min(63, rnd(b_j / dmin)) likewise;  with D = d*sc_j, M = dmin*mn_j:
 *         q = clamp(rnd((v + M) / D), 0, 15), 0 when D == 0.  So dmin*mn >= 0, as ggml has it.
 *         Error of element v of sub-block j against its decoded weight w:
 *           |v - w| <= max(d*sc_j / 2, 8*d + dmin) * (1 + 2^-16) + 2^-14
 *         (half a step of the sub-block's grid; or, where q or a 6-bit field clamps, the roundings
 *         of sc_j (15 * d/2), of mn_j (dmin/2) and of d / dmin to f16: 2^-12 relative, 2^-25 absolute).
 *   Q6_K: per 16-element group g  a_g = max|v| / 31;  d = f16(max_g a_g / 127);
 *         sc_g = min(127, rnd(a_g / d)) (0 when d == 0);  with D = d*sc_g:
 *         q = clamp(floorf(v / D + 32.5f), 0, 63), 0 when D == 0 (the weight is 0 whatever q is).
 *           |v - w| <= max(d*sc_g / 2, 17*d) * (1 + 2^-16) + 2^-13
 *   Both: every output field is in range and d / dmin are finite; 256 zeros give an all-zero
 *   super-block; a non-finite input: XH_E_INVALID. */
int xh_quantize_blocks(int dtype, const float* values, size_t n_blocks, void* out);
/* The inverse on the host: n_blocks blocks of a block dtype in the file layout -> n_blocks * 32
 * floats, each the value the kernels decode (d*q, d*(q - bias), fmaf(d, q, m); MXFP4:
 * ldexpf(value(c), e - 127), so e = 0 yields the f32 subnormals exactly).  XH_E_INVALID for a
 * non-block dtype, a null pointer or an MXFP4 block with e = 255.  XH_Q4_K / XH_Q6_K: n_blocks counts
 * super-blocks (n_blocks * 256 floats out), the values as defined at the enum. */
int xh_dequantize_blocks(int dtype, const void* blocks, size_t n_blocks, float* out);
/* Fill KV ring rows [slot0, slot0+n_slots) of one layer with synthetic fp16 N(0, std)-like values. */
int xh_kv_fill_synthetic(xh_ctx* ctx, int layer, int which, int slot0, int n_slots, uint64_t seed, float std);

/* One token of Model::forward (src/model.cpp:120-122 / src/infer.cpp:604-638).
 * kv_sink/kv_pos/kv_len follow src/infer.cpp:611-613.  logits_out: caller-owned host
 * float[vocab] (may be NULL; required for nothing).  Synchronous. */
int xh_forward(xh_ctx* ctx, int token, int pos, int mode, float* logits_out);

/* Greedy decode fully on device: starting from the current logits (left by the last
 * OUTPUT_LOGITS forward at position pos-1), repeat n_steps times:
 *   tok = argmax(logits) (Sampler::sample_argmax semantics, src/sampler.cpp:19-30);
 *   tokens_out[i] = tok; forward(tok, pos + i, OUTPUT_LOGITS).
 * No host round trip per token (one graph replay per step).  If stop_token_a/b >= 0 the
 * host stops after the step that produced one of them; returns the count in *n_done. */
int xh_decode_greedy(xh_ctx* ctx, int pos, int n_steps, int stop_token_a, int stop_token_b,
                     int* tokens_out, int* n_done);

/* ---- seeded temperature / top-k / top-p sampling ------------------------------------ */
typedef struct xh_sampling {
    float    temperature;  /* >= 0; 0 = greedy                          */
    int32_t  top_k;        /* >= 0; 0 = off                             */
    float    top_p;        /* in (0, 1]; 1 = off                        */
    uint64_t seed;
} xh_sampling;
/* The token at position `pos` is drawn from logits l[0..V) as follows.
 * - Greedy.  temperature == 0 gives exactly Sampler::sample_argmax: the first maximum among
 *   logits > FLT_MIN, else token 0.  top_k, top_p and seed are ignored.
 * - Weights.  Otherwise let m = max l and w_i = exp((l_i - m) / temperature), evaluated in f32
 *   with expf.  A -inf logit has weight 0 and is never drawn.  If no logit is finite, the token
 *   is 0.  NaN logits are outside the contract.
 * - Order.  Sort by logit descending, then index ascending.  Equal logits compare by their f32
 *   bits, so the order is exact.
 * - top-k.  With top_k > 0, keep the first min(top_k, V) tokens in that order.  Ties at the k-th
 *   logit go to the lower index.
 * - top-p.  With top_p < 1, among the kept tokens in that order, keep the shortest prefix whose
 *   weight reaches top_p x the kept total.  At least one token is always kept.
 * - Draw.  Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter (pos, 0, 0, 0).
 *   u = (x0 >> 8) * 2^-24, which lies in [0, 1).  The token is the first kept token in
 *   ascending index order whose cumulative kept weight exceeds u x the final kept total.  The
 *   counter is the position the sampled token will occupy.  A sequence therefore continues
 *   identically whether it is generated in one call or in several.
 * - Invalid parameters.  Negative or NaN temperature, top_k < 0, top_p outside (0, 1] or NaN, or
 *   a null pointer return XH_E_INVALID.  This is checked before the device is touched.
 * - Determinism.  The same logits bits, parameters and counter give the same token on every
 *   run, with graphs on or off.
 * How the device evaluates it (xalm_amd/csrc/sample.h): the weights as integers, w_i * 2^40
 * truncated (a sum of them is exact in any order), the top-p cut at the first prefix whose mass
 * reaches ceil(top_p * kept mass), the draw at the first cumulative mass above floor(u * final
 * kept mass).  Against the definition in exact arithmetic that moves a cut or a draw by less
 * than V * 2^-40 of the total, plus expf's error.  The vocabulary is at most 2^17 tokens. */

/* Sampled decode fully on device: xh_decode_greedy's loop with the token drawn as above, step i
 * at counter pos + i.  `sampling` is copied to a device block before the first step (changing
 * it needs no new graph capture).  The first token comes from the logits on the device. */
int xh_decode_sample(xh_ctx* ctx, int pos, int n_steps, const xh_sampling* sampling, int stop_token_a,
                     int stop_token_b, int* tokens_out, int* n_done);

/* ---- repetition penalties, logit bias, min-p and log-probabilities ---------------------- */
#define XH_CTL_MAX_WINDOW 1024
#define XH_CTL_MAX_BIAS   256
typedef struct xh_logit_ctl {
    float   repeat_penalty;     /* > 0, finite; 1 = off                                   */
    float   presence_penalty;   /* finite; 0 = off                                        */
    float   frequency_penalty;  /* finite; 0 = off                                        */
    int32_t last_n;             /* 0 .. XH_CTL_MAX_WINDOW; 0 = the three penalties off    */
    float   min_p;              /* in [0, 1]; 0 = off                                     */
    int32_t n_bias;             /* 0 .. XH_CTL_MAX_BIAS                                   */
    const int32_t* bias_token;  /* n_bias distinct ids in [0, vocab)                      */
    const float*   bias_value;  /* finite, or -inf (ban)                                  */
} xh_logit_ctl;
/* The extended draw: xh_sampling's definition applied to adjusted logits l', plus min-p.
 * - Window.  At step i of a call the token for position pos + i is drawn.  The window is the
 *   last min(last_n, n_history + i) entries of history ++ generated[0..i).  `history` holds the
 *   n_history tokens at positions pos - n_history .. pos - 1; the caller supplies it (the context
 *   does not record prompts; only its last XH_CTL_MAX_WINDOW entries can matter), it is copied to
 *   the device once per call, and generated tokens join the window on the device.  c_t is the
 *   number of occurrences of token t in the window.
 * - Adjusted logits.  Every operation below is one IEEE f32 operation rounded once (no fused
 *   multiply-add).  A token with a bias entry gets a = l_t + b_t, any other a = l_t.  With
 *   c_t > 0:  r = (a > 0) ? a / repeat_penalty : a * repeat_penalty;
 *             r = r - (float)c_t * frequency_penalty   (the product rounded, then the difference);
 *             l' = r - presence_penalty.
 *   With c_t == 0, l' = a.  So a token with no bias entry and c_t == 0 keeps l_t bit for bit (-0
 *   included: the sampler orders by f32 bits).  -inf stays -inf; NaN or +inf produced by the
 *   adjustment is outside the contract.
 * - min-p.  With min_p > 0 and temperature > 0 let w_i = expf((l'_i - m) / temperature) in f32, m
 *   the maximum of l', and n_minp the number of tokens with w_i >= min_p (at least 1: the maximum
 *   has w = 1).  The top-k stage keeps the first min(top_k or V, n_minp) tokens of the order;
 *   top-p then works over that set as before.
 * - Greedy.  temperature == 0 is the first maximum among l' > FLT_MIN, else token 0: min_p,
 *   top_k, top_p and seed are ignored, penalties and biases apply.
 * - Counter, Philox, determinism and "one call equals two" as xh_sampling; for the last, the
 *   second call is given history ++ the first call's tokens.
 * - Log-probability (Sampler::sample_prob, src/sampler.cpp:3-17, in log; what xh_perplexity
 *   reports): lp = (l_tok - M) - logf(sum_j expf(l_j - M)) over the RAW logits, M their maximum.
 *   No temperature, bias, penalty or cut enters it.
 * - Invalid parameters.  A field outside its stated range or NaN, a bias id duplicated or out of
 *   range, n_bias > 0 with a null array, n_history < 0, n_history > 0 with a null history, or a
 *   history token outside [0, vocab) return XH_E_INVALID before the device is touched.  A null
 *   ctl means all controls off.
 * How the device evaluates it (xalm_amd/csrc/sample_ext.h): the step head copies the raw logits to
 * a context-owned buffer, fixes the at most 1024 + 256 entries the window and the biases touch
 * (one owner thread per distinct token), and runs the sampler of xh_sampling on that buffer; the
 * logits xh_get_logits returns stay raw. */

/* xh_decode_sample's loop with the extended draw (its own step head and graph; the greedy and the
 * sampled loop are untouched).  logprobs_out (may be NULL) receives one log-probability per
 * token. */
int xh_decode_sample_ext(xh_ctx* ctx, int pos, int n_steps, const xh_sampling* sampling, const xh_logit_ctl* ctl,
                         const int* history, int n_history, int stop_token_a, int stop_token_b,
                         int* tokens_out, float* logprobs_out, int* n_done);

/* ---- regex-constrained decoding: a byte-level DFA masks the tokens ------------------------- */
#define XH_DFA_DEAD 0xFFFFu            /* no transition; also the "stuck" state */
#define XH_DFA_MAX_STATES 65535
typedef struct xh_byte_dfa {
    int32_t n_states;                  /* 1 .. XH_DFA_MAX_STATES */
    int32_t start;                     /* in [0, n_states) */
    const uint16_t* next;              /* [n_states][256]: next state or XH_DFA_DEAD */
    const uint8_t*  accept;            /* [n_states]: nonzero = the text so far may end here */
} xh_byte_dfa;
/* The constrained draw: xh_logit_ctl's definition applied to masked logits l''.
 * - Pieces.  Token t has a byte string piece[t], given once per context as a blob plus
 *   offsets[vocab + 1] (piece[t] = bytes[offsets[t] .. offsets[t + 1])), ascending from 0, at most
 *   16 MiB in all.  The host mirror fills it from the tokenizer: the vocab string, the single byte
 *   for a byte-fallback token; decode_one's strip of the space after BOS is not applied.
 * - Allowed set in state s.  A token with a non-empty piece is allowed when walking `next` from s
 *   over its bytes never meets XH_DFA_DEAD; its successor state is where the walk ends.  A token
 *   with an empty piece is never allowed.  The call's end tokens (stop_token_a / b, where >= 0) are
 *   allowed exactly when accept[s] is set, whatever their piece, and leave the state unchanged.
 * - Masked logits.  l''_t = l'_t if t is allowed, else -inf; l' are the adjusted logits of
 *   xh_logit_ctl (a null ctl: the raw logits).  Unmasked entries keep their bits.  min-p, top-k,
 *   top-p, Philox at counter pos + i and the integer-mass evaluation work on l'' exactly as
 *   xh_decode_sample_ext's on l'.  Log-probabilities stay over the raw logits.  If every allowed
 *   token carries -inf (all banned by bias), "no finite logit: the token is 0" holds as there, and
 *   the state is token 0's successor, XH_DFA_DEAD when 0 is forbidden.
 * - Greedy.  temperature == 0 takes the first token of the sampler's order (logit descending by f32
 *   bits, then index ascending) among the allowed tokens, that is top_k = 1.  The "> FLT_MIN, else
 *   token 0" rule of sample_argmax does not apply: token 0 may be forbidden.
 * - Stuck.  If no token is allowed, the step emits stop_token_a if it is >= 0, else stop_token_b,
 *   else 0, and the state becomes XH_DFA_DEAD.  In XH_DFA_DEAD every later step of the call emits
 *   that same token, without masking.  xh_regex_compile never produces such a DFA (every state
 *   reaches an accepting one, so some byte continues it, or it accepts); hand-made tables and
 *   vocabularies that lack the needed piece can.
 * - One call equals two.  The call takes state_in, the DFA's start or a previous call's state_out,
 *   and returns state_out; tokens and states are identical whether a run is one call or split
 *   anywhere (the second call given history ++ the first call's tokens, as xh_decode_sample_ext).
 * - Invalid arguments.  n_states out of range; start or state_in out of range (state_in ==
 *   XH_DFA_DEAD is accepted); a next entry that is neither < n_states nor XH_DFA_DEAD; a null
 *   table; offsets not ascending from 0; the blob over 16 MiB; a vocabulary over 2^17; a stop token
 *   >= vocab (the stuck state emits it); a constrained decode before both uploads: XH_E_INVALID
 *   before the device is touched.
 * How the device evaluates it (xalm_amd/csrc/sample_dfa.h): between the adjustment and the
 * sampler, threads stride over the vocabulary, each walking its pieces from the current state (a
 * device word the head advances) and writing -inf over forbidden tokens. */

/* Copy the pieces of the context's vocab_size tokens to the device (replacing earlier ones). */
int xh_constraint_set_vocab(xh_ctx* ctx, const uint8_t* bytes, const uint32_t* offsets);
/* Validate the DFA and copy it to the device (replacing an earlier one; no new graph capture).
 * NULL clears it. */
int xh_constraint_set(xh_ctx* ctx, const xh_byte_dfa* dfa);
/* xh_decode_sample_ext's loop with the constrained draw (its own step head and graph; the other
 * loops never read the constraint).  state_out (may be NULL) receives the state after the last
 * emitted token, state_in when n_steps is 0. */
int xh_decode_sample_dfa(xh_ctx* ctx, int pos, int n_steps, const xh_sampling* sampling, const xh_logit_ctl* ctl,
                         const int* history, int n_history, uint32_t state_in, int stop_token_a, int stop_token_b,
                         int* tokens_out, float* logprobs_out, uint32_t* state_out, int* n_done);

/* ---- truncation that adapts to the distribution: top-n-sigma, locally typical, Mirostat v2 ---- */
typedef struct xh_trunc_ctl {
    float typical_p;     /* in (0, 1]; 1 = off                         */
    float top_n_sigma;   /* >= 0, finite; 0 = off                      */
    float mirostat_tau;  /* >= 0, finite; 0 = Mirostat off             */
    float mirostat_eta;  /* > 0, finite when Mirostat is on; else ignored */
} xh_trunc_ctl;
/* The adaptive draw: xh_logit_ctl's definition with three more cuts between min-p and top-p.
 * - Input.  The logits l'': xh_logit_ctl's adjusted logits l', masked exactly as in
 *   xh_decode_sample_dfa when constrain != 0 (the state advance, the stuck rule and the end-token
 *   rule are that loop's too).  constrain != 0 without both uploads is XH_E_INVALID.
 * - Greedy.  temperature == 0 gives that loop's greedy choice (constrain == 0: xh_decode_sample_ext's,
 *   constrain != 0: xh_decode_sample_dfa's); xh_trunc_ctl takes no part and mu_out = mu_in.
 * - Masses.  Otherwise m = max l'', w_i = expf((l''_i - m) / temperature) and M_i = trunc(w_i * 2^40)
 *   as an unsigned 64-bit integer (the masses of xh_sampling's device evaluation; -inf has 0).
 * - Prefix stage.  top-k and min-p as xh_logit_ctl.  With top_n_sigma > 0, sigma is the population
 *   standard deviation of the finite l''_i, accumulated in double in two passes (the mean, then the
 *   squared deviations) in a fixed order; thr = (float)((double)m - (double)top_n_sigma * sigma);
 *   n_sigma = #{i : l''_i >= thr}, compared in f32 (the maximum always qualifies).  That set is a
 *   prefix of the order; the stage keeps the first min(top_k or V, n_minp, n_sigma) tokens.  It is
 *   taken on the logits before the temperature, as the method is defined.
 * - Typical stage (typical_p < 1), over the prefix set C.  S = sum_C M_i, an exact integer.  p_i =
 *   (float)M_i / (float)S, s_i = -logf(p_i), H = sum_C p_i s_i (a token with M_i = 0 contributes 0 and
 *   has s = +inf), d_i = |s_i - H|, all f32, the sum in a fixed order.  Order C by d ascending, ties
 *   by d's f32 bits being equal then index ascending; keep the shortest prefix of that order whose
 *   integer mass reaches ceil(typical_p * S), at least one token.  The most probable token may be
 *   dropped; a token without mass never is kept.  Which tokens are kept is decided on integers: the
 *   keys of d, the indices and the masses.
 * - top-p and the draw.  The dropped tokens become -inf in a context-owned working copy (the logits
 *   xh_get_logits returns are never written), and xh_sampling's definition runs on it with top_k
 *   off: the maximum and the masses are those of the survivors, Philox at counter pos + i.  With
 *   typical_p == 1 the draw is bit for bit xh_decode_sample_ext's / _dfa's under the effective
 *   top-k; with top_n_sigma == 0 and Mirostat off as well the loop emits exactly their tokens.
 * - Mirostat v2 (mirostat_tau > 0).  Requires top_k == 0, top_p == 1, min_p == 0 (or a null ctl),
 *   typical_p == 1 and top_n_sigma == 0 (at any temperature), else XH_E_INVALID; penalties, biases
 *   and the DFA mask apply.  S = sum M_i over all tokens, cut = (u64)ceil((double)S * exp2(-(double)mu)),
 *   n_mu = max(1, #{i : M_i >= cut}): a prefix of the order, the effective top-k.  After the draw, K
 *   the kept mass: obs = (float)(log2((double)K) - log2((double)M_tok)), mu' = mu - eta * (obs - tau),
 *   the three f32 operations rounded separately (no fused multiply-add).  mu lives in a device word
 *   the head reads and writes every step.  mu_in is finite and >= 0; the caller starts at 2 * tau (the
 *   host mirror does when none is given).  mu_out is the value after the last emitted token, mu_in
 *   when n_steps is 0.  A stuck step, XH_DFA_DEAD and a step with no finite logit leave mu unchanged.
 * - One call equals two.  Tokens, DFA states and the bits of mu are identical whether a run is one
 *   call or split anywhere; the second call is given history ++ the first call's tokens, state_out
 *   and mu_out.
 * - Invalid arguments.  A field outside its range or NaN, a null xh_trunc_ctl, mu_in negative or
 *   non-finite under Mirostat, and every invalid argument of xh_decode_sample_ext and, when
 *   constrain != 0, of xh_decode_sample_dfa: XH_E_INVALID before the device is touched.
 * - Log-probabilities stay over the raw logits; xh_set_top_logprobs records for this loop too.
 * How the device evaluates it (xalm_amd/csrc/sample_adapt.h): one 1024-thread workgroup runs the
 * adjustment, the mask, the sigma passes, the prefix selection, the typical stage (-d_i into a second
 * context-owned buffer, a mass-weighted radix selection over its keys, -inf over the dropped
 * entries), the sampler of xh_sampling and Mirostat's update.  The parameters, mu and the DFA state
 * sit in device words copied before the first step: changing them captures no new graph. */

/* xh_decode_sample_dfa's loop with the adaptive draw (its own step head and graph; the other four
 * heads are untouched).  constrain == 0: no mask, state_in is ignored and returned in state_out.
 * state_out and mu_out may be NULL. */
int xh_decode_sample_adapt(xh_ctx* ctx, int pos, int n_steps, const xh_sampling* sampling, const xh_logit_ctl* ctl,
                           const xh_trunc_ctl* trunc, const int* history, int n_history, int constrain,
                           uint32_t state_in, float mu_in, int stop_token_a, int stop_token_b, int* tokens_out,
                           float* logprobs_out, uint32_t* state_out, float* mu_out, int* n_done);
/* Host only, plain C++, no device (also what the host Sampler uses): the kept set of the adaptive
 * draw on l''[vocab] (already adjusted and masked) at temperature > 0, with the masses computed as
 * above by the host's expf.  kept_out[vocab] (may be NULL) = 1 for the tokens left after the typical
 * stage and before top-p (under Mirostat: the first n_mu tokens), *n_kept_out their number (0 when no
 * logit is finite), *thr_out the n-sigma threshold (-inf when off); any may be NULL.  With
 * Mirostat on and token >= 0, *mu_out = mu' had `token` been drawn from that set (mu when it is not in
 * it or has no mass); otherwise *mu_out = mu.  temperature == 0 is XH_E_INVALID: greedy truncates
 * nothing. */
int xh_truncate_host(const float* logits, int vocab, const xh_sampling* sampling, float min_p, const xh_trunc_ctl* trunc,
                     float mu, int token, uint8_t* kept_out, int* n_kept_out, float* thr_out, float* mu_out);

/* ---- sequence-aware sampling: DRY, no-repeat-n-gram, XTC ------------------------------------- */
#define XH_SEQ_MAX_MATCH    64     /* longest repeat DRY measures / largest n-gram */
#define XH_SEQ_MAX_BREAKERS 1024
typedef struct xh_seq_ctl {
    float   dry_multiplier;     /* >= 0, finite; 0 = DRY off                         */
    float   dry_base;           /* >= 1, finite                                      */
    int32_t dry_allowed_length; /* 1 .. XH_SEQ_MAX_MATCH                             */
    int32_t no_repeat_ngram;    /* 0 = off, else 2 .. XH_SEQ_MAX_MATCH               */
    int32_t seq_last_n;         /* 0 .. XH_CTL_MAX_WINDOW; 0 = DRY and n-gram off    */
    int32_t n_breakers;         /* 0 .. XH_SEQ_MAX_BREAKERS                          */
    const int32_t* breaker_token; /* distinct ids in [0, vocab), any order           */
    float   xtc_probability;    /* in [0, 1]; 0 = XTC off                            */
    float   xtc_threshold;      /* in (0, 1]                                         */
} xh_seq_ctl;
/* The sequence-aware draw: xh_trunc_ctl's definition with two more stages on the logits (DRY and the
 * n-gram ban) and one more cut (XTC).
 * - Window.  At step i the sequence window w[0..n) is the last min(seq_last_n, n_history + i) entries
 *   of history ++ generated[0..i): the ring of xh_logit_ctl and the same history argument.  last_n of
 *   xh_logit_ctl and seq_last_n are independent lengths over the one ring.
 * - Match length.  For a position j in [0, n-1) with w[j] == w[n-1], raw_j is the largest k with
 *   1 <= k <= min(j + 1, XH_SEQ_MAX_MATCH) and w[j-t] == w[n-1-t] for all t < k.  The match may overlap
 *   the suffix: a a a a matches itself shifted by one.  dry_j is the same with one more condition: no
 *   w[n-1-t], t < k, is a breaker (so dry_j = 0 when w[n-1] itself is one, and a breaker inside the
 *   suffix cuts dry_j there but not raw_j).  For every other j both are 0.  The token after the match
 *   is c = w[j+1]; rep_c = max_j dry_j and ng_c = max_j raw_j over the j with w[j+1] == c, 0 when
 *   there is none.
 * - DRY (dry_multiplier > 0).  For every c with rep_c >= dry_allowed_length: p = dry_multiplier, then
 *   p = p * dry_base exactly rep_c - dry_allowed_length times, each product one f32 rounding (no powf,
 *   no contraction), then l'_c = l'_c - p, one f32 subtraction.  A p that overflows to +inf gives
 *   -inf: a ban, inside the contract.
 * - no-repeat-n-gram (g = no_repeat_ngram >= 2).  Every c with ng_c >= g - 1 gets l'_c = -inf.
 *   Breakers play no part in it.
 * - Order.  Both stages run after xh_logit_ctl's adjustment (bias, then the three penalties) and
 *   before the DFA mask; DRY before the ban.  A token neither stage touches keeps its bits; -inf
 *   stays -inf.  With every token at -inf the rule "no finite logit: the token is 0" holds.
 * - Greedy.  Under temperature == 0 DRY and the ban apply as the penalties do; XTC takes no part.
 * - XTC (xtc_probability > 0, temperature > 0).  It runs after xh_trunc_ctl's typical stage and
 *   before top-p, over the set C that stage left (typical off: the prefix set).  Masses as there: m
 *   the maximum of l'', M_i = trunc(expf((l''_i - m) / T) * 2^40), S_C = sum_C M_i.  The coin: Philox
 *   under the draw's key at the draw's counter (pos + i, 0, 0, 0), word x1 (the draw keeps x0);
 *   u_x = (x1 >> 8) * 2^-24 and XTC fires iff u_x < xtc_probability, compared in f32.  When it fires,
 *   cut = (u64)ceil((double)xtc_threshold * (double)S_C) and A = {i in C : M_i >= cut}; mass is
 *   monotone in the key, so A is the first |A| tokens of C in the sampler's order.  If |A| >= 2 every
 *   token of A except its last in that order (the lowest key, and among equal keys the highest
 *   index) becomes -inf in the working copy, as does every token outside C.  top-p and the draw then
 *   run on the survivors as after the typical stage: the maximum and the masses are the survivors',
 *   and n_kept without top-p is |C| - (|A| - 1).  |C| is counted as xh_trunc_ctl's loop reports it:
 *   without top-k, min-p, n-sigma and the typical stage C is every token and |C| = vocab, the -inf
 *   entries of l'' (a DFA mask, a -inf bias, a ban) included; they carry no mass, are never in A and
 *   are never drawn.  Everything is decided on integers: keys, indices, masses.
 * - Mirostat requires xtc_probability == 0, else XH_E_INVALID, in line with its other exclusions.
 * - One call equals two.  Tokens, DFA states and mu are identical however a run is split; the second
 *   call is given history ++ the first call's tokens.
 * - Everything off.  With dry_multiplier == 0, no_repeat_ngram == 0 and xtc_probability == 0 the
 *   loop emits exactly xh_decode_sample_adapt's tokens, log-probabilities, states and mu bits.
 * - Invalid arguments.  A field outside its range or NaN (checked whether or not its stage is on), a
 *   breaker id out of range or duplicated, n_breakers > 0 with a null array, a null xh_seq_ctl, and
 *   everything xh_decode_sample_adapt rejects: XH_E_INVALID before the device is touched.
 * - Log-probabilities stay over the raw logits; xh_set_top_logprobs records for this loop too.
 * How the device evaluates it (xalm_amd/csrc/sample_seq.h): thread j of the 1024-thread workgroup
 * holds w[j] in LDS and its breaker flag (a binary search in a sorted LDS copy of the breakers),
 * walks its match back at most XH_SEQ_MAX_MATCH steps, and the lowest j of every distinct c takes
 * the maxima and writes l'_c; a barrier, then the DFA mask.  XTC sums C's masses, counts A, finds
 * its lowest key and that key's highest index in C, and writes -inf in one pass each. */

/* xh_decode_sample_adapt's loop with the sequence-aware stages (its own step head and graph; the
 * other five heads are untouched).  Arguments as there. */
int xh_decode_sample_seq(xh_ctx* ctx, int pos, int n_steps, const xh_sampling* sampling, const xh_logit_ctl* ctl,
                         const xh_trunc_ctl* trunc, const xh_seq_ctl* seq, const int* history, int n_history,
                         int constrain, uint32_t state_in, float mu_in, int stop_token_a, int stop_token_b,
                         int* tokens_out, float* logprobs_out, uint32_t* state_out, float* mu_out, int* n_done);
/* Host only, plain C++, no device (also what the host Sampler uses): DRY and the ban on
 * adjusted_in[vocab] (l' after xh_logit_ctl) under the window's last min(seq_last_n, n_window)
 * tokens.  out[vocab] = l' after both stages, rep_out / ng_out [vocab] = rep_c / ng_c; any of the
 * three may be NULL. */
int xh_seq_adjust_host(const float* adjusted_in, int vocab, const xh_seq_ctl* seq, const int* window, int n_window,
                       float* out, int* rep_out, int* ng_out);
/* Host only, plain C++: XTC on logits[vocab] (l'' as it was before the typical stage) at
 * temperature > 0 for the draw at counter pos.  kept_io[vocab]: in = the 0/1 map of C, out = C after
 * XTC; m is the maximum of logits[0..vocab) and the masses come from the host's expf.  *n_kept_out =
 * the survivors' number, *fired_out = 1 when the coin fired (whatever |A|); either may be NULL. */
int xh_xtc_host(const float* logits, int vocab, float temperature, const xh_seq_ctl* seq, uint64_t seed, uint64_t pos,
                uint8_t* kept_io, int* n_kept_out, int* fired_out);

/* ---- top-N alternative log-probabilities and ranks ------------------------------------------ */
#define XH_TOP_MAX 32
/* The top list of a logits row l[0..V), and the log-probability and rank of one of its tokens.
 * - Order.  The sampler's: logit descending by f32 bits (the key of xh_sampling's order, so +0 sorts
 *   above -0), then index ascending.
 * - Top list.  top[j], j < n_top, is the j-th token of that order.
 * - Log-probability.  lp_t = (l_t - M) - logf(sum_j expf(l_j - M)), M the row maximum: the
 *   log-probability of xh_logit_ctl, over the RAW logits only.  No temperature, bias, penalty or DFA
 *   mask enters it.  A -inf logit has lp = -inf; it still takes its place in the order when fewer
 *   than n_top logits are finite.  NaN is outside the contract.
 * - Rank.  The number of tokens that precede a token in the order, 0-based: 0 = the greedy choice.
 * - Range.  1 <= n_top <= min(XH_TOP_MAX, vocab); the vocabulary is at most 2^17, as for the sampler.
 * - Determinism.  Ids and ranks are decided in integers only (keys and indices), so they are exact.
 *   The same logits bits give the same ids, ranks and lp bits on every run, with graphs on or off.
 * - Invalid arguments.  n_top out of range, a null required pointer, a target outside [0, vocab), a
 *   vocabulary over 2^17, n < 2 for xh_score: XH_E_INVALID before the device is touched.
 * How the device evaluates it (xalm_amd/csrc/top_logprobs.h): one 1024-thread workgroup per row; the
 * maximum, the sum, a radix selection of the n_top-th key over LDS count histograms, a gather of
 * the keys above it plus the lowest indices of that key, and a sort of those at most 32 entries. */

/* Host only, plain C++, no device (also what the host Sampler uses): for each of the n_rows rows of
 * logits[n_rows][vocab], ids_out / lps_out [n_rows][n_top], and with targets[n_rows] that token's
 * target_lp_out / target_rank_out [n_rows].  targets, target_lp_out and target_rank_out are NULL
 * together or given together.  The sum is accumulated in double. */
int xh_top_logprobs_host(const float* logits, int vocab, int n_rows, int n_top, const int* targets, int* ids_out,
                         float* lps_out, float* target_lp_out, int* target_rank_out);
/* The same through the device kernel (the one the decode loops and xh_score launch) on host
 * pointers, no model and no context. */
int xh_op_top_logprobs(const float* logits, int vocab, int n_rows, int n_top, const int* targets, int* ids_out,
                       float* lps_out, float* target_lp_out, int* target_rank_out);
/* n_top > 0: every device decode loop (xh_decode_greedy, _sample, _sample_ext, _sample_dfa, _sample_adapt, _sample_seq) also
 * records, per step, the top list of the raw logits its token was chosen from and that token's
 * rank, in context-owned buffers (one launch of the row kernel beside the step head, which itself
 * is unchanged: the tokens are those of n_top = 0).  0 (the default) = off: the steps are exactly
 * those of a context that never called this.  n_top lives in a device word: changing it between
 * positive values needs no new graph capture; switching between 0 and positive recaptures. */
int xh_set_top_logprobs(xh_ctx* ctx, int n_top);
/* The first n_steps rows of the last decode call: ids_out / lps_out [n_steps][n_top], rank_out
 * [n_steps] (any may be NULL).  XH_E_STATE when no decode call has run since n_top was set (or it is
 * 0), XH_E_INVALID when n_steps exceeds the steps that call completed. */
int xh_get_top_logprobs(xh_ctx* ctx, int n_steps, int* ids_out, float* lps_out, int* rank_out);
/* Prompt scoring: xh_perplexity's passes (the same planning, every XH_OPT_PREFILL value, across the
 * ring wrap) with the row kernel as the per-row tail.  For i < n - 1, after tokens[i] at position
 * pos0 + i: logprobs_out[i] / ranks_out[i] = the log-probability and rank of tokens[i + 1],
 * top_ids_out / top_lps_out [n - 1][n_top] the top list, logits_out [n - 1][vocab] the raw logits
 * the rows were computed from ("echo logits").  n_top may be 0 (no top list); any output may be
 * NULL.  n >= 2.  Unlike xh_perplexity's probabilities these do not underflow, and the maximum is
 * the row's own. */
int xh_score(xh_ctx* ctx, const int* tokens, int n, int pos0, int n_top, float* logprobs_out, int* ranks_out,
             int* top_ids_out, float* top_lps_out, float* logits_out);

/* Hydrate: forward tokens[0..n) at positions pos0.. (HYDRATE_KV_CACHE for all but the last,
 * which computes logits if want_logits), the prompt loop of run_completion
 * (src/main.cpp:94-100) in one call.  logits_out may be NULL. */
int xh_prefill(xh_ctx* ctx, const int* tokens, int n, int pos0, int want_logits, float* logits_out);

/* Host only (no device work): how xh_prefill would run n tokens at pos0 under the context's
 * current options.  *n_batched = tokens that run in batched passes (the rest take the per-token
 * loop), *n_passes = the number of those passes; either may be NULL.  xh_prefill plans with the
 * same function.  Under XH_OPT_PREFILL 4 the pass length is known once a prompt has probed
 * hipBLASLt's plans. */
int xh_prefill_route(const xh_ctx* ctx, int n, int pos0, int* n_batched, int* n_passes);

/* Perplexity scoring, the loop of run_perplexity (src/main.cpp:243-254) in one call: forward
 * tokens[0..n-1) at positions pos0.. with logits and write probs_out[i] =
 * Sampler::sample_prob(tokens[i+1]) (src/sampler.cpp:3-17; n-1 floats, caller-owned).  The
 * logits stay on the device; with XH_OPT_PREFILL on, each pass computes every token's logits
 * with one lm_head GEMM.  n >= 2.  The caller takes log and sums, as the
 * reference does in double. */
int xh_perplexity(xh_ctx* ctx, const int* tokens, int n, int pos0, float* probs_out);

/* Debug timelines (device clock, 100 MHz; each launch overwrites).  enable bits: 2 = every
 * attention + Wo launch writes [workgroup][8] stamps (start, attention done / hand-off passed,
 * end, split known, scores done, p.V done, partial drained); 8 = every W1/W3 launch writes
 * [workgroup][4] (start, x staged, end, XCD << 32 | HW_ID); 16 = the last layer's launches and the
 * lm_head write [workgroup][4 | 8] into their own regions (tools/layer_trace.py); 0 = off,
 * -1 = unchanged.  Copies min(cap, *len) words of the trace buffer to `out` first. */
int xh_debug_trace(xh_ctx* ctx, int enable, uint64_t* out, int cap, int* len);

/* Test hook: wait for the context's stream and copy one activation buffer to the host.  which:
 * XH_READ_X the residual stream [dim], XH_READ_Q the clipped and roped q [n_heads * head_dim],
 * XH_READ_HB the GLU output [hidden_dim]; each holds what the last layer of the last step left
 * (with n_layers = 1 after one xh_forward: that layer's q, its GLU output and the final residual
 * stream).  cap = floats `out` holds; XH_E_INVALID when that is less than the buffer.  It changes
 * no kernel and no state. */
enum xh_read { XH_READ_X = 0, XH_READ_Q = 1, XH_READ_HB = 2 };
int xh_debug_read(xh_ctx* ctx, int which, float* out, size_t cap);

/* Test hook, host only (no context, no device): the launch shape the decode matvec of `role`
 * takes for weights of `dtype` (enum xh_dtype) at input length n; the launcher itself calls the
 * same selection.  role: 0 qkv (rmsnorm, clip, rope, K/V write), 1 W1/W3 (rmsnorm, GLU), 2 Wo / W2
 * (plain input, residual), 3 lm_head (rmsnorm, argmax candidates), 4 plain store (xh_op_matmul).
 * Returns enum xh_gemv_shape_id, plus XH_SHAPE_BIG_LDS when the staged input exceeds 64 KiB of
 * LDS (the launch first raises the kernel's dynamic-LDS limit); -1 for a dtype without a matvec,
 * an n that is no positive multiple of 32, or an input that does not fit the LDS at all. */
enum xh_gemv_shape_id {
    XH_SHAPE_Q384 = 0, XH_SHAPE_PF2PB = 1, XH_SHAPE_PF2P = 2, XH_SHAPE_GQ = 3, XH_SHAPE_GQL = 4, XH_SHAPE_PF2 = 5,
    XH_SHAPE_W2K = 6, XH_SHAPE_PF8 = 7, XH_SHAPE_SHORT = 8, XH_SHAPE_LONG = 9, XH_SHAPE_BIG_LDS = 16
};
int xh_gemv_shape(int role, int dtype, int n);

/* Test hook, host only (no context, no device): the path the single-token attention takes at
 * kv_len for a head shape, computed by the functions the launches themselves call (the split
 * count, the split length and its floors, the rows per round, the merge selection).  fused = 0: the
 * split launch (xh_op_mha / xh_op_mha8, and the decode step without the fused launch); fused = 1:
 * the attention side of the fused attention + Wo launch, XH_E_INVALID when no such launch exists
 * for the head shape or kv_dtype is XH_F8_E4M3.  kv_dtype: XH_F16 or XH_F8_E4M3.
 *   nsplit, T, n_active  the grid's splits per KV head, slots per split, splits holding slots
 *   step                 K/V rows per round of a split
 *   rounds_full / _last  rounds of a whole split (min(T, kv_len) slots) and of the last active one
 *   wph                  waves per q head in the softmax
 *   merge_mb, merge_nc   the in-kernel merge: 0 none (one active split, or the Wo side merges),
 *                        4 / 8 / 16 partial values per thread and round trip; (m, l) loads per lane
 *   stage                fused only: 1..4 partials merged in registers by the Wo workgroups,
 *                        5 = the heads arrive merged; 0 on the split launch */
typedef struct xh_attn_plan_t {
    int fused, nsplit, T, n_active, step, rounds_full, rounds_last, wph, merge_mb, merge_nc, stage;
} xh_attn_plan_t;
int xh_attn_plan(int head_dim, int n_heads, int n_kv_heads, int max_seq_len, int kv_dtype, int fused, int kv_len,
                 xh_attn_plan_t* out);

/* Copy the current device logits to the host. */
int xh_get_logits(xh_ctx* ctx, float* logits_out);

/* Zero the KV rings and state (a fresh sequence). */
int xh_reset(xh_ctx* ctx);

/* Direct KV ring access, for tests and for pre-filling long contexts.
 * which: 0 = key cache, 1 = value cache.  Rows are [slot][n_kv_heads*head_dim] fp16 bits. */
int xh_kv_write(xh_ctx* ctx, int layer, int which, int slot0, int n_slots, const uint16_t* host);
int xh_kv_read(xh_ctx* ctx, int layer, int which, int slot0, int n_slots, uint16_t* host);
/* The same on an fp8 context (xh_create_kv): rows of raw e4m3 codes, one byte per element.  A NaN
 * code (0x7F, 0xFF) in a write is XH_E_INVALID and nothing is written.  Writing K slots 0 or 1 also
 * sets the sink master to the exact fp16 image of the codes.  xh_kv_write / xh_kv_read return
 * XH_E_INVALID on an fp8 context, this pair on an fp16 one.  xh_kv_fill_synthetic on an fp8 context
 * stores the e4m3 rounding of the fp16 value it would have stored, and sets the master likewise. */
int xh_kv_write8(xh_ctx* ctx, int layer, int which, int slot0, int n_slots, const uint8_t* host);
int xh_kv_read8(xh_ctx* ctx, int layer, int which, int slot0, int n_slots, uint8_t* host);
/* Test hook: the layer's sink master, fp16 bits [2][kv_dim].  XH_E_INVALID on an fp16 context. */
int xh_kv_sink_read(xh_ctx* ctx, int layer, uint16_t* out);

/* The element of the fp8 KV ring, on the host in plain C++: clamp v to [-448, 448] with f32 min /
 * max, then the nearest e4m3fn value, ties to the even mantissa, subnormals down to 2^-9;
 * magnitudes below 2^-10 and the tie at 2^-10 give a zero; the sign is kept (-0 is 0x80).  NaN is
 * outside the contract.  This is the definition of what every K/V writer stores. */
int xh_f8_e4m3_from_f32(const float* in, size_t n, uint8_t* out);
/* The same through the device function the K/V writers call (the clamp, then v_cvt_pk_fp8_f32);
 * needs a device, no context.  Bit-identical to xh_f8_e4m3_from_f32 on every finite input class
 * the tests cover (all f16 values, the midpoints of adjacent codes and their neighbours, the
 * clamp's edges, the zero threshold): the converter needs no integer fallback. */
int xh_op_kv_quantize(const float* in, size_t n, uint8_t* out);

/* Bytes the forward pass reads per token: Model::active_bytes(pos), src/model.cpp:12-35. */
size_t xh_active_bytes(const xh_ctx* ctx, size_t pos);

/* Graph capture of the per-token step (default on).  Off = eager launches (debugging). */
int xh_set_graphs(xh_ctx* ctx, int enable);

/* Launch-structure variants.  XH_OPT_FUSE_ATTN_WO (default 1): 1 = attention and Wo (+ residual)
 * in one launch with an in-launch hand-off (attn_wo.h); 0 = two launches.  Same math. */
/* XH_OPT_PREFILL (default 1): xh_prefill / xh_perplexity process the prompt in passes, each
 * weight matrix streamed once per pass into a GEMM.  1 = f16 and fp8 weights on the LDS-tiled MFMA
 * GEMM (gemm16.h) in passes of up to PF_TOK_MM = 2048 tokens (fp8 matrices through their exact f16 image),
 * activations as exact f16 hi + lo pairs under a power-of-two row scale (|x - (hi + lo) / s| <=
 * 2^-22 |x|, a 22-bit mantissa where the reference's f32 has 24), products exact, f32
 * accumulation in an order fixed by the tiling (the same bits on every run); Q8_0 / Q4_0 / Q5_0
 * blocks likewise through their exact f16 hi + lo images (d*q has at most 19 significant bits);
 * the affine blocks Q4_1 / Q5_1, whose fmaf(d, q, m) is a general f32 with no exact f16 pair, take
 * the f32-input MFMA kernel under every value >= 1 (lm_head of xh_perplexity included), as bf16
 * and f32 weights do; MXFP4 (2 significant bits): a matrix whose recorded scale bytes all lie in
 * 114 <= e <= 140 (0.5 * 2^(e-127) and 6 * 2^(e-127) normal f16) goes through ONE exact f16 image
 * into gemm16.h under 1 and 4, the fp8 route, no lo half; any other MXFP4 matrix, every MXFP4
 * matrix under 2 and 3, and the lm_head of xh_perplexity / xh_score take the f32-input MFMA
 * kernel, which decodes the blocks in registers (xh_prefill_route plans by the same rule: one such
 * matrix in a layer makes the passes 64 tokens long); other weight dtypes
 * on the f32-input MFMA kernel (activations exactly as the reference) in passes of 64 tokens;
 * 2 = the split-f16 register-streaming MFMA kernel wherever the weights convert exactly to f16
 * (f16, fp8), passes of 64 tokens; 3 = f32-input MFMA only; 4 = as 1 with vendor hipBLASLt in place
 * of gemm16.h (passes of 512 tokens, the heuristic's first algorithm: deterministic per library
 * build); 0 = one forward per token (the reference's loop, src/main.cpp:94-100).  Same math per
 * token up to f32 rounding. */
/* XH_OPT_PREFILL_GLU_SPLIT (default 1): where the W2 GEMM takes split-f16 input, the GLU
 * epilogue of the W1/W3 GEMM writes those f16 hi/lo halves directly (one launch), and each
 * residual add runs in one launch with the following rmsnorm split; 0 = GLU to f32 first, then
 * split in the W2 GEMM's input pass, and residual and rmsnorm as separate launches.
 * Bit-identical results; a debug knob so tests cover both routes. */
/* XH_OPT_PREFILL_ATTN (default 1): the batched path's causal attention on MFMA tiles (32 query
 * rows x 32-slot K/V tiles per wave, running max/sum, q and p as exact f16 hi + lo pairs), the
 * K/V tiles shared by the 4 waves of a workgroup through an LDS ring (head_dim 128); 2 = the same
 * arithmetic with every wave reading its own tiles (bit-identical to 1); 0 = one workgroup per
 * token and KV head, split-KV (the decode attention's blocks).
 * Option id 4 (XH_OPT_COL_KV_MAX, removed in round 3 with the column-form attention) is no
 * longer accepted: xh_set_option / xh_get_option return XH_E_INVALID for it. */
/* XH_OPT_PREFILL_ATTN_SPLIT (default 1): under XH_OPT_PREFILL_ATTN 1, a pass too short to fill the
 * chip with (KV head, 128-row query tile) workgroups walks a long history in splits (each with its
 * own running max / sum), merged per row in split order afterwards (deterministic); 0 = one
 * workgroup walks the whole history.  Same math up to f32 rounding. */
/* XH_OPT_PREFILL_RING (default 1): a prompt that reaches past the KV ring (pos0 + n > max_seq_len)
 * is cut at position max_seq_len; the part below runs the batched passes as ever, the part from
 * there on — where the reference keeps two sink slots, writes token p to slot 2 + (p - 2) %
 * (max_seq_len - 2) and re-rotates the sink K rows every step (src/infer.cpp:608-613, :416-431) —
 * runs ring passes of at most min(pass length, max_seq_len - 2) tokens: each row attends over
 * the sinks at its own rotation count, the history its predecessors in the pass have not
 * overwritten, and the pass up to itself; the pass's K/V reach the ring after its attention.
 * Under XH_OPT_PREFILL_ATTN 1 at head_dim 128 only; other head shapes and modes, and one or two
 * tokens (alone or left over by the passes) keep the per-token loop there.  0 = any prompt that reaches
 * past the ring takes the per-token loop as a whole.  Same math up to f32 rounding; the sink
 * K rows come out bit-identical on both routes. */
/* XH_OPT_PREFILL_ATTN_KV8 (default 0): on an fp8 (e4m3) KV ring (xh_create_kv) 1 = the batched
 * path's attention follows XH_OPT_PREFILL_ATTN (1 / 2 / 0) and XH_OPT_PREFILL_ATTN_SPLIT as on an
 * fp16 context, on the MFMA kernels' fp8 form: K/V tiles loaded as codes, decoded by the gfx950
 * converter to their exact f16 image and multiplied as the fp16 kernels multiply (bit-identical to
 * the fp16 attention over that image); 0 = the attention is forced to the per-token split kernel
 * (XH_OPT_PREFILL_ATTN 0).  The pass plan (xh_prefill_route) and the K/V the passes write do not
 * depend on it.  On an fp16 context the value is stored and read back and has no effect.  Values
 * other than 0 / 1 are XH_E_INVALID.  No ring passes on an fp8 ring unless XH_OPT_PREFILL_RING_KV8. */
/* XH_OPT_PREFILL_RING_KV8 (default 0): on an fp8 (e4m3) KV ring 1 = the part of a prompt from position
 * max_seq_len on runs ring passes as on an fp16 context (XH_OPT_PREFILL_RING: the same cut, pass
 * lengths and one-or-two-token rule; xh_prefill_route answers as for an fp16 context), on the ring
 * kernels' fp8 form: the pass's K/V rows are staged as the codes the token loop would store, the
 * sinks iterate in their fp16 master and token t scores them against f8(master after t + 1
 * rotations), and the attention is the fp16 ring pass's over the f16 image of all those codes, bit
 * for bit; after the pass the master holds its last version and ring K slot r is f8(master[r]).
 * It has effect only when XH_OPT_PREFILL_ATTN_KV8, XH_OPT_PREFILL_RING and XH_OPT_PREFILL_ATTN are
 * all 1, head_dim is 128 and max_seq_len - 2 >= 2; otherwise, and on an fp16 context, the value is
 * stored and read back and has no effect.  0 = the per-token loop from the cut, as ever.  Values
 * other than 0 / 1 are XH_E_INVALID. */
enum xh_option {
    XH_OPT_FUSE_ATTN_WO = 1,
    XH_OPT_PREFILL = 2,
    XH_OPT_PREFILL_GLU_SPLIT = 3,
    XH_OPT_PREFILL_ATTN = 5,
    XH_OPT_PREFILL_ATTN_SPLIT = 6,
    XH_OPT_PREFILL_RING = 7,
    XH_OPT_PREFILL_ATTN_KV8 = 8,
    XH_OPT_PREFILL_RING_KV8 = 9
};
int xh_set_option(xh_ctx* ctx, int option, int value);
int xh_get_option(const xh_ctx* ctx, int option, int* value);

/* ---- exposed-for-tests ops (src/model.h:286-316), host pointers in/out -------------- */
/* matmul: xout[d] = W[d,n] @ x[n], W of `dtype` (src/infer.cpp:185-216). */
int xh_op_matmul(float* xout, const float* x, const void* w, int dtype, int n, int d);
/* rmsnorm (src/infer.cpp:224-251), weight of dtype F32 or BF16. */
int xh_op_rmsnorm(float* o, const float* x, const void* weight, int dtype, int size, float eps);
/* rope in place on vec[d] (src/infer.cpp:305-322). */
int xh_op_rope(float* vec, int d, int head_dim, int pos, float theta, int rotary_dim);
/* mha_cuda (src/model.h:308-313): xout[n_heads*head_dim]; kb/vb fp16 [max_seq_len][n_kv_heads*head_dim]. */
int xh_op_mha(float* xout, const uint16_t* kb, const uint16_t* vb, const float* q, int head_dim,
              int kv_len, int max_seq_len, int n_heads, int n_kv_heads);
/* The same over fp8 rings (e4m3 codes, [max_seq_len][n_kv_heads*head_dim] bytes; head_dim % 16 == 0),
 * through the launch code of an fp8 context's decode step. */
int xh_op_mha8(float* xout, const uint8_t* kb, const uint8_t* vb, const float* q, int head_dim,
               int kv_len, int max_seq_len, int n_heads, int n_kv_heads);

/* The prompt-pass GEMM of XH_OPT_PREFILL 1 (gemm16.h): y[t][r] = sum_k w[r][k] * (xh[t][k] + xl[t][k])
 * with f16 w [rows][K], f16 xh / xl [n][K] and f32 y [n][rows] (the K slices' partials summed in
 * slice order, as the prompt path's epilogue).  K % 64 == 0; ks = K slices (0: the prompt path's
 * choice for this shape).  No reference counterpart: the matmul of src/infer.cpp:104-135 over n
 * tokens at once. */
int xh_op_prompt_gemm(float* y, const uint16_t* w, const uint16_t* xh, const uint16_t* xl, int rows, int K, int n,
                      int ks);

/* The causal attention of a prompt pass (XH_OPT_PREFILL_ATTN 1 / 2; src/infer.cpp:279-301, :338) on
 * host buffers, through the launch code of the passes: q and out [n][n_heads * head_dim] f32, k and v
 * [pos0 + n][n_kv_heads * head_dim] fp16 bits with the pass's own rows in place; row t attends over
 * slots [0, pos0 + t].  mode 1: the shared-tile kernel at head_dim 128, the per-wave kernel at 64 /
 * 16 (as XH_OPT_PREFILL_ATTN 1); mode 2: the per-wave kernel.  nsplit 0: the passes' own number of
 * history splits on this device; k >= 1 forces k splits (the merge kernel behind them when k > 1):
 * mode 1 at head_dim 128 only, k <= max(1, pos0 / 64 / 4).  Head shapes: head_dim 128 / 64 with 1, 2,
 * 4 or 8 q heads per KV head, head_dim 16 with 2; anything else is XH_E_INVALID before any launch. */
int xh_op_prompt_attn(float* out, const float* q, const uint16_t* k, const uint16_t* v, int n, int pos0, int head_dim,
                      int n_heads, int n_kv_heads, int mode, int nsplit);
/* The same over fp8 K/V (an fp8 context under XH_OPT_PREFILL_ATTN_KV8 1), through the same launch
 * code: k and v [pos0 + n][n_kv_heads * head_dim] e4m3 codes, every other argument and the head
 * shapes as xh_op_prompt_attn.  By definition the result is xh_op_prompt_attn's over the codes' f16
 * image, bit for bit.  A NaN code (0x7F, 0xFF) in k or v is XH_E_INVALID before any launch, as in
 * xh_kv_write8. */
int xh_op_prompt_attn8(float* out, const float* q, const uint8_t* k, const uint8_t* v, int n, int pos0,
                       int head_dim, int n_heads, int n_kv_heads, int mode, int nsplit);
/* The attention of a ring pass (XH_OPT_PREFILL_RING; src/infer.cpp:608-613) at head_dim 128 on host
 * buffers: m tokens at positions p0.. >= max_seq_len, 3 <= m <= W = max_seq_len - 2.  k_ring / v_ring
 * [max_seq_len][kv_dim] fp16 bits: the ring as the pass finds it, and on return as the pass leaves
 * it (staging row t in slot 2 + (p0 - 2 + t) % W, sink_ver[m - 1] in K rows 0 and 1); ks / vs [m][kv_dim]
 * the pass's own rows; sink_ver [m][2][kv_dim] the sink K rows token t scores against; q and out
 * [m][n_heads * 128].  nsplit as in xh_op_prompt_attn with pos0 = W.  Launches: the window walk, the
 * merge that adds the sinks, the commit. */
int xh_op_prompt_attn_ring(float* out, uint16_t* k_ring, uint16_t* v_ring, const float* q, const uint16_t* ks,
                           const uint16_t* vs, const uint16_t* sink_ver, int m, int p0, int max_seq_len, int n_heads,
                           int n_kv_heads, int nsplit);
/* The same over fp8 K/V (an fp8 context under XH_OPT_PREFILL_RING_KV8 1), through the same launch
 * code: k_ring / v_ring, ks / vs and sink_ver hold one e4m3 code per element in the same shapes
 * (sink_ver [m][2][kv_dim] codes: f8 of the master's version token t scores against); every other
 * argument as xh_op_prompt_attn_ring, and what it rejects is rejected likewise.  By definition `out`
 * is xh_op_prompt_attn_ring's over the codes' f16 image, bit for bit, and the rings come back with
 * staging row t in slot 2 + (p0 - 2 + t) % W and sink_ver[m - 1] in K rows 0 and 1 (the hook has no
 * master).  A NaN code (0x7F, 0xFF) in any of the five code buffers is XH_E_INVALID before any
 * launch: out and the rings are untouched. */
int xh_op_prompt_attn_ring8(float* out, uint8_t* k_ring, uint8_t* v_ring, const float* q, const uint8_t* ks,
                            const uint8_t* vs, const uint8_t* sink_ver, int m, int p0, int max_seq_len,
                            int n_heads, int n_kv_heads, int nsplit);

/* One GEMM of a prompt pass on host buffers, through the launch code of the passes: y[n][rows] = x . w^T
 * with x f32 [n][K] and w [rows][K] of `dtype` in the file layout (repacked as xh_op_matmul does).  mode =
 * XH_OPT_PREFILL 1, 2 or 3 picks the route as a pass does; *route_out reports it: 0 = the row-major
 * split input of gemm16.h (f16 as stored; e4m3 / e5m2 / Q8_0 / Q4_0 / Q5_0 / MXFP4 with every scale
 * in 114 .. 140 through their f16 image), E > 0 = the fragment kernel (prefill_gemm16_kernel, E weights
 * per 16 bytes), -1 = the f32-input kernel (prefill_gemm_kernel).  Launches: prefill_split_kernel where
 * the route takes split input, the image kernel if any, the GEMM, prefill_epi_kernel with EPI_STORE
 * (times 1 / s_t on the row-major route, as a pass).  ks 0: the passes' K slicing; k >= 1 forces k slices
 * and is XH_E_INVALID unless k obeys the route's picker: a power of two, K in k slices of whole
 * 64-deep steps and k <= 8 (route 0), of whole 8E-deep rings (E > 0; -1 when K % 8E == 0, else of 2E),
 * k <= 64 and k * ceil(rows / tile) <= 1024 there.  XH_E_INVALID before any launch also for: a dtype with
 * no prompt GEMM, K % (2 * decoder chunk) != 0, n > 64 off the row-major route (n > 2048 on it), an
 * MXFP4 block with e = 255, a NULL pointer.  No reference counterpart (src/infer.cpp:104-135 over n
 * tokens at once). */
int xh_op_prompt_matmul(float* y, const float* x, const void* w, int dtype, int rows, int K, int n, int mode, int ks,
                        int* route_out);
/* The exact f16 image(s) the row-major route multiplies, by the passes' image kernels: hi_out [rows][K]
 * f16 bits for e4m3 / e5m2 (finite codes) / MXFP4 (scales in 114 .. 140) with lo_out NULL; hi_out and
 * lo_out for Q8_0 / Q4_0 / Q5_0 (w = hi + lo exactly).  w in the file layout, K % 32 == 0.  max_groups 0:
 * the passes' cap of 8192 workgroups; k >= 1 caps the grid at k, so every thread strides. */
int xh_op_prompt_weight_image(int dtype, const void* w, int rows, int K, uint16_t* hi_out, uint16_t* lo_out,
                              int max_groups);
/* The producers of a prompt GEMM's split input, and the epilogue, on given partials part [ks][n][row]
 * (summed in slice order, times part_s[t] when part_s is not NULL).  layout: 0 = row-major halves,
 * 8 / 16 = the fragment layout for that many weights per 16 bytes.  The producers need dim % 8 == 0
 * (layout 0) or dim % (2 * layout) == 0.
 *   XH_STAGE_SPLIT                 x [n][dim] -> halves                         (prefill_split_kernel)
 *   XH_STAGE_NORM_SPLIT            rmsnorm(x) * norm_w -> halves                (prefill_rmsnorm_split_kernel)
 *   XH_STAGE_RESID_NORM_SPLIT      x += partials (row = dim), then as NORM_SPLIT, one launch
 *   XH_STAGE_RESID_THEN_NORM_SPLIT the same in two: EPI_RESID, then prefill_rmsnorm_split_kernel
 *   XH_STAGE_GLU_SPLIT             act(g) * u of partials (row = 2 dim, g / u interleaved) -> halves, one launch
 *   XH_STAGE_GLU_THEN_SPLIT        the same in two: EPI_GLU, then prefill_split_kernel
 *   XH_STAGE_STORE                 EPI_STORE of partials (row = dim, any parity) into y_out [n][out_stride]
 *                                  (0: dim), which comes in as the rows to be overwritten
 * The fused kinds give the bits of their two-launch kinds.  Outputs of the producers: x (the RESID kinds:
 * updated in place), inv_s_out [n] = 1 / s_t, hi_out / lo_out [n][dim] f16 bits row-major (a fragment
 * layout gathered back through the kernels' own offset function), *pad_out = non-zero halves in the
 * padding rows n .. 32 ceil(n / 32) of a fragment layout (they start as 0xffff).  norm_w: dim weights of
 * norm_dtype XH_F32 or XH_BF16.  Arguments a kind does not use may be NULL / 0. */
enum xh_prompt_stage {
    XH_STAGE_SPLIT = 0,
    XH_STAGE_NORM_SPLIT = 1,
    XH_STAGE_RESID_NORM_SPLIT = 2,
    XH_STAGE_RESID_THEN_NORM_SPLIT = 3,
    XH_STAGE_GLU_SPLIT = 4,
    XH_STAGE_GLU_THEN_SPLIT = 5,
    XH_STAGE_STORE = 6
};
int xh_op_prompt_stage(int kind, const float* part, int ks, const float* part_s, float* x, int n, int dim,
                       const void* norm_w, int norm_dtype, float eps, int act, int layout, size_t out_stride, float* y_out,
                       float* inv_s_out, uint16_t* hi_out, uint16_t* lo_out, int* pad_out);
/* Host only, no device: weight rows per wave (route -1 or E > 0) or per workgroup (route 0) of the
 * prompt GEMM of that route, as xh_op_prompt_matmul reports it. */
int xh_prompt_gemm_tile(int route);

/* The sampler of xh_decode_sample (the same device function) on host logits[vocab], no model and
 * no context: draw d = 0 .. n_draws-1 at counter pos0 + d writes tokens_out[d] and n_kept_out[d],
 * the size of the kept set (greedy: 1; no finite logit: 0).  n_draws <= 65536. */
int xh_op_sample(const float* logits, int vocab, const xh_sampling* sampling, uint64_t pos0, int n_draws,
                 int* tokens_out, int* n_kept_out);
/* The extended draw (xh_logit_ctl above; the same device functions as xh_decode_sample_ext) on host
 * logits[vocab], no model and no context: draw d at counter pos0 + d, all draws over the same fixed
 * window (its last min(last_n, n_window) tokens); adjusted_out (may be NULL) receives l'[vocab] as
 * the device computed it, logprob_out (may be NULL) the n_draws log-probabilities. */
int xh_op_sample_ext(const float* logits, int vocab, const xh_sampling* sampling, const xh_logit_ctl* ctl,
                     const int* window, int n_window, uint64_t pos0, int n_draws,
                     int* tokens_out, int* n_kept_out, float* adjusted_out, float* logprob_out);
/* Host only, no device: the adjustment of xh_logit_ctl in plain C++ (also what the host Sampler
 * uses): out[vocab] = l' for logits[vocab] under the window's last min(last_n, n_window) tokens. */
int xh_adjust_logits(const float* logits, int vocab, const xh_logit_ctl* ctl, const int* window,
                     int n_window, float* out);
/* The constrained draw (the same device functions as xh_decode_sample_dfa) on host logits[vocab],
 * no model and no context: draw d at counter pos0 + d, every draw from `state` over the same window;
 * masked_out (may be NULL) receives l''[vocab] as the device computed it (l' when state is
 * XH_DFA_DEAD), next_state_out[n_draws] each draw's successor state, n_kept_out 0 for a stuck draw,
 * logprob_out (may be NULL) the log-probabilities. */
int xh_op_sample_dfa(const float* logits, int vocab, const xh_sampling* sampling, const xh_logit_ctl* ctl,
                     const int* window, int n_window, const xh_byte_dfa* dfa, const uint8_t* bytes,
                     const uint32_t* offsets, uint32_t state, int stop_token_a, int stop_token_b, uint64_t pos0,
                     int n_draws, int* tokens_out, int* n_kept_out, float* masked_out, uint32_t* next_state_out,
                     float* logprob_out);
/* The adaptive draw (xh_trunc_ctl above; the same device functions as xh_decode_sample_adapt) on host
 * logits[vocab], no model and no context: draw d at counter pos0 + d, every draw from `state` and `mu`
 * over the same window.  dfa NULL = unconstrained (bytes, offsets, state and the stop tokens are
 * ignored; next_state_out receives `state`).  tokens_out, n_kept_out (the final kept set's size),
 * next_state_out and mu_out hold n_draws entries each; kept_out[vocab] (may be NULL) is the 0/1 map
 * of the set after the typical stage and before top-p (all 0 for a greedy or stuck draw, or with no
 * finite logit), thr_out (may be NULL) the f32 n-sigma threshold (-inf when off). */
int xh_op_sample_adapt(const float* logits, int vocab, const xh_sampling* sampling, const xh_logit_ctl* ctl,
                       const xh_trunc_ctl* trunc, const int* window, int n_window, const xh_byte_dfa* dfa,
                       const uint8_t* bytes, const uint32_t* offsets, uint32_t state, float mu, int stop_token_a,
                       int stop_token_b, uint64_t pos0, int n_draws, int* tokens_out, int* n_kept_out,
                       uint32_t* next_state_out, float* mu_out, uint8_t* kept_out, float* thr_out);
/* The sequence-aware draw (xh_seq_ctl above; the same device functions as xh_decode_sample_seq) on host
 * logits[vocab], no model and no context; arguments as xh_op_sample_adapt, the window serving
 * xh_logit_ctl's last_n and xh_seq_ctl's seq_last_n alike.  adjusted_out [vocab] = l' after DRY and
 * the ban, before the mask; rep_out / ng_out [vocab] = rep_c / ng_c (0 for a token that follows no
 * match); kept_out [n_draws][vocab] = each draw's 0/1 map after XTC and before top-p (without a
 * removal: xh_op_sample_adapt's kept_out); xtc_fired_out [n_draws] = 1 where the coin fired, whatever
 * |A| (0 for a greedy or stuck draw).  All five may be NULL. */
int xh_op_sample_seq(const float* logits, int vocab, const xh_sampling* sampling, const xh_logit_ctl* ctl,
                     const xh_trunc_ctl* trunc, const xh_seq_ctl* seq, const int* window, int n_window,
                     const xh_byte_dfa* dfa, const uint8_t* bytes, const uint32_t* offsets, uint32_t state, float mu,
                     int stop_token_a, int stop_token_b, uint64_t pos0, int n_draws, int* tokens_out, int* n_kept_out,
                     uint32_t* next_state_out, float* mu_out, float* adjusted_out, int* rep_out, int* ng_out,
                     uint8_t* kept_out, int* xtc_fired_out);
/* Host only, no device, plain C++ (also what the host Sampler uses): allowed_out[t] = 1 if token t
 * is allowed in `state`, else 0, and next_state_out[t] its successor state (XH_DFA_DEAD when
 * forbidden); nothing is allowed in XH_DFA_DEAD. */
int xh_constraint_mask(const xh_byte_dfa* dfa, const uint8_t* bytes, const uint32_t* offsets, int vocab, uint32_t state,
                       int stop_token_a, int stop_token_b, uint8_t* allowed_out, uint16_t* next_state_out);
/* Host only, no context, no device: compile a regular expression, matched against the whole text
 * byte by byte, into a trimmed DFA: every state reaches an accepting state, and a transition into a
 * removed state is XH_DFA_DEAD.  Syntax: literal bytes (UTF-8 as its bytes); \\ \. \n \t \r \xHH
 * \d \w \s and any escaped punctuation; . (any byte but \n); [a-z], [^...] (escapes allowed, a
 * leading ] is literal); ( ), |, * + ?, {m}, {m,n}, {m,} with counts <= 256.  One quantifier per
 * atom (no lazy or stacked ones); a literal { is escaped; groups nest at most 256 deep.  Thompson NFA, subset construction, no
 * minimisation.  next [cap_states][256] and accept [cap_states] are caller-owned (may be NULL with
 * cap_states 0 to ask for the size).  XH_E_INVALID: a syntax error, the empty language, or more than
 * XH_DFA_MAX_STATES states before trimming; XH_E_NOMEM, with *n_states set: cap_states is too
 * small. */
int xh_regex_compile(const char* pattern, uint16_t* next, uint8_t* accept, int cap_states, int* n_states, int* start);
/* Philox4x32-10 on the host (no device): key (seed & 0xffffffff, seed >> 32), counter
 * (pos mod 2^32, 0, 0, 0): only the low 32 bits of pos are used. */
int xh_philox4x32(uint64_t seed, uint64_t pos, uint32_t out[4]);

/* ---- timing hooks used by bench.py (HIP events on the context's own stream) -------- */
/* Average device time (microseconds) of one launch of kernel `which` (0 = the fused
 * gate/up matvec, 1 = qkv, 2 = wo, 3 = down, 4 = lm_head, 5 = attention, 6 = the sampled step
 * head of xh_decode_sample under its last parameters, 7 = the extended step head of
 * xh_decode_sample_ext under its last parameters, 8 = the constrained step head of
 * xh_decode_sample_dfa under its last parameters, 9 = the top-N row kernel on the context's logits
 * under the current xh_set_top_logprobs width, XH_E_STATE when that is 0, 10 = the adaptive step head
 * of xh_decode_sample_adapt under its last parameters, XH_E_STATE before such a call, 11 = the
 * sequence-aware step head of xh_decode_sample_seq likewise) over `iters` back-to-back launches with
 * the current step parameters (layers rotate, so the Infinity Cache never serves a repeat).
 * 6, 7 and 8 advance the decode loop's position with every launch (7 and 8 also append to their
 * window, 8 also advances the DFA state; 10 and 11 advance what 7 and 8 do, and mu): reset or re-hydrate afterwards.  8 needs an xh_decode_sample_dfa
 * call since the last xh_constraint_set / xh_constraint_set_vocab, else XH_E_STATE. */
int xh_time_kernel(xh_ctx* ctx, int which, int iters, float* avg_us);
/* Bytes one launch of that kernel must move (algorithmic). */
size_t xh_kernel_bytes(const xh_ctx* ctx, int which, int kv_len);

#ifdef __cplusplus
}
#endif
#endif /* XALM_HIP_H */
