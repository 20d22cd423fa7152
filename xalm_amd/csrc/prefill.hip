// prefill.hip — batched prompt passes: pass buffers, the GEMM and attention dispatch of prefill.h
// and gemm16.h (this unit alone includes them: they define non-template kernels), and the ABI
// entries xh_prefill and xh_perplexity.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <vector>

#include "ctx.h"
#include "prefill.h"
#include "top_logprobs_host.h"

using namespace xalm;

namespace {

// ---------------------------------------------------------------------------------------
// batched prefill (prefill.h)
// ---------------------------------------------------------------------------------------
constexpr int PF_WAVE_TARGET = 1024;  // 1 wave per SIMD (RT=2: 2048 -16 %, 512 -38 %; fewer, longer K slices)
constexpr int PF_RT = 2;                // 32-row tiles per GEMM wave (1: -11 %, 4: -9 %)
constexpr int PF_RT16 = 4;              // 32-row tiles per split-f16 GEMM wave
constexpr size_t PF_PART_ROWS = 32 * PF_RT16 * PF_WAVE_TARGET;  // >= ks * rows (ks * ceil(rows/(32 RT)) <= target)

constexpr int PF_CLS_CHUNK = (int)(PF_PART_ROWS / 4);  // lm_head rows per GEMM (ks <= 4 fits the partials)

// partials buffer: the register-streaming MFMA kernels' K slices of 64 tokens, or up to 2 T
// token rows of partials over the widest matrix (gemm16.h K slices: ks * n <= 2 T; hipBLASLt: the
// hi and lo halves)
size_t pf_part_floats(const xh_ctx* ctx, const int T) {
    const xh_config& c = ctx->c;
    const int rows = std::max({ctx->q_dim + 2 * ctx->kv_dim, 2 * c.hidden_dim, c.dim, std::min(c.vocab_size, PF_CLS_CHUNK)});
    return std::max(PF_PART_ROWS * PF_TOK, (size_t)2 * T * rows);
}

}  // namespace

void xalm::pf_free(xh_ctx* ctx) {
    for (int g = 0; g < PfBufs::N_GROUPS; g++) ctx->pf.free_group(g);
}

namespace {

// pass buffers for T tokens (kept while later passes fit; a longer pass length reallocates)
int pf_alloc(xh_ctx* ctx, const int T) {
    PfBufs& b = ctx->pf;
    if (b.cap[PfBufs::PASS] >= T) return 0;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    pf_free(ctx);
    const xh_config& c = ctx->c;
    const size_t t = (size_t)T;
    int rc;
    if ((rc = dmalloc(ctx, &b.tok, t)) || (rc = dmalloc(ctx, &b.x, t * c.dim)) ||
        (rc = dmalloc(ctx, &b.xn, t * c.dim)) || (rc = dmalloc(ctx, &b.q, t * ctx->q_dim)) ||
        (rc = dmalloc(ctx, &b.att, t * ctx->q_dim)) || (rc = dmalloc(ctx, &b.h, t * c.hidden_dim)) ||
        (rc = dmalloc(ctx, &b.part, pf_part_floats(ctx, T))) || (rc = dmalloc(ctx, &b.sp, t)))
        return rc;
    // xh: the split-kernel fragments of <= 64 tokens, or hi rows then lo rows of a row-major
    // pass input (gemm16.h / hipBLASLt); xl: the split kernel's lo fragments
    const size_t kmax = std::max({(size_t)c.dim, (size_t)c.hidden_dim, (size_t)ctx->q_dim});
    if ((rc = dmalloc(ctx, &b.xh, 2 * std::max(t, (size_t)PF_TOK) * kmax)) ||
        (rc = dmalloc(ctx, &b.xl, PF_TOK * kmax)) || (rc = dmalloc(ctx, &b.xs, std::max(t, (size_t)PF_TOK))))
        return rc;
    b.cap[PfBufs::PASS] = T;
    return 0;
}

// A group beside the pass buffers, allocated on its first use and sized for the pass: the
// per-token split attention's partials (XH_OPT_PREFILL_ATTN 0), a ring pass's staging rows and
// sink versions, a perplexity pass's logits and targets.  Keeps dmalloc's code and message.
int pf_alloc_group(xh_ctx* ctx, const int g) {
    PfBufs& b = ctx->pf;
    if (b.cap[g] >= b.cap[PfBufs::PASS]) return 0;
    b.free_group(g);
    const size_t t = (size_t)b.cap[PfBufs::PASS];
    int rc = 0;
    auto get = [&](auto** p, const size_t n) {
        if (!rc) rc = dmalloc(ctx, p, n);
    };
    if (g == PfBufs::ATTN0) {
        get(&b.po, t * ctx->nsplit * ctx->q_dim);
        get(&b.pml, t * ctx->nsplit * ctx->c.n_heads * 2);
        get(&b.cnt, t * ctx->c.n_kv_heads);
    } else if (g == PfBufs::RING) {
        // rows of the ring's element type (an fp8 ring: kv_dim codes, kv_dim / 2 uint16_t)
        const size_t row = ctx->kv_dim * ctx->kv_esz() / 2;
        get(&b.ks, t * row);
        get(&b.vs, t * row);
        get(&b.sinkv, t * 2 * row);
        if (ctx->kv8()) get(&b.sinkm, (size_t)2 * ctx->kv_dim);
    } else {
        get(&b.logits, t * ctx->c.vocab_size);
        get(&b.tgt, t);
    }
    if (!rc) b.cap[g] = b.cap[PfBufs::PASS];
    return rc;
}

// The model's GEMMs: W [rows][K] of decode form dt.  A layer's four in launch order, and the
// lm_head (all vocab_size rows; it runs in chunks of PF_CLS_CHUNK).
// wide: an MXFP4 matrix that takes no f16 image (a scale byte outside [MX_E_F16_LO, MX_E_F16_HI]:
// the upload's *_x flag; the lm_head always): the f32-input MFMA kernel decodes it in registers.
struct PfMat { const char* what; int dt; const void* w; int K, rows; bool wide; };
enum { PF_QKV, PF_WO, PF_W13, PF_W2 };
std::array<PfMat, 4> pf_layer_mats(const xh_ctx* ctx, const int l) {
    const xh_config& c = ctx->c;
    const LayerW& w = ctx->L[l];
    return {{{"qkv", kdt(w.qkv_dt, w.qkv_x), w.wqkv, c.dim, ctx->q_dim + 2 * ctx->kv_dim, w.qkv_x},
             {"wo", kdt(w.wo_dt, w.wo_x), w.wo, ctx->q_dim, c.dim, w.wo_x},
             {"w1/w3", kdt(w.w13_dt, w.w13_x), w.w13, c.dim, 2 * c.hidden_dim, w.w13_x},
             {"w2", kdt(w.w2_dt, w.w2_x), w.w2, c.hidden_dim, c.dim, w.w2_x}}};
}
PfMat pf_cls_mat(const xh_ctx* ctx) {
    return {"lm_head", kdt(ctx->wcls_dt, ctx->wcls_x), ctx->wcls, ctx->c.dim, ctx->c.vocab_size, true};
}
// every layer's GEMMs, then one lm_head chunk
std::vector<PfMat> pf_all_mats(const xh_ctx* ctx) {
    std::vector<PfMat> gs;
    for (int l = 0; l < (int)ctx->L.size(); l++)
        for (const PfMat& g : pf_layer_mats(ctx, l)) gs.push_back(g);
    gs.push_back(pf_cls_mat(ctx));
    gs.back().rows = std::min(PF_CLS_CHUNK, gs.back().rows);
    return gs;
}

// K slices for a GEMM of `rows` outputs: about PF_WAVE_TARGET waves, K divisible into whole
// chunk pairs
int pf_ks(int rows, int K, int E) {
    const int n_rt = (rows + 32 * PF_RT - 1) / (32 * PF_RT);
    int ks = 1;
    // slices stay whole multiples of 4 chunk pairs (the pipelined kernel) where K allows
    const int unit = K % (8 * E) == 0 ? 8 * E : 2 * E;
    while (ks < 64 && (size_t)2 * ks * n_rt <= PF_WAVE_TARGET && K % (2 * ks * unit) == 0) ks *= 2;
    return ks;
}

template <int DT>
void pf_gemm_t(const PfGemmArgs& a, hipStream_t s) {
    const int waves = (a.rows + 32 * PF_RT - 1) / (32 * PF_RT) * a.ks;
    constexpr int E = WDec<DT>::E;
    const dim3 grid((waves + PF_WAVES - 1) / PF_WAVES);
    if ((a.K / a.ks) % (8 * E) == 0)
        hipLaunchKernelGGL((prefill_gemm_kernel<DT, true, PF_RT>), grid, dim3(PF_THREADS), 0, s, a);
    else
        hipLaunchKernelGGL((prefill_gemm_kernel<DT, false, PF_RT>), grid, dim3(PF_THREADS), 0, s, a);
}
// split-f16 GEMM: K slices of whole 4-stage rings (8E), about PF_WAVE_TARGET waves, partials fit
int pf_ks16(int rows, int K, int E) {
    if (K % (8 * E)) return 0;
    const int n_rt = (rows + 32 * PF_RT16 - 1) / (32 * PF_RT16);
    int ks = 1;
    while (ks < 64 && (size_t)2 * ks * n_rt <= PF_WAVE_TARGET && K % (2 * ks * 8 * E) == 0) ks *= 2;
    while (ks > 1 && (size_t)ks * rows > PF_PART_ROWS) ks /= 2;
    return (size_t)ks * rows <= PF_PART_ROWS ? ks : 0;
}
template <int DT>
void pf_gemm16_t(const PfGemm16Args& a, hipStream_t s) {
    const int waves = (a.rows + 32 * PF_RT16 - 1) / (32 * PF_RT16) * a.ks;
    hipLaunchKernelGGL((prefill_gemm16_kernel<DT, PF_RT16>), dim3((waves + PF_WAVES - 1) / PF_WAVES), dim3(PF_THREADS),
                       0, s, a);
}
// weights the f16 GEMMs take: f16 as stored, e4m3 / e5m2 through their exact f16 image (kdt
// keeps the _EXACT dtypes, whose NaN / Inf codes the reference decodes to finite values, off it)
bool pf_f8(int dt) { return dt == XH_F8_E4M3 || dt == XH_F8_E5M2; }
bool pf_f16w(int dt) { return dt == XH_F16 || pf_f8(dt); }
// Does the GEMM of p run on the row-major split input: gemm16.h (XH_OPT_PREFILL 1: K in whole
// 64-deep steps) or hipBLASLt (4: a plan for every shape)?
bool pf_lay0(const PfGemmPlan& p) {
    const int dt = p.dt, K = p.K;
    // MXFP4 (2 significant bits): ONE exact f16 image, the fp8 route (XH_OPT_PREFILL 1 and 4), when
    // every scale byte of the matrix lies in [MX_E_F16_LO, MX_E_F16_HI]; else (wide) the f32-input
    // MFMA kernel, as under XH_OPT_PREFILL 2 and 3
    if (gq_mx(dt)) {
        if (p.wide || K % 32) return false;
        if (p.mode == 1) return K % MM_KMULT == 0;
        return p.mode == 4 && p.blas;
    }
    // gguf blocks: their exact f16 hi + lo images through gemm16.h (XH_OPT_PREFILL 1); the affine
    // blocks (fmaf(d, q, m): no exact f16 pair) always take the f32-input MFMA kernel
    if (gq_affine(dt) || gq_k(dt)) return false;  // the K-quants likewise (Q6_K: up to 24 significant bits)
    if (gq_dt(dt)) return p.mode == 1 && K % MM_KMULT == 0;
    if (!pf_f16w(dt)) return false;
    if (p.mode == 1) return K % MM_KMULT == 0;
    if (p.mode == 4) return p.blas;
    return false;
}
// the plan of a GEMM of this context (n, the partials and a forced slicing left to the caller)
PfGemmPlan pf_plan_of(const xh_ctx* ctx, int dt, int K, int rows, bool wide) {
    PfGemmPlan p{};
    p.mode = ctx->prefill_gemm;
    p.blas = p.mode == 4 && blas_ok(ctx) > 0;
    p.dt = dt; p.K = K; p.rows = rows; p.wide = wide;
    p.n_cu = ctx->n_cu;
    return p;
}
bool pf_lay0(const xh_ctx* ctx, int dt, int K, bool wide) { return pf_lay0(pf_plan_of(ctx, dt, K, 0, wide)); }
// Once per prefill: (XH_OPT_PREFILL 4, once per context) does hipBLASLt have an f16 plan for every
// full-pass GEMM of the model (if not, every dtype keeps the MFMA kernels); and the f16 image
// buffer of the largest fp8 matrix that goes to the f16 GEMMs.
int pf_prepare(xh_ctx* ctx) {
    const std::vector<PfMat> gs = pf_all_mats(ctx);
    if (ctx->prefill_gemm == 4 && !blas_ok(ctx)) {
        int ok = 1;
        for (const PfMat& g : gs) {
            if (!pf_f16w(g.dt) && !(gq_mx(g.dt) && !g.wide)) continue;
            bool have = false;
            int rc = blas_has_plan(ctx, g.rows, g.K, 2 * PF_TOK_BLAS, &have);
            if (rc) return rc;
            if (!have) ok = -1;
        }
        blas_set_ok(ctx, ok);
    }
    size_t wdq = 0;  // fp8: one f16 image; gguf blocks: hi and lo images
    for (const PfMat& g : gs)
        if ((pf_f8(g.dt) || gq_dt(g.dt)) && pf_lay0(ctx, g.dt, g.K, g.wide))
            wdq = std::max(wdq, (size_t)g.rows * g.K * (gq_dt(g.dt) && !gq_mx(g.dt) ? 2 : 1));
    if (wdq > ctx->pf_wdq_elems) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        hipFree(ctx->pf_wdq);
        ctx->pf_wdq = nullptr;
        ctx->pf_wdq_elems = 0;
        int rc = dmalloc(ctx, &ctx->pf_wdq, wdq);
        if (rc) return rc;
        ctx->pf_wdq_elems = wdq;
    }
    return 0;
}
// Layout of the split-f16 input of the GEMM over W (dtype dt, [rows][K]): pf_gemm_route of its plan
int pf_layout(const xh_ctx* ctx, int dt, int K, int rows, bool wide) {
    return pf_gemm_route(pf_plan_of(ctx, dt, K, rows, wide));
}
// split-f16 halves of a pass's rows: hi into pf.xh; lo into pf.xl (fragments) or right after
// the hi rows (row-major)
uint16_t* pf_lo(xh_ctx* ctx, int layout, int n, int K) { return pf_split_lo(layout, n, K, ctx->pf.xh, ctx->pf.xl); }
// grid of the split kernels: one workgroup per token row, fragments padded to 32-token tiles
int pf_split_grid(int layout, int n) { return layout ? 32 * ((n + 31) / 32) : n; }
int pf_layout(const xh_ctx* ctx, const PfMat& g) { return pf_layout(ctx, g.dt, g.K, g.rows, g.wide); }
// Tokens per pass: PF_TOK_MM (gemm16.h) / PF_TOK_BLAS (hipBLASLt) when every layer GEMM takes the
// row-major input (the lm_head of a perplexity pass aside: it runs on 64-token slices when it
// cannot), else 64 (the register-streaming MFMA kernels' two token tiles)
int pf_pass_tokens(const xh_ctx* ctx) {
    for (int l = 0; l < (int)ctx->L.size(); l++)
        for (const PfMat& g : pf_layer_mats(ctx, l))
            if (!pf_lay0(ctx, g.dt, g.K, g.wide)) return PF_TOK;
    return ctx->prefill_gemm == 4 ? PF_TOK_BLAS : PF_TOK_MM;
}
// One pass of prefill_batched: m tokens at positions p0.. (ring: all >= max_seq_len), and what one
// launch leaves for the next.  scaled: the last pf_gemm's partials carry 1 / s_t (pf.xs);
// split_ready: the next GEMM's split input is already in pf.xh (pf_norm, pf_resid_norm, pf_glu).
struct PfPass { int m, p0; bool ring; bool scaled; bool split_ready; };
// rmsnorm of the pass's rows (pf.x) as the input of the GEMM g (K = dim): written straight into
// the split-f16 halves when that GEMM takes a split input (one launch)
void pf_norm(xh_ctx* ctx, PfPass& ps, const void* nw, int ndt, const PfMat& g) {
    const xh_config& c = ctx->c;
    PfBufs& b = ctx->pf;
    const int lay = pf_layout(ctx, g);
    if (lay >= 0) {
        pf_norm_split_launch(b.x, c.dim, nw, ndt, c.norm_eps, ps.m, lay, b.xh, pf_lo(ctx, lay, ps.m, c.dim), b.xs,
                             ctx->stream);
        ps.split_ready = true;
    } else {
        pf_norm_launch(b.x, c.dim, nw, ndt, c.norm_eps, ps.m, b.xn, ctx->stream);
    }
}
// one prompt GEMM launch (gemm16.h): the 4-wave instantiation when the launch has at least
// MM_W4_PER_CU workgroups per CU, else the default
void mm_launch(const MmArgs& a, int n_cu, hipStream_t s) {
    const int grid = a.n_rt * a.n_tt * a.ks;
    if (grid >= MM_W4_PER_CU * n_cu) {
        ensure_lds((const void*)mm_f16_kernel_w4, MM_LDS_W4);
        hipLaunchKernelGGL(mm_f16_kernel_w4, dim3(grid), dim3(MM_THREADS_W4), MM_LDS_W4, s, a);
    } else {
        ensure_lds((const void*)mm_f16_kernel, MM_LDS);
        hipLaunchKernelGGL(mm_f16_kernel, dim3(grid), dim3(MM_THREADS), MM_LDS, s, a);
    }
}
struct PfGemmF32 {  // for_dt: the f32-input MFMA kernel of a dtype
    const PfGemmArgs& a; hipStream_t s;
    template <int DT> int run() const { pf_gemm_t<DT>(a, s); return 0; }
};
// a launch body's refusal (PF_GEMM_E_*) as the pass's error
int pf_gemm_err(xh_ctx* ctx, int rc, const PfMat& g, int n) {
    switch (rc) {
        case PF_GEMM_E_IMAGE: return set_err(ctx, XH_E_INVALID, "prefill: %s weight image does not fit", g.what);
        case PF_GEMM_E_FIT:
            return set_err(ctx, XH_E_INVALID, "prefill: %s GEMM %d x %d over %d tokens does not fit", g.what, g.rows, g.K, n);
        case PF_GEMM_E_DTYPE: return set_err(ctx, XH_E_INVALID, "prefill: %s dtype %d not supported", g.what, g.dt);
        default: return set_err(ctx, XH_E_INVALID, "prefill: %s shape not supported", g.what);
    }
}
// Y partials of g's W[rows][K] . X[n][K] into pf.part ([ks][n][rows]).  Split-f16 paths convert x
// first unless ps.split_ready says its halves are there already.  0 or an error code.  The launches
// are the context-free bodies below (pf_gemm_*); hipBLASLt (XH_OPT_PREFILL 4) alone needs the context.
int pf_gemm(xh_ctx* ctx, PfPass& ps, const PfMat& g, const float* x, int n, int& ks) {
    PfBufs& b = ctx->pf;
    PfGemmPlan p = pf_plan_of(ctx, g.dt, g.K, g.rows, g.wide);
    p.n = n;
    p.part_floats = pf_part_floats(ctx, b.cap[PfBufs::PASS]);
    const PfGemmIo io{g.w, x, b.xh, b.xl, b.xs, ctx->pf_wdq, ctx->pf_wdq_elems, b.part};
    const int lay = pf_gemm_route(p);
    ps.scaled = false;
    if (lay >= 0) {
        if (!ps.split_ready) pf_split_launch(x, g.K, n, lay, b.xh, pf_lo(ctx, lay, n, g.K), b.xs, ctx->stream);
        ps.split_ready = false;
    }
    int rc;
    if (lay == 0) {
        // row-major hi rows then lo rows; partials unscaled, the epilogue multiplies by 1 / s_t
        const uint16_t *w_hi = nullptr, *w_lo = nullptr;
        if ((rc = pf_gemm_images(p, io, &w_hi, &w_lo, ctx->stream))) return pf_gemm_err(ctx, rc, g, n);
        ps.scaled = true;
        if (ctx->prefill_gemm == 4) {
            // hi and lo rows as one B operand of 2n columns: partials [2][n][rows]; a pass length
            // hipBLASLt has no algorithm for runs on gemm16.h instead (same layout, same bound)
            bool have = false;
            rc = blas_has_plan(ctx, g.rows, g.K, 2 * n, &have);
            if (rc) return rc;
            if (have || g.K % MM_KMULT) {
                rc = blas_gemm(ctx, w_hi, g.K, g.rows, b.xh, 2 * n, b.part);
                if (rc) return rc;
                ks = 2;
                return 0;
            }
        }
        rc = pf_gemm_rowmajor(p, io, w_hi, w_lo, &ks, ctx->stream);
    } else if (lay > 0) {
        rc = pf_gemm_frag(p, io, lay, &ks, ctx->stream);
    } else {
        rc = pf_gemm_f32(p, io, &ks, ctx->stream);
    }
    return rc ? pf_gemm_err(ctx, rc, g, n) : 0;
}
void pf_epi_launch(const PfEpiArgs& e, hipStream_t s) {
    const int threads = e.n * ((e.rows + 1) / 2);
    hipLaunchKernelGGL(prefill_epi_kernel, dim3((threads + 255) / 256), dim3(256), 0, s, e);
}
void pf_epi(xh_ctx* ctx, const PfPass& ps, PfEpiArgs e) {
    e.part = ctx->pf.part;
    e.part_s = ps.scaled ? ctx->pf.xs : nullptr;
    pf_epi_launch(e, ctx->stream);
}
// x += the last GEMM's partials (EPI_RESID), then the rmsnorm of the updated rows as the input of
// the GEMM g (K = dim): one launch when that GEMM takes the split input and the rows fit the
// LDS, else pf_epi + pf_norm (the same bits either way)
int pf_resid_norm(xh_ctx* ctx, PfPass& ps, int ks, const void* nw, int ndt, const PfMat& g) {
    const xh_config& c = ctx->c;
    PfBufs& b = ctx->pf;
    const int lay = pf_layout(ctx, g);
    const size_t lds = (size_t)c.dim * sizeof(float);  // + the kernel's static red[4]
    if (lay >= 0 && ctx->pf_resid_norm && c.dim % 8 == 0 && lds + 4 * sizeof(float) <= 64 * 1024) {
        HIP_TRY(ctx, hipGetLastError());  // an earlier launch's error is reported as such
        pf_resid_norm_split_launch(b.part, ks, ps.scaled ? b.xs : nullptr, b.x, c.dim, nw, ndt, c.norm_eps, ps.m, lay, b.xh,
                                   pf_lo(ctx, lay, ps.m, c.dim), b.xs, ctx->stream);
        HIP_TRY(ctx, hipGetLastError());
        ps.split_ready = true;
        return 0;
    }
    PfEpiArgs e{};
    e.ks = ks; e.n = ps.m; e.rows = c.dim; e.epi = EPI_RESID; e.out = b.x;
    pf_epi(ctx, ps, e);
    pf_norm(ctx, ps, nw, ndt, g);
    return 0;
}
// h = act(g) * u of the W1/W3 partials (EPI_GLU) as the input of the W2 GEMM: straight into its
// split-f16 halves in one launch when it takes a split input and a row of h fits the LDS (the
// launch's only precondition, so any error here is real), else into pf.h
int pf_glu(xh_ctx* ctx, PfPass& ps, int ks, const PfMat& w2) {
    const xh_config& c = ctx->c;
    PfBufs& b = ctx->pf;
    const int lay = pf_layout(ctx, w2);
    // dynamic LDS = one f32 row of h; the kernel adds a static 16-float reduction array
    const size_t lds = (size_t)c.hidden_dim * sizeof(float);
    if (lay >= 0 && ctx->pf_glu_split && lds + 16 * sizeof(float) <= 64 * 1024) {
        // part_s and inv_s are both pf.xs: a workgroup reads its token's factor before the
        // barrier and writes the new one after it
        HIP_TRY(ctx, hipGetLastError());  // an earlier launch's error is reported as such
        pf_glu_split_launch(b.part, ks, ps.scaled ? b.xs : nullptr, ps.m, c.hidden_dim, c.act, lay, b.xh,
                            pf_lo(ctx, lay, ps.m, c.hidden_dim), b.xs, ctx->stream);
        HIP_TRY(ctx, hipGetLastError());
        ps.split_ready = true;
        return 0;
    }
    PfEpiArgs e{};
    e.ks = ks; e.n = ps.m; e.rows = 2 * c.hidden_dim; e.epi = EPI_GLU; e.out = b.h; e.act = c.act;
    pf_epi(ctx, ps, e);
    return 0;
}
template <int HD, int QPK, int KV>
void pf_attn_t(xh_ctx* ctx, const AttnArgs& a, int n) {
    const size_t smem = attn_smem_bytes(HD, QPK, ctx->t_max, a.nsplit);
    auto k = prefill_attn_kernel<HD, QPK, KV>;
    if (smem > 64 * 1024) ensure_lds((const void*)k);
    hipLaunchKernelGGL(k, dim3(ctx->c.n_kv_heads, a.nsplit, n), dim3(ATTN_THREADS), smem, ctx->stream, a,
                       (const StepParams*)ctx->pf.sp, ctx->q_dim, ctx->c.n_kv_heads);
}
// History splits of the shared-tile prompt attention: a pass whose (KV head, query tile)
// workgroups cannot fill two per CU (a short pass: 8 workgroups for <= 32 tokens at 8 KV heads)
// walks its history in up to that many splits of >= FA_MIN_SPLIT_STAGES ring stages each (the
// split partials live in pf.part, free between the qkv epilogue and the Wo GEMM).
constexpr int FA_MIN_SPLIT_STAGES = 4;
// query tiles of the shared-tile kernels: PF_FA_WAVES waves of 32 / qpk tokens each
int fa2_query_tiles(int n, int qpk) {
    const int per = PF_FA_WAVES * (32 / qpk);
    return (n + per - 1) / per;
}
// head shapes of the batched path's attention: head_dim 128 / 64 with 1, 2, 4 or 8 q heads per KV
// head (MHA through GQA), and the test fixtures' head_dim 16 x 2
constexpr bool pf_attn_shape(int hd, int qpk) {
    return ((hd == 128 || hd == 64) && (qpk == 1 || qpk == 2 || qpk == 4 || qpk == 8)) || (hd == 16 && qpk == 2);
}
// One causal prompt attention on device pointers, the launch body of the passes and of
// xh_op_prompt_attn: the shared-tile kernel (shared: head_dim 128 only) over nsplit history splits
// with the merge behind it when nsplit > 1 (partials in `part`), else the per-wave kernel.
// KV: the element type behind kc / vc (XH_F8_E4M3: one code per element).
template <int HD, int QPK, int KV>
void pf_fa_t(const PfAttnDims& d, bool shared, const float* q, const uint16_t* kc, const uint16_t* vc, float* out, int n,
             int pos0, int nsplit, float* part, hipStream_t s) {
    constexpr int TPW = 32 / QPK;
    const int q_dim = d.n_heads * HD, kv_dim = d.n_kv_heads * HD;
    if constexpr (HD == 128) {
        if (shared) {
            constexpr int NW = PF_FA_WAVES;
            auto k = prefill_fa2_kernel<QPK, NW, KV>;
            ensure_lds((const void*)k);
            const int nqt = fa2_query_tiles(n, QPK);
            float* po = nsplit > 1 ? part : nullptr;
            float2* pml = nsplit > 1 ? (float2*)(part + (size_t)nsplit * n * q_dim) : nullptr;
            hipLaunchKernelGGL(k, dim3(d.n_kv_heads, nqt, nsplit), dim3(64 * NW), fa_lds_bytes(), s, q, kc, vc, out, n, pos0,
                               q_dim, kv_dim, po, pml);
            if (nsplit > 1)
                hipLaunchKernelGGL(prefill_fa_merge_kernel<false>, dim3(d.n_heads, n), dim3(256), 0, s, (const float*)po,
                                   (const float2*)pml, out, n, nsplit, q_dim, FaSinks{});
            return;
        }
    }
    hipLaunchKernelGGL((prefill_fa_kernel<HD, QPK, KV>), dim3(d.n_kv_heads, (n + TPW - 1) / TPW), dim3(64), 0, s, q, kc, vc, out,
                       n, pos0, q_dim, kv_dim);
}
template <int HD>
int pf_fa_hd(const PfAttnDims& d, int kv_dt, bool shared, const float* q, const uint16_t* kc, const uint16_t* vc, float* out, int n,
             int pos0, int nsplit, float* part, hipStream_t s) {
    return for_qpk(d.n_heads / d.n_kv_heads, [&](auto Q) {
        constexpr int QPK = decltype(Q)::value;
        if constexpr (pf_attn_shape(HD, QPK)) {
            if (kv_dt == XH_F8_E4M3) pf_fa_t<HD, QPK, XH_F8_E4M3>(d, shared, q, kc, vc, out, n, pos0, nsplit, part, s);
            else pf_fa_t<HD, QPK, XH_F16>(d, shared, q, kc, vc, out, n, pos0, nsplit, part, s);
            return 0;
        }
        return -1;
    });
}
// The attention of a ring pass after its sink versions, on device pointers (head_dim 128): the
// window walk into split partials, the merge that adds the sinks, the commit to the ring.
// KV: the element type behind every K/V buffer (XH_F8_E4M3: one code per element; sinkm / master:
// the fp16 master's last version and its home, both null for a ring without a master).
template <int QPK, int KV>
int pf_ring_t(const PfAttnDims& d, const float* q, uint16_t* kc, uint16_t* vc, const uint16_t* ks, const uint16_t* vs,
              const uint16_t* sinkv, float* out, int m, int p0, int max_seq_len, int nsplit, float* part, hipStream_t s,
              const uint16_t* sinkm, uint16_t* master) {
    constexpr int NW = PF_FA_WAVES;
    const int W = max_seq_len - 2;
    const int q_dim = d.n_heads * 128, kv_dim = d.n_kv_heads * 128;
    FaRing rg{ks, vs, W, (p0 - 2) % W};
    const int nqt = fa2_query_tiles(m, QPK);
    float* po = part;
    float2* pml = (float2*)(part + (size_t)nsplit * m * q_dim);
    auto k = prefill_fa2_ring_kernel<QPK, NW, KV>;
    ensure_lds((const void*)k);
    hipLaunchKernelGGL(k, dim3(d.n_kv_heads, nqt, nsplit), dim3(64 * NW), fa_lds_bytes(), s, q, (const uint16_t*)kc,
                       (const uint16_t*)vc, rg, m, q_dim, kv_dim, po, pml);
    const FaSinks sk{q, sinkv, vc, kv_dim, QPK};
    hipLaunchKernelGGL((prefill_fa_merge_kernel<true, KV>), dim3(d.n_heads, m), dim3(256), 0, s, (const float*)po,
                       (const float2*)pml, out, m, nsplit, q_dim, sk);
    hipLaunchKernelGGL(prefill_ring_commit_kernel<KV>, dim3(m + 1), dim3(256), 0, s, rg, sinkv, kc, vc, m, kv_dim, sinkm,
                       master);
    return 0;
}

}  // namespace

// ---- the prompt GEMM's launch bodies (ctx.h): what pf_gemm and the test ops both run ----------
// weights per 16-byte chunk of the f32-input MFMA kernel's decoders (WDec<DT>::E)
int xalm::pf_elems(int dt) {
    if (dt == XH_F8_E4M3_EXACT || dt == XH_F8_E5M2_EXACT || dt == XH_Q8_0) return 16;
    return gq_dt(dt) ? 32 : elems_per_16b(dt);  // the nibble blocks (Q8_0 above)
}
// 0 = row-major (gemm16.h or hipBLASLt), E > 0 = the split-f16 register-streaming kernel's
// fragments, -1 = no split (f32-input MFMA).  XH_OPT_PREFILL 1 / 4: row-major for f16 / e4m3 / e5m2
// where the GEMM fits, else the split kernel for fp8; 2: the split kernel for f16 and fp8; 3: never
// split.  The split kernel also needs a K slicing.
int xalm::pf_gemm_route(const PfGemmPlan& p) {
    if (pf_lay0(p)) return 0;
    const bool f8 = pf_f8(p.dt);
    const int m = p.mode;
    if (!(m == 2 || ((m == 1 || m == 4) && f8))) return -1;
    if (p.dt != XH_F16 && !f8) return -1;
    const int E = elems_per_16b(p.dt);
    return pf_ks16(p.rows, p.K, E) ? E : -1;
}
int xalm::pf_gemm_row_tile(int route) { return route == 0 ? MM_BR : 32 * (route > 0 ? PF_RT16 : PF_RT); }
bool xalm::pf_gemm_ks_ok(const PfGemmPlan& p, int route) {
    const int ks = p.ks, K = p.K;
    if (ks <= 0 || (ks & (ks - 1))) return false;  // every picker doubles
    if (route == 0) {                              // mm_pick_ks
        const int images = gq_dt(p.dt) && !gq_mx(p.dt) ? 2 : 1;
        return ks <= 8 && K % (ks * MM_KMULT) == 0 && (size_t)images * ks * p.n * p.rows <= p.part_floats;
    }
    const int E = route > 0 ? route : pf_elems(p.dt);
    const int rt = route > 0 ? PF_RT16 : PF_RT;
    const int n_rt = (p.rows + 32 * rt - 1) / (32 * rt);
    // pf_ks16: slices of whole rings; pf_ks: of whole rings where K allows, else of chunk pairs
    const int unit = route > 0 || K % (8 * E) == 0 ? 8 * E : 2 * E;
    if (ks > 64 || K % (ks * unit) || (ks > 1 && (size_t)ks * n_rt > PF_WAVE_TARGET)) return false;
    return (size_t)ks * p.rows <= PF_PART_ROWS && (size_t)ks * p.n * p.rows <= p.part_floats;
}
uint16_t* xalm::pf_split_lo(int lay, int n, int K, uint16_t* xh, uint16_t* xl) { return lay ? xl : xh + (size_t)n * K; }
size_t xalm::pf_split_index(int t, int k, int K, int lay) { return split_off(t, k, K, lay); }
void xalm::pf_split_launch(const float* x, int K, int n, int lay, uint16_t* xh, uint16_t* xl, float* inv_s, hipStream_t s) {
    hipLaunchKernelGGL(prefill_split_kernel, dim3(pf_split_grid(lay, n)), dim3(256), 0, s, x, K, n, lay, xh, xl, inv_s);
}
int xalm::pf_gemm_images(const PfGemmPlan& p, const PfGemmIo& io, const uint16_t** w_hi, const uint16_t** w_lo,
                         hipStream_t s) {
    const int dt = p.dt, rows = p.rows, K = p.K;
    const size_t cap = (size_t)(p.max_groups > 0 ? p.max_groups : PF_IMAGE_GROUPS);
    *w_hi = (const uint16_t*)io.w;
    *w_lo = nullptr;  // gguf blocks: the lo image, a second GEMM into more partials
    if (pf_f8(dt)) {
        // the matrix's exact f16 image first (one streaming pass: 1 B read, 2 B written per weight)
        const size_t n16 = (size_t)rows * K / 16;
        if ((size_t)rows * K > io.wdq_elems || K % 16) return PF_GEMM_E_IMAGE;
        const int grid = (int)std::min<size_t>((n16 + 255) / 256, cap);
        if (dt == XH_F8_E4M3)
            hipLaunchKernelGGL(pf_dequant_f16_kernel<XH_F8_E4M3>, dim3(grid), dim3(256), 0, s, (const u32x4*)io.w, n16,
                               (u32x4*)io.wdq);
        else
            hipLaunchKernelGGL(pf_dequant_f16_kernel<XH_F8_E5M2>, dim3(grid), dim3(256), 0, s, (const u32x4*)io.w, n16,
                               (u32x4*)io.wdq);
        *w_hi = io.wdq;
    }
    if (gq_mx(dt)) {
        // MXFP4 in the f16 range: one exact image, as fp8 (0.53 B read, 2 B written per weight)
        if ((size_t)rows * K > io.wdq_elems || K % 32) return PF_GEMM_E_IMAGE;
        const size_t chunks = (size_t)rows * K / 32;
        const int grid = (int)std::min<size_t>((chunks + 255) / 256, cap);
        hipLaunchKernelGGL(pf_dequant_mx_kernel, dim3(grid), dim3(256), 0, s, (const uint8_t*)io.w, rows, K, io.wdq);
        *w_hi = io.wdq;
    }
    if (gq_dt(dt) && !gq_mx(dt)) {
        if ((size_t)2 * rows * K > io.wdq_elems || K % 32) return PF_GEMM_E_IMAGE;
        const size_t chunks = (size_t)rows * K / 8;
        const int grid = (int)std::min<size_t>((chunks + 255) / 256, cap);
        uint16_t* hi = io.wdq;
        uint16_t* lo = io.wdq + (size_t)rows * K;
        if (dt == XH_Q8_0)
            hipLaunchKernelGGL(pf_dequant_gq_kernel<XH_Q8_0>, dim3(grid), dim3(256), 0, s, (const uint8_t*)io.w, rows, K, hi, lo);
        else if (dt == XH_Q5_0)
            hipLaunchKernelGGL(pf_dequant_gq_kernel<XH_Q5_0>, dim3(grid), dim3(256), 0, s, (const uint8_t*)io.w, rows, K, hi, lo);
        else if (dt == XH_Q4_0)
            hipLaunchKernelGGL(pf_dequant_gq_kernel<XH_Q4_0>, dim3(grid), dim3(256), 0, s, (const uint8_t*)io.w, rows, K, hi, lo);
        else
            return PF_GEMM_E_DTYPE;  // the affine blocks have no exact f16 pair
        *w_hi = hi;
        *w_lo = lo;
    }
    return PF_GEMM_OK;
}
int xalm::pf_gemm_rowmajor(const PfGemmPlan& p, const PfGemmIo& io, const uint16_t* w_hi, const uint16_t* w_lo, int* ks_out,
                           hipStream_t s) {
    const int rows = p.rows, K = p.K, n = p.n;
    const int images = w_lo ? 2 : 1;
    const size_t cap = p.part_floats;
    MmArgs a{};
    a.w = w_hi; a.xh = io.xh; a.xl = io.xh + (size_t)n * K; a.out = io.part;
    a.rows = rows; a.K = K; a.n = n; a.ks = p.ks > 0 ? p.ks : mm_pick_ks(rows, K, n, cap / images, p.n_cu);
    a.n_rt = mm_row_tiles(rows); a.n_tt = mm_tok_tiles(n);
    if (a.ks <= 0 || K % (a.ks * MM_KMULT) || (size_t)images * a.ks * n * rows > cap) return PF_GEMM_E_FIT;
    mm_launch(a, p.n_cu, s);
    if (w_lo) {  // partials [ks, 2 ks): W_lo . X, summed after W_hi's by the epilogue
        a.w = w_lo;
        a.out = io.part + (size_t)a.ks * n * rows;
        mm_launch(a, p.n_cu, s);
    }
    *ks_out = images * a.ks;
    return PF_GEMM_OK;
}
int xalm::pf_gemm_frag(const PfGemmPlan& p, const PfGemmIo& io, int lay, int* ks_out, hipStream_t s) {
    PfGemm16Args a{};
    a.w = io.w; a.row_bytes = (size_t)p.K * (16 / lay); a.K = p.K; a.rows = p.rows;
    a.xh = io.xh; a.xl = io.xl; a.inv_s = io.xs; a.n = p.n; a.ks = p.ks > 0 ? p.ks : pf_ks16(p.rows, p.K, lay);
    a.part = io.part;
    if (p.n > PF_TOK || a.ks <= 0 || p.K % (a.ks * 8 * lay)) return PF_GEMM_E_SHAPE;
    if ((size_t)a.ks * p.n * p.rows > p.part_floats) return PF_GEMM_E_FIT;
    switch (p.dt) {
        case XH_F16: pf_gemm16_t<XH_F16>(a, s); break;
        case XH_F8_E4M3: pf_gemm16_t<XH_F8_E4M3>(a, s); break;
        case XH_F8_E5M2: pf_gemm16_t<XH_F8_E5M2>(a, s); break;
        default: return PF_GEMM_E_DTYPE;
    }
    *ks_out = a.ks;
    return PF_GEMM_OK;
}
int xalm::pf_gemm_f32(const PfGemmPlan& p, const PfGemmIo& io, int* ks_out, hipStream_t s) {
    const int dt = p.dt, K = p.K, rows = p.rows;
    const int E = pf_elems(dt);
    if (K % (2 * E) || p.n > PF_TOK) return PF_GEMM_E_SHAPE;
    PfGemmArgs a{};
    a.w = io.w; a.K = K; a.rows = rows; a.x = io.x; a.n = p.n; a.part = io.part;
    a.row_bytes = gq_dt(dt) ? gq_pitch(dt, K) : (size_t)K * (16 / E);
    a.ks = p.ks > 0 ? p.ks : pf_ks(rows, K, E);
    if ((size_t)a.ks * rows > PF_PART_ROWS || K % (a.ks * 2 * E)) return PF_GEMM_E_SHAPE;
    if ((size_t)a.ks * p.n * rows > p.part_floats) return PF_GEMM_E_FIT;
    if (for_dt(dt, PfGemmF32{a, s}) < 0) return PF_GEMM_E_DTYPE;
    *ks_out = a.ks;
    return PF_GEMM_OK;
}
void xalm::pf_norm_split_launch(const float* x, int dim, const void* nw, int ndt, float eps, int n, int lay, uint16_t* xh,
                                uint16_t* xl, float* inv_s, hipStream_t s) {
    hipLaunchKernelGGL(prefill_rmsnorm_split_kernel, dim3(pf_split_grid(lay, n)), dim3(256), 0, s, x, dim, nw, ndt, eps, n, lay,
                       xh, xl, inv_s);
}
void xalm::pf_norm_launch(const float* x, int dim, const void* nw, int ndt, float eps, int n, float* o, hipStream_t s) {
    hipLaunchKernelGGL(prefill_rmsnorm_kernel, dim3(n), dim3(256), 0, s, x, dim, nw, ndt, eps, o);
}
void xalm::pf_resid_norm_split_launch(const float* part, int ks, const float* part_s, float* x, int dim, const void* nw,
                                      int ndt, float eps, int n, int lay, uint16_t* xh, uint16_t* xl, float* inv_s,
                                      hipStream_t s) {
    const size_t lds = (size_t)dim * sizeof(float);  // + the kernel's static red[4]
    hipLaunchKernelGGL(prefill_resid_norm_split_kernel, dim3(pf_split_grid(lay, n)), dim3(256), lds, s, part, ks, part_s, x, dim,
                       nw, ndt, eps, n, lay, xh, xl, inv_s);
}
void xalm::pf_glu_split_launch(const float* part, int ks, const float* part_s, int n, int hidden, int act, int lay,
                               uint16_t* xh, uint16_t* xl, float* inv_s, hipStream_t s) {
    // dynamic LDS = one f32 row of h; the kernel adds a static 16-float reduction array
    const size_t lds = (size_t)hidden * sizeof(float);
    hipLaunchKernelGGL(prefill_glu_split_kernel, dim3(pf_split_grid(lay, n)), dim3(1024), lds, s, part, ks, n, hidden, act, lay,
                       xh, xl, inv_s, part_s);
}
void xalm::pf_epi_plain_launch(const float* part, const float* part_s, int ks, int n, int rows, int epi, float* out,
                               size_t out_stride, int act, hipStream_t s) {
    PfEpiArgs e{};
    e.part = part; e.part_s = part_s; e.ks = ks; e.n = n; e.rows = rows; e.epi = epi; e.out = out;
    e.out_stride = out_stride; e.act = act;
    pf_epi_launch(e, s);
}

bool xalm::pf_attn_shape_ok(int hd, int qpk) { return pf_attn_shape(hd, qpk); }
int xalm::pf_fa_split_max(int pos0) { return std::max(1, pos0 / (32 * FA_TPS) / FA_MIN_SPLIT_STAGES); }
int xalm::pf_fa_pick_nsplit(const PfAttnDims& d, int n_cu, int n, int pos0, size_t part_floats) {
    const int wg = d.n_kv_heads * fa2_query_tiles(n, d.n_heads / d.n_kv_heads);
    int ns = std::min((2 * n_cu + wg - 1) / wg, pos0 / (32 * FA_TPS) / FA_MIN_SPLIT_STAGES);
    ns = (int)std::min<size_t>((size_t)ns, part_floats / pf_fa_part_floats(d, 1, n));
    return std::max(ns, 1);
}
int xalm::pf_fa_launch(const PfAttnDims& d, int kv_dt, bool shared, const float* q, const uint16_t* kc, const uint16_t* vc,
                       float* out, int n, int pos0, int nsplit, float* part, hipStream_t s) {
    if (d.n_kv_heads <= 0 || d.n_heads % d.n_kv_heads || (kv_dt != XH_F16 && kv_dt != XH_F8_E4M3)) return -1;
    return d.head_dim == 128  ? pf_fa_hd<128>(d, kv_dt, shared, q, kc, vc, out, n, pos0, nsplit, part, s)
           : d.head_dim == 64 ? pf_fa_hd<64>(d, kv_dt, shared, q, kc, vc, out, n, pos0, nsplit, part, s)
           : d.head_dim == 16 ? pf_fa_hd<16>(d, kv_dt, shared, q, kc, vc, out, n, pos0, nsplit, part, s)
                              : -1;
}
int xalm::pf_ring_launch(const PfAttnDims& d, int kv_dt, const float* q, uint16_t* kc, uint16_t* vc, const uint16_t* ks,
                         const uint16_t* vs, const uint16_t* sinkv, float* out, int m, int p0, int max_seq_len, int nsplit,
                         float* part, hipStream_t s, const uint16_t* sinkm, uint16_t* master) {
    if (d.head_dim != 128 || d.n_kv_heads <= 0 || d.n_heads % d.n_kv_heads || (kv_dt != XH_F16 && kv_dt != XH_F8_E4M3))
        return -1;
    return for_qpk(d.n_heads / d.n_kv_heads, [&](auto Q) {
        constexpr int QPK = decltype(Q)::value;
        if (kv_dt == XH_F8_E4M3)
            return pf_ring_t<QPK, XH_F8_E4M3>(d, q, kc, vc, ks, vs, sinkv, out, m, p0, max_seq_len, nsplit, part, s, sinkm,
                                              master);
        return pf_ring_t<QPK, XH_F16>(d, q, kc, vc, ks, vs, sinkv, out, m, p0, max_seq_len, nsplit, part, s, nullptr, nullptr);
    });
}

namespace {

PfAttnDims pf_dims(const xh_ctx* ctx) { return {ctx->c.head_dim, ctx->c.n_heads, ctx->c.n_kv_heads}; }
// the prompt attention in force: XH_OPT_PREFILL_ATTN, but 0 (prefill_attn_kernel, the decode
// blocks) on an fp8 KV ring unless XH_OPT_PREFILL_ATTN_KV8 asks for the MFMA kernels' fp8 form
// (prefill.h, KV = XH_F8_E4M3); the stored options are untouched
int pf_attn_mode_of(const xh_ctx* ctx) { return ctx->kv8() && !ctx->pf_attn_kv8 ? 0 : ctx->pf_attn_mode; }
// the splits of a pass of n tokens over pos0 slots of history, within the partials buffer
int pf_fa_nsplit(const xh_ctx* ctx, int n, int pos0) {
    if (!ctx->pf_fa_split) return 1;
    return pf_fa_pick_nsplit(pf_dims(ctx), ctx->n_cu, n, pos0, pf_part_floats(ctx, ctx->pf.cap[PfBufs::PASS]));
}
// the shapes of pf_attn_shape are the only instantiations; -1 for another one
int pf_attn_any(xh_ctx* ctx, const AttnArgs& a, int n, int pos0) {
    const int hd = ctx->c.head_dim;
    if (pf_attn_mode_of(ctx) != 0) {
        const bool shared = ctx->pf_attn_mode == 1 && hd == 128;
        return pf_fa_launch(pf_dims(ctx), ctx->kv_dt, shared, a.q, a.kc, a.vc, a.out, n, pos0,
                            shared ? pf_fa_nsplit(ctx, n, pos0) : 1, ctx->pf.part, ctx->stream);
    }
    auto go = [&](auto H) {
        constexpr int HD = decltype(H)::value;
        return for_qpk(ctx->qpk, [&](auto Q) {
            constexpr int QPK = decltype(Q)::value;
            if constexpr (pf_attn_shape(HD, QPK)) {
                if (ctx->kv8()) pf_attn_t<HD, QPK, XH_F8_E4M3>(ctx, a, n);
                else pf_attn_t<HD, QPK, XH_F16>(ctx, a, n);
                return 0;
            }
            return -1;
        });
    };
    return hd == 128 ? go(std::integral_constant<int, 128>{}) : hd == 64 ? go(std::integral_constant<int, 64>{})
           : hd == 16 ? go(std::integral_constant<int, 16>{}) : -1;
}
// 0, XH_E_INVALID for a head shape with no prompt attention, or the split buffers' allocation error
int pf_attn(xh_ctx* ctx, const AttnArgs& a, int n, int pos0) {
    const int hd = ctx->c.head_dim;
    AttnArgs b = a;
    if (pf_attn_shape(hd, ctx->qpk) && pf_attn_mode_of(ctx) == 0) {
        const int rc = pf_alloc_group(ctx, PfBufs::ATTN0);
        if (rc) return rc;
        b.part_o = ctx->pf.po; b.part_ml = ctx->pf.pml; b.counters = ctx->pf.cnt;
    }
    const int rc = pf_attn_any(ctx, b, n, pos0);
    return rc < 0 ? set_err(ctx, XH_E_INVALID, "prefill: head shape not instantiated") : 0;
}

// Attention of a ring pass (prefill.h, prefill_fa2_ring_kernel): m <= W = max_seq_len - 2 tokens at
// positions p0.. >= max_seq_len, their K/V in the staging rows.  Four launches per layer: the
// sink K versions, the window walk into split partials (pf.part: free between the qkv epilogue
// and the Wo GEMM), the merge that adds the sinks, and the commit of the staged rows and the last
// sink version to the ring.
int pf_attn_ring(xh_ctx* ctx, int l, int m, int p0) {
    const PfAttnDims d = pf_dims(ctx);
    const int nsplit = pf_fa_nsplit(ctx, m, ctx->c.max_seq_len - 2);
    if (pf_fa_part_floats(d, nsplit, m) > pf_part_floats(ctx, ctx->pf.cap[PfBufs::PASS]))
        return set_err(ctx, XH_E_INVALID, "prefill: the ring pass's attention partials do not fit");
    uint16_t *kc = ctx->kcache(l), *vc = ctx->vcache(l);
    const dim3 vgrid((ctx->kv_dim + 255) / 256);
    if (ctx->kv8())  // the sinks iterate in the layer's fp16 master; the versions are its codes
        hipLaunchKernelGGL(prefill_sink_versions_kernel<XH_F8_E4M3>, vgrid, dim3(256), 0, ctx->stream,
                           (const uint16_t*)ctx->master(l), (const float*)ctx->sink_cos, (const float*)ctx->sink_sin,
                           ctx->kv_dim, ctx->c.head_dim, m, ctx->pf.sinkv, ctx->pf.sinkm);
    else
        hipLaunchKernelGGL(prefill_sink_versions_kernel<XH_F16>, vgrid, dim3(256), 0, ctx->stream, (const uint16_t*)kc,
                           (const float*)ctx->sink_cos, (const float*)ctx->sink_sin, ctx->kv_dim, ctx->c.head_dim, m,
                           ctx->pf.sinkv, (uint16_t*)nullptr);
    const int rc = pf_ring_launch(d, ctx->kv_dt, ctx->pf.q, kc, vc, ctx->pf.ks, ctx->pf.vs, ctx->pf.sinkv, ctx->pf.att, m, p0,
                                  ctx->c.max_seq_len, nsplit, ctx->pf.part, ctx->stream, ctx->pf.sinkm,
                                  ctx->kv8() ? ctx->master(l) : nullptr);
    return rc < 0 ? set_err(ctx, XH_E_INVALID, "prefill: head shape not instantiated") : rc;
}

// Whether the batched path covers prompts on this model at all (else the per-token loop): an
// instantiated head shape, K multiples of the chunk pair (always, for K % 32).
bool pf_supported(const xh_ctx* ctx) {
    const xh_config& c = ctx->c;
    if (!ctx->prefill_batched || !pf_attn_shape(c.head_dim, ctx->qpk)) return false;
    // every GEMM's K in whole chunk pairs of its decoder (f32-input kernel; the others need less)
    for (const PfMat& g : pf_all_mats(ctx))
        if (g.K % (2 * pf_elems(g.dt))) return false;
    return c.dim % 32 == 0 && c.hidden_dim % 32 == 0 && ctx->q_dim % 32 == 0;
}
// Ring passes (positions >= max_seq_len): the shared-tile attention's head shape only
// (prefill_fa2_ring_kernel is head_dim 128), and a ring with at least two slots behind the sinks
// An fp8 KV ring has them under XH_OPT_PREFILL_RING_KV8 on top of XH_OPT_PREFILL_ATTN_KV8 only (the
// ring kernels' fp8 form: staged codes, the sinks' versions from their fp16 master).
bool pf_ring_ok(const xh_ctx* ctx) {
    if (ctx->kv8() && !(ctx->pf_ring_kv8 && ctx->pf_attn_kv8)) return false;
    return ctx->pf_ring && ctx->c.head_dim == 128 && ctx->pf_attn_mode == 1 && ctx->c.max_seq_len - 2 >= 2;
}

// How a prompt of n tokens at pos0 runs: pieces in order, each batched (PF_RING: ring passes of at
// most min(pass length, max_seq_len - 2) tokens, all at positions >= max_seq_len) or PF_LOOP, one
// decode step per token.  The prompt is cut at pos = L = max_seq_len, so no pass straddles it:
// below L the batched passes as ever (a piece shorter than min_n takes the loop: xh_prefill's
// one-token rule), from L on ring passes — fewer than PF_RING_MIN tokens, alone or left over by
// the passes before them, take the loop there too.  Without ring passes (XH_OPT_PREFILL_RING 0, or
// a head shape they do not cover) a prompt that reaches past L takes the loop as a whole.
// PF_RING_MIN: at the end of a 32k ring two decode steps take 6.6 ms, a ring pass of two tokens
// 7.5 ms, of eight 7.5 ms against 26.1 (tools/ring_pass.py, profiles/ring_pass.txt).
constexpr int PF_RING_MIN = 3;
enum { PF_LOOP = 0, PF_BATCH = 1, PF_RING = 2 };
struct PfPiece { int off, n, kind, passes; };
void pf_plan(const xh_ctx* ctx, int n, int pos0, int min_n, std::vector<PfPiece>& out) {
    const int L = ctx->c.max_seq_len;
    out.clear();
    const bool wraps = pos0 > L - n;  // pos0 + n > L
    // an fp8 KV ring without ring passes batches the part below L and takes the loop from the cut
    if (!pf_supported(ctx) || (wraps && !pf_ring_ok(ctx) && !ctx->kv8())) {
        out.push_back({0, n, PF_LOOP, 0});
        return;
    }
    const int pass = pf_pass_tokens(ctx);
    const int na = wraps ? std::max(0, L - pos0) : n, nb = n - na;
    if (na > 0) out.push_back({0, na, na >= min_n ? PF_BATCH : PF_LOOP, na >= min_n ? (na + pass - 1) / pass : 0});
    if (nb > 0 && !pf_ring_ok(ctx)) {
        out.push_back({na, nb, PF_LOOP, 0});
    } else if (nb > 0) {
        const int rp = std::min(pass, L - 2);
        const int rem = nb % rp, tail = rem > 0 && rem < PF_RING_MIN ? rem : 0;
        if (nb > tail) out.push_back({na, nb - tail, PF_RING, (nb - tail + rp - 1) / rp});
        if (tail) out.push_back({n - tail, tail, PF_LOOP, 0});
    }
}

// A pass's tokens and per-token step parameters to the device (sps: host staging, reused by the
// next pass after the driver's synchronize), then its embedding rows into pf.x
int pf_stage(xh_ctx* ctx, const PfPass& ps, const int* tokens, std::vector<StepParams>& sps) {
    const xh_config& c = ctx->c;
    PfBufs& b = ctx->pf;
    HIP_TRY(ctx, hipMemcpyAsync(b.tok, tokens, (size_t)ps.m * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    for (int t = 0; t < ps.m; t++) {
        StepParams& h = sps[t];
        h = StepParams{};
        h.token = tokens[t];
        h.pos = ps.p0 + t;
        h.kv_sink = ps.ring ? 2 : 0;  // src/infer.cpp:611-613
        h.kv_pos = ps.ring ? 2 + (ps.p0 + t - 2) % (c.max_seq_len - 2) : ps.p0 + t;
        h.kv_len = ps.ring ? c.max_seq_len : ps.p0 + t + 1;
        h.max_seq_len = c.max_seq_len;
    }
    HIP_TRY(ctx, hipMemcpyAsync(b.sp, sps.data(), (size_t)ps.m * sizeof(StepParams), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(prefill_embed_kernel, dim3(ps.m), dim3(256), 0, ctx->stream, (const int*)b.tok,
                       (const void*)ctx->embed, ctx->embed_dt, c.dim, b.x);
    return 0;
}
// Layer l over the pass's rows: pf.x in, pf.x out, K/V rows written
int pf_layer(xh_ctx* ctx, PfPass& ps, int l) {
    const xh_config& c = ctx->c;
    PfBufs& b = ctx->pf;
    const LayerW& w = ctx->L[l];
    const auto mats = pf_layer_mats(ctx, l);
    const int m = ps.m;
    int rc, ks = 0;
    // attention block (src/infer.cpp:380-452)
    // layers after the first: the previous W2 residual and this rmsnorm ran as one launch
    if (l == 0) pf_norm(ctx, ps, w.attn_norm, w.an_dt, mats[PF_QKV]);
    if ((rc = pf_gemm(ctx, ps, mats[PF_QKV], b.xn, m, ks))) return rc;
    PfEpiArgs e{};
    e.ks = ks; e.n = m; e.rows = mats[PF_QKV].rows; e.epi = ctx->kv8() ? EPI_QKV8 : EPI_QKV; e.q = b.q;
    if (ctx->kv8()) e.sink_master = ctx->master(l);
    e.kcache = ctx->kcache(l); e.vcache = ctx->vcache(l); e.q_dim = ctx->q_dim; e.kv_dim = ctx->kv_dim;
    e.head_dim = c.head_dim; e.rope_freq = ctx->rope_freq; e.qkv_clip = c.qkv_clip; e.pos0 = ps.p0; e.act = c.act;
    if (ps.ring) { e.kstage = b.ks; e.vstage = b.vs; }
    pf_epi(ctx, ps, e);
    if (ps.ring) {
        if ((rc = pf_attn_ring(ctx, l, m, ps.p0))) return rc;
    } else {
        AttnArgs aa = attn_args(ctx, l);
        aa.q = b.q; aa.out = b.att;
        // splits for this pass's longest row (attn_block: >= ATTN_MIN_T slots per split)
        aa.nsplit = std::min(ctx->nsplit, std::max(1, (ps.p0 + m + ATTN_MIN_T - 1) / ATTN_MIN_T));
        if ((rc = pf_attn(ctx, aa, m, ps.p0))) return rc;
    }
    if ((rc = pf_gemm(ctx, ps, mats[PF_WO], b.att, m, ks))) return rc;
    // residual, then the feed-forward block's rmsnorm (src/infer.cpp:449-452, 455-494)
    if ((rc = pf_resid_norm(ctx, ps, ks, w.ffn_norm, w.fn_dt, mats[PF_W13]))) return rc;
    if ((rc = pf_gemm(ctx, ps, mats[PF_W13], b.xn, m, ks))) return rc;
    if ((rc = pf_glu(ctx, ps, ks, mats[PF_W2]))) return rc;
    if ((rc = pf_gemm(ctx, ps, mats[PF_W2], b.h, m, ks))) return rc;
    if (l + 1 < c.n_layers) {
        // residual, then the next layer's attention rmsnorm (src/infer.cpp:491-494, 380)
        const LayerW& wn = ctx->L[l + 1];
        return pf_resid_norm(ctx, ps, ks, wn.attn_norm, wn.an_dt, pf_layer_mats(ctx, l + 1)[PF_QKV]);
    }
    e = PfEpiArgs{};
    e.ks = ks; e.n = m; e.rows = c.dim; e.epi = EPI_RESID; e.out = b.x;
    pf_epi(ctx, ps, e);
    return 0;
}
// xh_score's per-row tail in place of token_prob_kernel: the row kernel of top_logprobs.h.  The
// run's `probs` buffer is `lp` (the targets' log-probabilities), so a row's offset into every
// whole-run device buffer here is probs - lp.
struct ScoreTail {
    int n_top;            // 0: no top list
    float* lp;            // [rows]
    int* rank;            // [rows]
    int* ids;             // [rows][n_top]
    float* lps;           // [rows][n_top]
    float* logits_host;   // [rows][vocab] on the host, or nullptr: the echo of the rows' raw logits
};
// m rows at `logits` (row stride = vocab) with device targets `tgt`, the first of them row
// probs - sc.lp of the run
int score_rows(xh_ctx* ctx, const ScoreTail& sc, const float* logits, int m, const int* tgt, float* probs) {
    const size_t V = (size_t)ctx->c.vocab_size, off = (size_t)(probs - sc.lp), nt = (size_t)sc.n_top;
    launch_top_logprobs(logits, (int)V, V, m, nullptr, sc.n_top, nullptr, 0, tgt, sc.n_top, sc.n_top ? sc.ids + off * nt : nullptr,
                        sc.n_top ? sc.lps + off * nt : nullptr, probs, sc.rank + off, ctx->stream);
    if (sc.logits_host)
        HIP_TRY(ctx, hipMemcpyAsync(sc.logits_host + off * V, logits, (size_t)m * V * 4, hipMemcpyDeviceToHost, ctx->stream));
    return 0;
}

// Model::forward's OUTPUT_LOGITS tail (src/infer.cpp:620-637) for every token of the pass, then
// probs[t] = Sampler::sample_prob of token t's target (targets: host, probs: device, m each);
// under sc, xh_score's tail instead
int pf_logits_probs(xh_ctx* ctx, PfPass& ps, const int* targets, float* probs, const ScoreTail* sc) {
    const xh_config& c = ctx->c;
    PfBufs& b = ctx->pf;
    const int m = ps.m;
    int rc;
    HIP_TRY(ctx, hipMemcpyAsync(b.tgt, targets, (size_t)m * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(prefill_rmsnorm_kernel, dim3(m), dim3(256), 0, ctx->stream, (const float*)b.x, c.dim,
                       (const void*)ctx->final_norm, ctx->final_norm_dt, c.norm_eps, b.xn);
    const PfMat cls = pf_cls_mat(ctx);
    const size_t cls_rb = dev_row_bytes(ctx->wcls_dt, c.dim);
    // lm_head weights off the hipBLASLt path (bf16 on the fp8 checkpoints): 64-token slices
    const int tstep = pf_lay0(ctx, cls.dt, c.dim, cls.wide) ? m : PF_TOK;
    for (int r0 = 0; r0 < c.vocab_size; r0 += PF_CLS_CHUNK) {
        PfMat g = cls;
        g.w = (const char*)cls.w + (size_t)r0 * cls_rb;
        g.rows = std::min(PF_CLS_CHUNK, c.vocab_size - r0);
        for (int t0 = 0; t0 < m; t0 += tstep) {
            const int mt = std::min(tstep, m - t0);
            int ks = 0;
            if ((rc = pf_gemm(ctx, ps, g, b.xn + (size_t)t0 * c.dim, mt, ks))) return rc;
            PfEpiArgs e{};
            e.ks = ks; e.n = mt; e.rows = g.rows; e.epi = EPI_STORE;
            e.out = b.logits + (size_t)t0 * c.vocab_size + r0;
            e.out_stride = (size_t)c.vocab_size;
            pf_epi(ctx, ps, e);
        }
    }
    if (sc) return score_rows(ctx, *sc, b.logits, m, b.tgt, probs);
    hipLaunchKernelGGL(token_prob_kernel, dim3(m), dim3(1024), 0, ctx->stream, (const float*)b.logits, c.vocab_size,
                       (size_t)c.vocab_size, (const int*)b.tgt, probs);
    return 0;
}

// tokens[0..n) at positions pos0..: HYDRATE for every token, then the last token's logits.
// probs (device, n floats) != nullptr: also every token's logits (final rmsnorm + lm_head as
// one GEMM per pass) and probs[i] = sample_prob(targets[i]) (targets: host, n ints).
// ring: every position is >= max_seq_len (pf_plan): ring passes.
int prefill_batched(xh_ctx* ctx, const int* tokens, int n, int pos0, int want_logits, const int* targets = nullptr,
                    float* probs = nullptr, bool ring = false, const ScoreTail* sc = nullptr) {
    const xh_config& c = ctx->c;
    int rc = pf_prepare(ctx);
    if (rc) return rc;
    const int pass = ring ? std::min(pf_pass_tokens(ctx), c.max_seq_len - 2) : pf_pass_tokens(ctx);
    if ((rc = pf_alloc(ctx, std::min(pass, std::max(n, PF_TOK))))) return rc;
    if (ring && (rc = pf_alloc_group(ctx, PfBufs::RING))) return rc;
    if (probs && (rc = pf_alloc_group(ctx, PfBufs::LOGITS))) return rc;
    std::vector<StepParams> sps(pass);
    for (int off = 0; off < n; off += pass) {
        PfPass ps{std::min(n - off, pass), pos0 + off, ring, false, false};
        if ((rc = pf_stage(ctx, ps, tokens + off, sps))) return rc;
        for (int l = 0; l < c.n_layers; l++)
            if ((rc = pf_layer(ctx, ps, l))) return rc;
        if (probs && (rc = pf_logits_probs(ctx, ps, targets + off, probs + off, sc))) return rc;
        HIP_TRY(ctx, hipGetLastError());
        if (off + ps.m == n) {
            // the last token's residual stream is the decode path's x
            HIP_TRY(ctx, hipMemcpyAsync(ctx->x, ctx->pf.x + (size_t)(ps.m - 1) * c.dim, (size_t)c.dim * 4,
                                        hipMemcpyDeviceToDevice, ctx->stream));
        }
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // sps / token staging reused by the next pass
    }
    // step parameters of the last prompt token (as the per-token loop leaves them)
    rc = host_step_params(ctx, tokens[n - 1], pos0 + n - 1);
    if (rc) return rc;
    if (want_logits) {
        if (!launch_gemv(GEMV_LOGITS, pf_cls_mat(ctx).dt, cls_args(ctx), ctx->stream, ctx->max_gemv_waves))
            return set_err(ctx, XH_E_INVALID, "unsupported wcls dtype");
        ctx->cand_valid = true;
    }
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}


}  // namespace

int xalm::mm_op_ks(int rows, int K, int n, int* ks) {
    if (K % MM_KMULT) return 1;
    if (*ks == 0) *ks = mm_pick_ks(rows, K, n, (size_t)8 * n * rows);
    return *ks <= 0 || K % (*ks * MM_KMULT) ? 2 : 0;
}
void xalm::mm_op_launch(const uint16_t* w, const uint16_t* xh, const uint16_t* xl, float* out, int rows, int K, int n,
                        int ks, int n_cu) {
    MmArgs a{};
    a.w = w; a.xh = xh; a.xl = xl; a.out = out;
    a.rows = rows; a.K = K; a.n = n; a.ks = ks; a.n_rt = mm_row_tiles(rows); a.n_tt = mm_tok_tiles(n);
    mm_launch(a, n_cu, nullptr);
}

namespace {
// The pieces of pf_plan in order.  probs (device, n floats): xh_perplexity's run, every token with
// logits and probs[i] = sample_prob(targets[i]); else xh_prefill's, the last token's logits if wanted.
// sc: xh_score's run, probs = sc->lp and the row kernel as the per-row tail.
int run_plan(xh_ctx* ctx, const int* tokens, int n, int pos0, int want_logits, const int* targets, float* probs,
             const ScoreTail* sc = nullptr) {
    int rc = 0;
    // hipBLASLt's plans decide the pass length (XH_OPT_PREFILL 4): probe them before planning
    if (ctx->prefill_gemm == 4 && n >= 2 && pf_supported(ctx) && (rc = pf_prepare(ctx))) return rc;
    std::vector<PfPiece> plan;
    pf_plan(ctx, n, pos0, probs ? 1 : 2, plan);
    const int V = ctx->c.vocab_size;
    bool tgt_up = false;
    for (const PfPiece& pc : plan) {
        const bool last = pc.off + pc.n == n;
        if (pc.kind != PF_LOOP) {
            rc = prefill_batched(ctx, tokens + pc.off, pc.n, pos0 + pc.off, last && want_logits,
                                 probs ? targets + pc.off : nullptr, probs ? probs + pc.off : nullptr, pc.kind == PF_RING, sc);
            // it leaves the last token's step parameters in flight from the one pinned host slot
            if (!rc && !last) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        } else {
            if (probs && !tgt_up) {
                HIP_TRY(ctx, copy_sync(ctx, ctx->ppl_tgt, targets, (size_t)n * sizeof(int), hipMemcpyHostToDevice));
                tgt_up = true;
            }
            for (int i = pc.off; i < pc.off + pc.n && !rc; i++) {
                rc = host_step_params(ctx, tokens[i], pos0 + i);
                if (!rc) rc = run_step(ctx, probs || (i == n - 1 && want_logits));
                if (rc) break;
                if (sc)
                    rc = score_rows(ctx, *sc, ctx->logits, 1, ctx->ppl_tgt + i, probs + i);
                else if (probs)
                    hipLaunchKernelGGL(token_prob_kernel, dim3(1), dim3(1024), 0, ctx->stream, (const float*)ctx->logits, V,
                                       (size_t)V, (const int*)ctx->ppl_tgt + i, probs + i);
                if (rc) break;
                // the step parameters are copied from one pinned host slot: drain before reuse
                if (hipStreamSynchronize(ctx->stream) != hipSuccess) rc = set_err(ctx, XH_E_HIP, "hipStreamSynchronize failed");
            }
        }
        if (rc) return rc;
    }
    return 0;
}
}  // namespace

extern "C" {

int xh_prefill_route(const xh_ctx* ctx, int n, int pos0, int* n_batched, int* n_passes) {
    if (!ctx || n <= 0 || pos0 < 0) return XH_E_INVALID;
    std::vector<PfPiece> plan;
    pf_plan(ctx, n, pos0, 2, plan);
    int nb = 0, np = 0;
    for (const PfPiece& pc : plan)
        if (pc.kind != PF_LOOP) { nb += pc.n; np += pc.passes; }
    if (n_batched) *n_batched = nb;
    if (n_passes) *n_passes = np;
    return 0;
}

int xh_prefill(xh_ctx* ctx, const int* tokens, int n, int pos0, int want_logits, float* logits_out) {
    if (!ctx || !tokens || n <= 0 || pos0 < 0) return set_err(ctx, XH_E_INVALID, "bad prefill arguments");
    for (int i = 0; i < n; i++)
        if (tokens[i] < 0 || tokens[i] >= ctx->c.vocab_size) return set_err(ctx, XH_E_INVALID, "token out of range");
    HIP_TRY(ctx, hipSetDevice(ctx->dev));
    int rc = check_ready(ctx);
    if (rc) return rc;
    // pf_plan: batched passes, ring passes from max_seq_len on; a one-token piece runs the decode
    // step (one graph replay of the matvecs) rather than a pass of GEMMs over one token: 3.3 vs
    // 7.3 ms at the end of a 32k ring (tools/short_pass.py)
    if ((rc = run_plan(ctx, tokens, n, pos0, want_logits, nullptr, nullptr))) return rc;
    if (logits_out && want_logits)
        HIP_TRY(ctx, hipMemcpyAsync(logits_out, ctx->logits, (size_t)ctx->c.vocab_size * 4, hipMemcpyDeviceToHost,
                                    ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return check_aw(ctx);
}

// The perplexity loop of run_perplexity (src/main.cpp:243-254): forward tokens[0..n-1) at
// positions pos0.. with logits, probs_out[i] = Sampler::sample_prob(tokens[i + 1]) after token
// i (src/sampler.cpp:3-17).  The logits never leave the device; batched passes where the
// prompt path allows (pf_plan, as xh_prefill), else token by token.
int xh_perplexity(xh_ctx* ctx, const int* tokens, int n, int pos0, float* probs_out) {
    if (!ctx || !tokens || !probs_out || n < 2 || pos0 < 0) return set_err(ctx, XH_E_INVALID, "bad perplexity arguments");
    for (int i = 0; i < n; i++)
        if (tokens[i] < 0 || tokens[i] >= ctx->c.vocab_size) return set_err(ctx, XH_E_INVALID, "token out of range");
    HIP_TRY(ctx, hipSetDevice(ctx->dev));
    int rc = check_ready(ctx);
    if (rc) return rc;
    const int m = n - 1;
    if (ctx->ppl_cap < m) {
        hipFree(ctx->ppl_tgt); hipFree(ctx->ppl_prob);
        ctx->ppl_tgt = nullptr; ctx->ppl_prob = nullptr; ctx->ppl_cap = 0;
        if ((rc = dmalloc(ctx, &ctx->ppl_tgt, (size_t)m)) || (rc = dmalloc(ctx, &ctx->ppl_prob, (size_t)m))) return rc;
        ctx->ppl_cap = m;
    }
    if ((rc = run_plan(ctx, tokens, m, pos0, 0, tokens + 1, ctx->ppl_prob))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(probs_out, ctx->ppl_prob, (size_t)m * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return check_aw(ctx);
}

// xh_perplexity's run (the same plan, passes and buffers for the targets and the per-token
// figure) with the row kernel of top_logprobs.h as the per-row tail: log-probability and rank of
// tokens[i + 1], the top list, and on request the rows' raw logits.
int xh_score(xh_ctx* ctx, const int* tokens, int n, int pos0, int n_top, float* logprobs_out, int* ranks_out,
             int* top_ids_out, float* top_lps_out, float* logits_out) {
    if (!ctx || !tokens || n < 2 || pos0 < 0) return set_err(ctx, XH_E_INVALID, "bad score arguments");
    if (n_top < 0 || n_top > XH_TOP_MAX || n_top > ctx->c.vocab_size)
        return set_err(ctx, XH_E_INVALID, "n_top %d outside 0 .. min(%d, vocab)", n_top, XH_TOP_MAX);
    if (ctx->c.vocab_size > TOP_MAX_VOCAB) return set_err(ctx, XH_E_INVALID, "vocab_size > %d", TOP_MAX_VOCAB);
    for (int i = 0; i < n; i++)
        if (tokens[i] < 0 || tokens[i] >= ctx->c.vocab_size) return set_err(ctx, XH_E_INVALID, "token out of range");
    HIP_TRY(ctx, hipSetDevice(ctx->dev));
    int rc = check_ready(ctx);
    if (rc) return rc;
    const int m = n - 1;
    if (ctx->ppl_cap < m) {
        hipFree(ctx->ppl_tgt); hipFree(ctx->ppl_prob);
        ctx->ppl_tgt = nullptr; ctx->ppl_prob = nullptr; ctx->ppl_cap = 0;
        if ((rc = dmalloc(ctx, &ctx->ppl_tgt, (size_t)m)) || (rc = dmalloc(ctx, &ctx->ppl_prob, (size_t)m))) return rc;
        ctx->ppl_cap = m;
    }
    // the run's ranks and top lists: this call's own
    struct Buf {
        void* p = nullptr;
        ~Buf() { if (p) hipFree(p); }
    } d_rank, d_ids, d_lps;
    const size_t top = (size_t)m * (size_t)n_top;
    if (hipMalloc(&d_rank.p, (size_t)m * sizeof(int)) != hipSuccess ||
        (n_top && (hipMalloc(&d_ids.p, top * sizeof(int)) != hipSuccess || hipMalloc(&d_lps.p, top * sizeof(float)) != hipSuccess)))
        return set_err(ctx, XH_E_HIP, "hipMalloc failed");
    const ScoreTail sc = {n_top, ctx->ppl_prob, (int*)d_rank.p, (int*)d_ids.p, (float*)d_lps.p, logits_out};
    if ((rc = run_plan(ctx, tokens, m, pos0, 0, tokens + 1, ctx->ppl_prob, &sc))) return rc;
    if (logprobs_out)
        HIP_TRY(ctx, hipMemcpyAsync(logprobs_out, ctx->ppl_prob, (size_t)m * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    if (ranks_out) HIP_TRY(ctx, hipMemcpyAsync(ranks_out, d_rank.p, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    if (top_ids_out && n_top)
        HIP_TRY(ctx, hipMemcpyAsync(top_ids_out, d_ids.p, top * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    if (top_lps_out && n_top)
        HIP_TRY(ctx, hipMemcpyAsync(top_lps_out, d_lps.p, top * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return check_aw(ctx);
}
}  // extern "C"
