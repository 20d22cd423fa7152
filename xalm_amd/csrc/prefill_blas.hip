// prefill_blas.hip — hipBLASLt behind XH_OPT_PREFILL 4 (host code only).  The one file that
// includes the vendor header; the context holds its state as an opaque pointer.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <hipblaslt/hipblaslt.h>  // types only: the library is dlopen'ed (blas_api)

#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "ctx.h"

using namespace xalm;

// created on the first prompt that uses it: handle, workspace, plans per shape
struct xalm::BlasState {
    struct Plan {
        hipblasLtMatmulDesc_t md = nullptr;
        hipblasLtMatrixLayout_t la = nullptr, lb = nullptr, lc = nullptr;
        std::vector<hipblasLtMatmulAlgo_t> cands;  // the heuristic's candidates (empty: none; [0] is used)
        bool ready = false;
    };
    hipblasLtHandle_t handle = nullptr;
    void* ws = nullptr;
    int ok = 0;
    std::map<std::vector<int>, Plan> plans;
};

namespace {

using BlasPlan = BlasState::Plan;

constexpr size_t PF_BLAS_WS = 256ull << 20;            // hipBLASLt workspace

// hipBLASLt serves only XH_OPT_PREFILL 4 (the vendor GEMM in place of gemm16.h).  Its entry
// points are resolved on first use with dlopen / dlsym, so libxalm_hip.so has no link
// dependency on it (a process that already loaded a copy, e.g. torch's, gets that copy by
// soname); without it, mode 4 fails with an error and everything else is unaffected.
struct BlasApi {
#define XH_BLAS_FN(name) decltype(&hipblasLt##name) name = nullptr;
    XH_BLAS_FN(Create) XH_BLAS_FN(Destroy) XH_BLAS_FN(MatmulDescCreate) XH_BLAS_FN(MatmulDescDestroy)
    XH_BLAS_FN(MatmulDescSetAttribute) XH_BLAS_FN(MatrixLayoutCreate) XH_BLAS_FN(MatrixLayoutDestroy)
    XH_BLAS_FN(MatmulPreferenceCreate) XH_BLAS_FN(MatmulPreferenceDestroy) XH_BLAS_FN(MatmulPreferenceSetAttribute)
    XH_BLAS_FN(MatmulAlgoGetHeuristic) XH_BLAS_FN(Matmul)
#undef XH_BLAS_FN
    bool ok = false;
    std::string err;
};
const BlasApi* blas_api(std::string* why = nullptr) {
    static BlasApi api;
    static std::once_flag once;
    std::call_once(once, [] {
        void* h = nullptr;
        for (const char* so : {"libhipblaslt.so.1", "libhipblaslt.so", "/opt/rocm/lib/libhipblaslt.so.1"})
            if ((h = dlopen(so, RTLD_NOW | RTLD_LOCAL))) break;
        if (!h) {
            const char* e = dlerror();
            api.err = e ? e : "dlopen failed";
            return;
        }
        bool all = true;
#define XH_BLAS_SYM(name)                                                                \
        api.name = reinterpret_cast<decltype(api.name)>(dlsym(h, "hipblasLt" #name)); \
        all = all && api.name;
        XH_BLAS_SYM(Create) XH_BLAS_SYM(Destroy) XH_BLAS_SYM(MatmulDescCreate) XH_BLAS_SYM(MatmulDescDestroy)
        XH_BLAS_SYM(MatmulDescSetAttribute) XH_BLAS_SYM(MatrixLayoutCreate) XH_BLAS_SYM(MatrixLayoutDestroy)
        XH_BLAS_SYM(MatmulPreferenceCreate) XH_BLAS_SYM(MatmulPreferenceDestroy) XH_BLAS_SYM(MatmulPreferenceSetAttribute)
        XH_BLAS_SYM(MatmulAlgoGetHeuristic) XH_BLAS_SYM(Matmul)
#undef XH_BLAS_SYM
        api.ok = all;
        if (!all) api.err = "hipBLASLt: missing entry points";
    });
    if (why) *why = api.err;
    return api.ok ? &api : nullptr;
}

#define BLAS_TRY(ctx, expr)                                                                          \
    do {                                                                                             \
        hipblasStatus_t _s = (expr);                                                                 \
        if (_s != HIPBLAS_STATUS_SUCCESS)                                                            \
            return set_err((ctx), XH_E_HIP, "%s failed: hipBLASLt status %d", #expr, (int)_s);       \
    } while (0)

// Plan of Y[n][rows] (f32) = X[n][K] (f16) . W[rows][K]^T on hipBLASLt.  Column-major view:
// D (rows x n, ld rows) = op(A) B with A = W stored K x rows (ld K, transposed), B = X stored
// K x n (ld K); f16 A and B, f32 compute (f16 x f16 products are exact in f32).  fp8 weights
// reach it as their exact f16 image (pf_dequant): the torch-bundled hipBLASLt, loaded first
// under the same soname in a process that imported torch, has no e4m3 / e5m2 kernels.  One
// plan per (rows, K, n) holding the heuristic's candidates; *plan = nullptr when there are none.
// At most PF_BLAS_MAX_PLANS plans per context (one per GEMM shape and pass length): a new pass length
// past that runs on gemm16.h, so the map does not grow with every prompt length seen.
constexpr size_t PF_BLAS_MAX_PLANS = 256;
int blas_plan(xh_ctx* ctx, int rows, int K, int n, BlasPlan** plan) {
    *plan = nullptr;
    std::string why;
    if (!blas_api(&why)) return set_err(ctx, XH_E_HIP, "XH_OPT_PREFILL 4 needs hipBLASLt: %s", why.c_str());
    if (!ctx->blas) ctx->blas = new BlasState;
    BlasState& b = *ctx->blas;
    if (!b.handle) {
        BLAS_TRY(ctx, blas_api()->Create(&b.handle));
        char* ws = nullptr;
        int rc = dmalloc(ctx, &ws, PF_BLAS_WS);
        if (rc) return rc;
        b.ws = ws;
    }
    const std::vector<int> key{rows, K, n};
    auto it = b.plans.find(key);
    if (it == b.plans.end() && b.plans.size() >= PF_BLAS_MAX_PLANS) return 0;  // gemm16.h instead
    if (it == b.plans.end()) {
        BlasPlan& p = b.plans[key];  // destroyed with the context, even half-built
        BLAS_TRY(ctx, blas_api()->MatmulDescCreate(&p.md, HIPBLAS_COMPUTE_32F, HIP_R_32F));
        const hipblasOperation_t opT = HIPBLAS_OP_T, opN = HIPBLAS_OP_N;
        BLAS_TRY(ctx, blas_api()->MatmulDescSetAttribute(p.md, HIPBLASLT_MATMUL_DESC_TRANSA, &opT, sizeof opT));
        BLAS_TRY(ctx, blas_api()->MatmulDescSetAttribute(p.md, HIPBLASLT_MATMUL_DESC_TRANSB, &opN, sizeof opN));
        BLAS_TRY(ctx, blas_api()->MatrixLayoutCreate(&p.la, HIP_R_16F, K, rows, K));
        BLAS_TRY(ctx, blas_api()->MatrixLayoutCreate(&p.lb, HIP_R_16F, K, n, K));
        BLAS_TRY(ctx, blas_api()->MatrixLayoutCreate(&p.lc, HIP_R_32F, rows, n, rows));
        hipblasLtMatmulPreference_t pref;
        BLAS_TRY(ctx, blas_api()->MatmulPreferenceCreate(&pref));
        size_t wss = PF_BLAS_WS;
        constexpr int NH = 8;
        hipblasLtMatmulHeuristicResult_t heur[NH];
        int nret = 0;
        hipblasStatus_t st = blas_api()->MatmulPreferenceSetAttribute(pref, HIPBLASLT_MATMUL_PREF_MAX_WORKSPACE_BYTES,
                                                                   &wss, sizeof wss);
        if (st == HIPBLAS_STATUS_SUCCESS)
            st = blas_api()->MatmulAlgoGetHeuristic(b.handle, p.md, p.la, p.lb, p.lc, p.lc, pref, NH, heur, &nret);
        blas_api()->MatmulPreferenceDestroy(pref);
        for (int i = 0; st == HIPBLAS_STATUS_SUCCESS && i < nret; i++) p.cands.push_back(heur[i].algo);
        p.ready = true;
        it = b.plans.find(key);
    }
    if (!it->second.ready) return set_err(ctx, XH_E_HIP, "hipBLASLt: plan %d x %d x %d failed earlier", rows, K, n);
    if (!it->second.cands.empty()) *plan = &it->second;
    return 0;
}

}  // namespace

int xalm::blas_ok(const xh_ctx* ctx) { return ctx->blas ? ctx->blas->ok : 0; }
void xalm::blas_set_ok(xh_ctx* ctx, int ok) {
    if (!ctx->blas) ctx->blas = new BlasState;
    ctx->blas->ok = ok;
}
int xalm::blas_has_plan(xh_ctx* ctx, int rows, int K, int n, bool* have) {
    BlasPlan* p = nullptr;
    const int rc = blas_plan(ctx, rows, K, n, &p);
    *have = p != nullptr;
    return rc;
}

// the GEMM on the heuristic's first candidate for its shape: a fixed algorithm, so a prompt gives
// the same logits on every run (no run-time timing of candidates, whose tilings and split-K
// choices sum in different orders)
int xalm::blas_gemm(xh_ctx* ctx, const void* w, int K, int rows, const uint16_t* x, int n, float* y) {
    BlasPlan* pp = nullptr;
    int rc = blas_plan(ctx, rows, K, n, &pp);
    if (rc) return rc;
    if (!pp) return set_err(ctx, XH_E_HIP, "hipBLASLt: no algorithm for %d x %d x %d", rows, K, n);
    const float alpha = 1.f, beta = 0.f;
    BLAS_TRY(ctx, blas_api()->Matmul(ctx->blas->handle, pp->md, &alpha, w, pp->la, x, pp->lb, &beta, y, pp->lc, y, pp->lc,
                                  &pp->cands[0], ctx->blas->ws, PF_BLAS_WS, ctx->stream));
    return 0;
}

void xalm::blas_free(xh_ctx* ctx) {
    if (!ctx->blas) return;
    for (auto& kv : ctx->blas->plans) {
        const BlasPlan& p = kv.second;
        for (hipblasLtMatrixLayout_t l : {p.la, p.lb, p.lc})
            if (l) blas_api()->MatrixLayoutDestroy(l);
        if (p.md) blas_api()->MatmulDescDestroy(p.md);
    }
    if (ctx->blas->handle) blas_api()->Destroy(ctx->blas->handle);
    hipFree(ctx->blas->ws);
    delete ctx->blas;
    ctx->blas = nullptr;
}
