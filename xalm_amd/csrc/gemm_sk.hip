// gemm_sk.hip — the launch body of the weight-streaming code GEMM for prompt passes of at most 64 tokens
// (gemm_sk.h: this unit alone includes it), shared by the passes (prefill.hip) and by
// xh_op_prompt_matmul_sk (ops.hip).  Nothing here reads a context.
#include <hip/hip_runtime.h>

#include "ctx.h"
#include "gemm_sk.h"

using namespace xalm;

namespace {
template <int DT, int TT>
void sk_launch_t(const MkArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((mm_sk_kernel<DT, TT>), dim3(a.n_rt * a.ks), dim3(SK_THREADS), sk_lds(TT), s, a);
}
template <int DT>
void sk_launch(const MkArgs& a, hipStream_t s) {
    switch (a.n_tt) {
        case 1: sk_launch_t<DT, 1>(a, s); break;
        case 2: sk_launch_t<DT, 2>(a, s); break;
        case 3: sk_launch_t<DT, 3>(a, s); break;
        default: sk_launch_t<DT, 4>(a, s); break;
    }
}
}  // namespace

int xalm::sk_row_tile() { return SK_BR; }
bool xalm::sk_ks_ok(int dt, int K, int ks) { return ks >= 1 && ks <= SK_MAX_KS && !(ks & (ks - 1)) && K % (ks * sk_kmult(dt)) == 0; }

// io.xh: the row-major hi rows then lo rows of the layout-0 producers; the partials are unscaled (the
// epilogue multiplies by 1 / s_t, io.xs)
int xalm::pf_gemm_sk(const PfGemmPlan& p, const PfGemmIo& io, int* ks_out, hipStream_t s) {
    const int rows = p.rows, K = p.K, n = p.n;
    if (!sk_dt(p.dt)) return PF_GEMM_E_DTYPE;
    if (rows < 1 || n < 1 || n > SK_TOK || K < sk_kmult(p.dt) || K % sk_kmult(p.dt)) return PF_GEMM_E_SHAPE;
    MkArgs a{};
    a.w = (const uint8_t*)io.w; a.xh = io.xh; a.xl = io.xh + (size_t)n * K; a.out = io.part;
    a.pitch = gq_pitch(p.dt, (size_t)K);
    a.rows = rows; a.K = K; a.n = n; a.ks = p.ks > 0 ? p.ks : sk_pick_ks(p.dt, rows, K, n, p.part_floats, p.n_cu);
    a.n_rt = (rows + SK_BR - 1) / SK_BR; a.n_tt = (n + 15) / 16;
    if (!sk_ks_ok(p.dt, K, a.ks) || (size_t)a.ks * n * rows > p.part_floats) return PF_GEMM_E_FIT;
    switch (p.dt) {
        case XH_Q8_0: sk_launch<XH_Q8_0>(a, s); break;
        case XH_Q4_0: sk_launch<XH_Q4_0>(a, s); break;
        case XH_Q4_1: sk_launch<XH_Q4_1>(a, s); break;
        case XH_Q5_0: sk_launch<XH_Q5_0>(a, s); break;
        case XH_Q5_1: sk_launch<XH_Q5_1>(a, s); break;
        case XH_Q4_K: sk_launch<XH_Q4_K>(a, s); break;
        default: sk_launch<XH_Q6_K>(a, s); break;
    }
    *ks_out = a.ks;
    return PF_GEMM_OK;
}
