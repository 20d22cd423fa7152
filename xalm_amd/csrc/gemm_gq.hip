// gemm_gq.hip — the launch body of the block-code prompt GEMM for Q8_0 / Q4_0 / Q4_1 / Q5_0 / Q5_1
// (gemm_gq.h: this unit alone includes it), shared by the passes (prefill.hip) and by
// xh_op_prompt_matmul_gq (ops.hip).  Nothing here reads a context.
#include <hip/hip_runtime.h>

#include "ctx.h"
#include "gemm_gq.h"

using namespace xalm;

namespace {
template <int DT>
int mg_launch(const MkArgs& a, hipStream_t s) {
    if (!ensure_lds((const void*)mm_gq_kernel<DT>, MK_LDS)) return PF_GEMM_E_FIT;
    hipLaunchKernelGGL(mm_gq_kernel<DT>, dim3(a.n_rt * a.n_tt * a.ks), dim3(MK_THREADS), MK_LDS, s, a);
    return PF_GEMM_OK;
}
}  // namespace

// io.xh: the row-major hi rows then lo rows of the layout-0 producers; the partials are unscaled (the
// epilogue multiplies by 1 / s_t, io.xs)
int xalm::pf_gemm_gq(const PfGemmPlan& p, const PfGemmIo& io, int* ks_out, hipStream_t s) {
    const int rows = p.rows, K = p.K, n = p.n;
    if (!mg_dt(p.dt)) return PF_GEMM_E_DTYPE;
    if (rows < 1 || n < 1 || K < MM_KMULT || K % MM_KMULT) return PF_GEMM_E_SHAPE;
    MkArgs a{};
    a.w = (const uint8_t*)io.w; a.xh = io.xh; a.xl = io.xh + (size_t)n * K; a.out = io.part;
    a.pitch = gq_pitch(p.dt, (size_t)K);
    a.rows = rows; a.K = K; a.n = n; a.ks = p.ks > 0 ? p.ks : mg_pick_ks(rows, K, n, p.part_floats, p.n_cu);
    a.n_rt = (rows + MK_BR - 1) / MK_BR; a.n_tt = (n + MK_BT - 1) / MK_BT;
    if (a.ks <= 0 || a.ks > 8 || K % (a.ks * MM_KMULT) || (size_t)a.ks * n * rows > p.part_floats) return PF_GEMM_E_FIT;
    int rc;
    switch (p.dt) {
        case XH_Q8_0: rc = mg_launch<XH_Q8_0>(a, s); break;
        case XH_Q4_0: rc = mg_launch<XH_Q4_0>(a, s); break;
        case XH_Q4_1: rc = mg_launch<XH_Q4_1>(a, s); break;
        case XH_Q5_0: rc = mg_launch<XH_Q5_0>(a, s); break;
        default: rc = mg_launch<XH_Q5_1>(a, s); break;
    }
    if (rc) return rc;
    *ks_out = a.ks;
    return PF_GEMM_OK;
}
