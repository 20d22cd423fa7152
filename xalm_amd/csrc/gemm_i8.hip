// gemm_i8.hip — the launch bodies of the int8 prompt GEMM for Q8_0 / Q4_0 / Q4_1 / Q5_0 / Q5_1 and of its
// activation quantiser (gemm_i8.h: this unit alone includes it), shared by the passes (prefill.hip) and by
// xh_op_prompt_matmul_i8 (ops.hip).  Nothing here reads a context.
#include <hip/hip_runtime.h>

#include "ctx.h"
#include "gemm_i8.h"

using namespace xalm;

namespace {
template <int DT>
int mi_launch(const MiArgs& a, hipStream_t s) {
    if (!ensure_lds((const void*)mm_i8_kernel<DT>, MI_LDS)) return PF_GEMM_E_FIT;
    hipLaunchKernelGGL(mm_i8_kernel<DT>, dim3(a.n_rt * a.n_tt * a.ks), dim3(MI_THREADS), MI_LDS, s, a);
    return PF_GEMM_OK;
}
}  // namespace

size_t xalm::pf_i8_row_bytes(int K) { return mi_xpitch((size_t)K); }

void xalm::pf_quant_q8_launch(const uint16_t* xh, const uint16_t* xl, int K, int n, int8_t* xq, hipStream_t s) {
    const size_t lanes = (size_t)n * (K / 16);
    hipLaunchKernelGGL(prefill_quant_q8_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, s, xh, xl, xq, K, n);
}

// xq: the quantiser's rows of io.xh's halves; the partials are unscaled (the epilogue multiplies by 1 / s_t, io.xs)
int xalm::pf_gemm_i8(const PfGemmPlan& p, const PfGemmIo& io, const int8_t* xq, int* ks_out, hipStream_t s) {
    const int rows = p.rows, K = p.K, n = p.n;
    if (!mi_dt(p.dt)) return PF_GEMM_E_DTYPE;
    if (rows < 1 || n < 1 || K < MM_KMULT || K % MM_KMULT) return PF_GEMM_E_SHAPE;
    MiArgs a{};
    a.w = (const uint8_t*)io.w; a.xq = xq; a.out = io.part;
    a.pitch = gq_pitch(p.dt, (size_t)K);
    a.rows = rows; a.K = K; a.n = n; a.ks = p.ks > 0 ? p.ks : mi_pick_ks(rows, K, n, p.part_floats, p.n_cu);
    a.n_rt = (rows + MI_BR - 1) / MI_BR; a.n_tt = (n + MI_BT - 1) / MI_BT;
    if (a.ks <= 0 || a.ks > 8 || K % (a.ks * MM_KMULT) || (size_t)a.ks * n * rows > p.part_floats) return PF_GEMM_E_FIT;
    int rc;
    switch (p.dt) {
        case XH_Q8_0: rc = mi_launch<XH_Q8_0>(a, s); break;
        case XH_Q4_0: rc = mi_launch<XH_Q4_0>(a, s); break;
        case XH_Q4_1: rc = mi_launch<XH_Q4_1>(a, s); break;
        case XH_Q5_0: rc = mi_launch<XH_Q5_0>(a, s); break;
        default: rc = mi_launch<XH_Q5_1>(a, s); break;
    }
    if (rc) return rc;
    *ks_out = a.ks;
    return PF_GEMM_OK;
}
