// gemm_kq.hip — the launch body of the K-quant prompt GEMM (gemm_kq.h: this unit alone includes it),
// shared by the passes (prefill.hip) and by xh_op_prompt_matmul_kq (ops.hip).  Nothing here reads a context.
#include <hip/hip_runtime.h>

#include "ctx.h"
#include "gemm_kq.h"

using namespace xalm;

// io.xh: the row-major hi rows then lo rows of the layout-0 producers; the partials are unscaled (the
// epilogue multiplies by 1 / s_t, io.xs)
int xalm::pf_gemm_kq(const PfGemmPlan& p, const PfGemmIo& io, int* ks_out, hipStream_t s) {
    const int rows = p.rows, K = p.K, n = p.n;
    if (!gq_k(p.dt)) return PF_GEMM_E_DTYPE;
    if (rows < 1 || n < 1 || K < MK_KMULT || K % MK_KMULT) return PF_GEMM_E_SHAPE;
    MkArgs a{};
    a.w = (const uint8_t*)io.w; a.xh = io.xh; a.xl = io.xh + (size_t)n * K; a.out = io.part;
    a.pitch = gq_pitch(p.dt, (size_t)K);
    a.rows = rows; a.K = K; a.n = n; a.ks = p.ks > 0 ? p.ks : mk_pick_ks(rows, K, n, p.part_floats, p.n_cu);
    a.n_rt = (rows + MK_BR - 1) / MK_BR; a.n_tt = (n + MK_BT - 1) / MK_BT;
    if (a.ks <= 0 || a.ks > 8 || K % (a.ks * MK_KMULT) || (size_t)a.ks * n * rows > p.part_floats) return PF_GEMM_E_FIT;
    const dim3 grid(a.n_rt * a.n_tt * a.ks);
    if (p.dt == XH_Q4_K) {
        if (!ensure_lds((const void*)mm_kq_kernel<XH_Q4_K>, MK_LDS)) return PF_GEMM_E_FIT;
        hipLaunchKernelGGL(mm_kq_kernel<XH_Q4_K>, grid, dim3(MK_THREADS), MK_LDS, s, a);
    } else {
        if (!ensure_lds((const void*)mm_kq_kernel<XH_Q6_K>, MK_LDS)) return PF_GEMM_E_FIT;
        hipLaunchKernelGGL(mm_kq_kernel<XH_Q6_K>, grid, dim3(MK_THREADS), MK_LDS, s, a);
    }
    *ks_out = a.ks;
    return PF_GEMM_OK;
}
