// gemm_bf16.hip — the launch bodies of the bf16-weight prompt GEMM and its piece producers
// (gemm_bf16.h: this unit alone includes it), shared by the passes (prefill.hip) and by
// xh_op_prompt_matmul_bf16 (ops.hip).  Nothing here reads a context.
#include <hip/hip_runtime.h>

#include "ctx.h"
#include "gemm_bf16.h"

using namespace xalm;

void xalm::pf_split_bf16_launch(const float* x, int K, int n, uint16_t* x3, hipStream_t s) {
    hipLaunchKernelGGL(prefill_split_bf16_kernel, dim3(n), dim3(256), 0, s, x, K, n, x3);
}
void xalm::pf_norm_split_bf16_launch(const float* x, int dim, const void* nw, int ndt, float eps, int n, uint16_t* x3,
                                     hipStream_t s) {
    hipLaunchKernelGGL(prefill_rmsnorm_split_bf16_kernel, dim3(n), dim3(256), 0, s, x, dim, nw, ndt, eps, n, x3);
}
int xalm::pf_gemm_bf16(const PfGemmPlan& p, const PfGemmIo& io, int* ks_out, hipStream_t s) {
    const int rows = p.rows, K = p.K, n = p.n;
    if (rows < 1 || n < 1 || K < MM_KMULT || K % MM_KMULT) return PF_GEMM_E_SHAPE;
    MbArgs a{};
    a.w = (const uint16_t*)io.w; a.x = io.xh; a.out = io.part;
    a.rows = rows; a.K = K; a.n = n; a.ks = p.ks > 0 ? p.ks : mm_pick_ks(rows, K, n, p.part_floats, p.n_cu, MB_BT);
    a.n_rt = (rows + MB_BR - 1) / MB_BR; a.n_tt = (n + MB_BT - 1) / MB_BT;
    if (a.ks <= 0 || a.ks > 8 || K % (a.ks * MM_KMULT) || (size_t)a.ks * n * rows > p.part_floats) return PF_GEMM_E_FIT;
    if (!ensure_lds((const void*)mm_bf16_kernel, mb_lds(MB_NS))) return PF_GEMM_E_FIT;
    hipLaunchKernelGGL(mm_bf16_kernel, dim3(a.n_rt * a.n_tt * a.ks), dim3(MB_THREADS), mb_lds(MB_NS), s, a);
    *ks_out = a.ks;
    return PF_GEMM_OK;
}
