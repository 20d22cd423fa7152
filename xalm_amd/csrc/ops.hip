// ops.hip — single ops on host pointers for the tests (xh_op_*) and the per-kernel timing hooks
// of bench.py (xh_time_kernel, xh_kernel_bytes).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "ctx.h"
#include "standalone.h"

using namespace xalm;

extern "C" {

// ---------------------------------------------------------------------------------------
// exposed-for-tests ops (host pointers).  They run the same kernels as the forward pass.
// ---------------------------------------------------------------------------------------
namespace {
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) hipFree(p); }
};
int op_alloc(DevBuf& b, size_t bytes, const void* src) {
    if (hipMalloc(&b.p, bytes ? bytes : 16) != hipSuccess) return set_err(nullptr, XH_E_HIP, "hipMalloc failed");
    if (src && hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice) != hipSuccess)
        return set_err(nullptr, XH_E_HIP, "hipMemcpy failed");
    return 0;
}
int op_finish(void* dst, const DevBuf& b, size_t bytes) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_err(nullptr, XH_E_HIP, "kernel launch failed: %s", hipGetErrorString(e));
    if (hipDeviceSynchronize() != hipSuccess) return set_err(nullptr, XH_E_HIP, "kernel failed");
    if (hipMemcpy(dst, b.p, bytes, hipMemcpyDeviceToHost) != hipSuccess)
        return set_err(nullptr, XH_E_HIP, "hipMemcpy D2H failed");
    return 0;
}
// xh_op_kv_quantize: pairs through kv8_pack, the K/V writers' device function (an odd tail with 0)
__global__ __launch_bounds__(256) void kv_quantize_kernel(const float* in, size_t n, uint8_t* out) {
    const size_t pairs = (n + 1) / 2;
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < pairs; p += (size_t)gridDim.x * 256) {
        const bool two = 2 * p + 1 < n;
        const uint32_t pk = kv8_pack(in[2 * p], two ? in[2 * p + 1] : 0.f);
        out[2 * p] = (uint8_t)(pk & 0xffu);
        if (two) out[2 * p + 1] = (uint8_t)(pk >> 8);
    }
}
}  // namespace

int xh_op_matmul(float* xout, const float* x, const void* w, int dtype, int n, int d) {
    if (!xout || !x || !w || n <= 0 || d <= 0 || n % 16) return set_err(nullptr, XH_E_INVALID, "bad matmul args");
    if (!matrix_dtype_ok(dtype)) return set_err(nullptr, XH_E_INVALID, "unsupported dtype %d", dtype);
    DevBuf bw, bx, bo;
    int rc;
    if (gq_dt(dtype) && n % gq_group(dtype)) return set_err(nullptr, XH_E_INVALID, "bad matmul args: n %% %d", gq_group(dtype));
    // gguf blocks: w in the file layout, repacked to the planar device rows
    std::vector<uint8_t> gq_tmp;
    if (gq_mx(dtype)) {
        uint8_t lo, hi;
        mx_e_range((const uint8_t*)w, (size_t)d * (n / 32), &lo, &hi);
        if (hi == 255) return set_err(nullptr, XH_E_INVALID, "bad matmul args: an MXFP4 block with e = 255 (NaN)");
    }
    if (gq_dt(dtype)) {
        gq_tmp.resize((size_t)d * dev_row_bytes(dtype, n));
        gq_repack(dtype, (const uint8_t*)w, d, n, gq_tmp.data());
        w = gq_tmp.data();
    }
    const size_t wbytes = (size_t)d * dev_row_bytes(dtype, n);
    if ((rc = op_alloc(bw, wbytes, w)) || (rc = op_alloc(bx, (size_t)n * 4, x)) || (rc = op_alloc(bo, (size_t)d * 4, nullptr)))
        return rc;
    GemvArgs a{};
    a.w = bw.p; a.row_bytes = dev_row_bytes(dtype, n); a.n = n; a.rows = d;
    a.x = (const float*)bx.p; a.out = (float*)bo.p;
    bool special = false;
    if (dtype == XH_F8_E4M3 || dtype == XH_F8_E5M2)
        for (size_t i = 0; i < wbytes && !special; i++) special = f8_special(((const uint8_t*)w)[i], dtype == XH_F8_E5M2);
    launch_gemv(GEMV_STORE, kdt(dtype, special), a, nullptr, 4096);
    return op_finish(xout, bo, (size_t)d * 4);
}

int xh_op_rmsnorm(float* o, const float* x, const void* weight, int dtype, int size, float eps) {
    if (!o || !x || !weight || size <= 0 || size % 4 || !(dtype == XH_F32 || dtype == XH_BF16))
        return set_err(nullptr, XH_E_INVALID, "bad rmsnorm args");
    DevBuf bw, bx, bo;
    int rc;
    if ((rc = op_alloc(bw, (size_t)size * dtype_size(dtype), weight)) || (rc = op_alloc(bx, (size_t)size * 4, x)) ||
        (rc = op_alloc(bo, (size_t)size * 4, nullptr)))
        return rc;
    hipLaunchKernelGGL(rmsnorm_kernel, dim3(1), dim3(256), 0, nullptr, (float*)bo.p, (const float*)bx.p,
                       (const void*)bw.p, dtype, size, eps);
    return op_finish(o, bo, (size_t)size * 4);
}

int xh_op_rope(float* vec, int d, int head_dim, int pos, float theta, int rotary_dim) {
    if (!vec || d <= 0 || d % 2 || head_dim <= 0 || head_dim % 2) return set_err(nullptr, XH_E_INVALID, "bad rope args");
    std::vector<float> fr(head_dim / 2);
    for (int j = 0; j < head_dim; j += 2)
        fr[j / 2] = j >= rotary_dim ? 0.f : 1.0f / powf(theta, (float)j / (float)rotary_dim);
    DevBuf bv, bf;
    int rc;
    if ((rc = op_alloc(bv, (size_t)d * 4, vec)) || (rc = op_alloc(bf, fr.size() * 4, fr.data()))) return rc;
    hipLaunchKernelGGL(rope_kernel, dim3((d / 2 + 255) / 256), dim3(256), 0, nullptr, (float*)bv.p, d, head_dim, pos,
                       (const float*)bf.p);
    return op_finish(vec, bv, (size_t)d * 4);
}

// xh_op_mha / xh_op_mha8: rings of esz bytes per element through launch_attn, as the decode step
static int op_mha_any(float* xout, const void* kb, const void* vb, const float* q, int head_dim, int kv_len,
                      int max_seq_len, int n_heads, int n_kv_heads, int kv_dt) {
    if (!xout || !kb || !vb || !q || kv_len <= 0 || kv_len > max_seq_len || n_kv_heads <= 0 || n_heads % n_kv_heads)
        return set_err(nullptr, XH_E_INVALID, "bad mha args");
    if (kv_dt == XH_F8_E4M3 && (head_dim <= 0 || head_dim % 16))
        return set_err(nullptr, XH_E_INVALID, "mha8: head_dim %d is no multiple of 16", head_dim);
    const int qpk = n_heads / n_kv_heads, kv_dim = n_kv_heads * head_dim;
    const int nsplit = attn_nsplit(n_kv_heads, max_seq_len);
    const int t_max = attn_split_len(max_seq_len, nsplit);
    DevBuf bk, bv, bq, bo, bpo, bpm, bsp, bcnt;
    std::vector<int> zeros((size_t)n_kv_heads, 0);
    StepParams sp{};
    sp.kv_len = kv_len;
    sp.max_seq_len = max_seq_len;
    int rc;
    const size_t kvb = (size_t)max_seq_len * kv_dim * (kv_dt == XH_F8_E4M3 ? 1 : 2);
    if ((rc = op_alloc(bk, kvb, kb)) || (rc = op_alloc(bv, kvb, vb)) || (rc = op_alloc(bq, (size_t)n_heads * head_dim * 4, q)) ||
        (rc = op_alloc(bo, (size_t)n_heads * head_dim * 4, nullptr)) ||
        (rc = op_alloc(bpo, (size_t)nsplit * n_heads * head_dim * 4, nullptr)) ||
        (rc = op_alloc(bpm, (size_t)nsplit * n_heads * 2 * 4, nullptr)) || (rc = op_alloc(bsp, sizeof sp, &sp)) ||
        (rc = op_alloc(bcnt, zeros.size() * sizeof(int), zeros.data())))
        return rc;
    AttnArgs a{};
    a.q = (const float*)bq.p; a.kc = (const uint16_t*)bk.p; a.vc = (const uint16_t*)bv.p; a.kv_dim = kv_dim;
    a.n_heads = n_heads; a.nsplit = nsplit; a.out = (float*)bo.p; a.part_o = (float*)bpo.p;
    a.part_ml = (float*)bpm.p; a.counters = (int*)bcnt.p; a.sp = (const StepParams*)bsp.p;
    if (!launch_attn(a, head_dim, qpk, n_kv_heads, t_max, nullptr, kv_dt))
        return set_err(nullptr, XH_E_INVALID, "unsupported head_dim %d / qpk %d", head_dim, qpk);
    return op_finish(xout, bo, (size_t)n_heads * head_dim * 4);
}

int xh_op_mha(float* xout, const uint16_t* kb, const uint16_t* vb, const float* q, int head_dim, int kv_len,
              int max_seq_len, int n_heads, int n_kv_heads) {
    return op_mha_any(xout, kb, vb, q, head_dim, kv_len, max_seq_len, n_heads, n_kv_heads, XH_F16);
}

int xh_op_mha8(float* xout, const uint8_t* kb, const uint8_t* vb, const float* q, int head_dim, int kv_len,
               int max_seq_len, int n_heads, int n_kv_heads) {
    return op_mha_any(xout, kb, vb, q, head_dim, kv_len, max_seq_len, n_heads, n_kv_heads, XH_F8_E4M3);
}

int xh_op_kv_quantize(const float* in, size_t n, uint8_t* out) {
    if (!in || !out) return set_err(nullptr, XH_E_INVALID, "bad kv_quantize args");
    if (!n) return 0;
    DevBuf bi, bo;
    int rc;
    if ((rc = op_alloc(bi, n * 4, in)) || (rc = op_alloc(bo, n, nullptr))) return rc;
    hipLaunchKernelGGL(kv_quantize_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, nullptr,
                       (const float*)bi.p, n, (uint8_t*)bo.p);
    return op_finish(out, bo, n);
}

int xh_op_prompt_gemm(float* y, const uint16_t* w, const uint16_t* xh, const uint16_t* xl, int rows, int K, int n,
                      int ks) {
    const bool args_ok = y && w && xh && xl && rows > 0 && n > 0 && K > 0 && ks >= 0 && ks <= 64;
    const int bad = args_ok ? mm_op_ks(rows, K, n, &ks) : 1;  // 1: K % MM_KMULT too
    if (bad == 1) return set_err(nullptr, XH_E_INVALID, "bad prompt_gemm args");
    if (bad) return set_err(nullptr, XH_E_INVALID, "K %d not in %d slices of 64", K, ks);
    DevBuf bw, bx, bo;
    int rc;
    const size_t xe = (size_t)n * K;
    if ((rc = op_alloc(bw, (size_t)rows * K * 2, w)) || (rc = op_alloc(bx, 2 * xe * 2, nullptr)) ||
        (rc = op_alloc(bo, (size_t)ks * n * rows * 4, nullptr)))
        return rc;
    if (hipMemcpy(bx.p, xh, xe * 2, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy((uint16_t*)bx.p + xe, xl, xe * 2, hipMemcpyHostToDevice) != hipSuccess)
        return set_err(nullptr, XH_E_HIP, "hipMemcpy failed");
    int dev = 0, n_cu = 256;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        return set_err(nullptr, XH_E_HIP, "no device");
    mm_op_launch((const uint16_t*)bw.p, (const uint16_t*)bx.p, (const uint16_t*)bx.p + xe, (float*)bo.p, rows, K, n, ks, n_cu);
    std::vector<float> part((size_t)ks * n * rows);
    if ((rc = op_finish(part.data(), bo, part.size() * 4))) return rc;
    for (size_t i = 0; i < (size_t)n * rows; i++) {
        float v = 0.f;
        for (int s = 0; s < ks; s++) v += part[(size_t)s * n * rows + i];  // slice order, as prefill_epi_kernel
        y[i] = v;
    }
    return 0;
}

namespace {
int op_n_cu(int* n_cu) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(n_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        return set_err(nullptr, XH_E_HIP, "no device");
    return 0;
}
// a forced split count against the bound the passes obey over pos0 slots of history
// (and the grid's z extent)
bool op_split_ok(int nsplit, int pos0) { return nsplit <= std::min(pf_fa_split_max(pos0), 65535); }

// xh_op_prompt_attn / xh_op_prompt_attn8: k / v of element type kv_dt (fp16 bits, or one e4m3 code each)
int op_prompt_attn_any(float* out, const float* q, const void* k, const void* v, int n, int pos0, int head_dim, int n_heads,
                       int n_kv_heads, int mode, int nsplit, int kv_dt) {
    if (!out || !q || !k || !v || n <= 0 || pos0 < 0 || pos0 > (1 << 28) || n > (1 << 20) || nsplit < 0)
        return set_err(nullptr, XH_E_INVALID, "bad prompt_attn args");
    if (n_kv_heads <= 0 || n_heads <= 0 || n_heads > 1024 || n_heads % n_kv_heads ||
        !pf_attn_shape_ok(head_dim, n_heads / n_kv_heads))
        return set_err(nullptr, XH_E_INVALID, "prompt_attn: no prompt attention for head_dim %d, %d / %d heads", head_dim,
                       n_heads, n_kv_heads);
    if (mode != 1 && mode != 2) return set_err(nullptr, XH_E_INVALID, "prompt_attn: mode %d (1 or 2)", mode);
    const bool shared = mode == 1 && head_dim == 128;
    if (nsplit > 0 && !shared)
        return set_err(nullptr, XH_E_INVALID, "prompt_attn: splits are forced under mode 1 at head_dim 128 only");
    if (nsplit > 0 && !op_split_ok(nsplit, pos0))
        return set_err(nullptr, XH_E_INVALID, "prompt_attn: %d splits over %d slots (at most %d)", nsplit, pos0,
                       pf_fa_split_max(pos0));
    const PfAttnDims d{head_dim, n_heads, n_kv_heads};
    int rc, n_cu = 0;
    if ((rc = op_n_cu(&n_cu))) return rc;
    if (nsplit == 0) nsplit = shared ? pf_fa_pick_nsplit(d, n_cu, n, pos0, SIZE_MAX) : 1;
    DevBuf bq, bk, bv, bo, bp;
    const size_t qe = (size_t)n * n_heads * head_dim, kve = (size_t)(pos0 + n) * n_kv_heads * head_dim;
    const size_t esz = kv_dt == XH_F8_E4M3 ? 1 : 2;
    if (kv_dt == XH_F8_E4M3)
        for (size_t i = 0; i < kve; i++)
            if (f8_special(((const uint8_t*)k)[i], false) || f8_special(((const uint8_t*)v)[i], false))
                return set_err(nullptr, XH_E_INVALID, "prompt_attn8: element %zu of k or v is the NaN code", i);
    if ((rc = op_alloc(bq, qe * 4, q)) || (rc = op_alloc(bk, kve * esz, k)) || (rc = op_alloc(bv, kve * esz, v)) ||
        (rc = op_alloc(bo, qe * 4, nullptr)) || (rc = op_alloc(bp, nsplit > 1 ? pf_fa_part_floats(d, nsplit, n) * 4 : 0, nullptr)))
        return rc;
    if (pf_fa_launch(d, kv_dt, shared, (const float*)bq.p, (const uint16_t*)bk.p, (const uint16_t*)bv.p, (float*)bo.p, n, pos0, nsplit,
                     (float*)bp.p, nullptr) < 0)
        return set_err(nullptr, XH_E_INVALID, "prompt_attn: head shape not instantiated");
    return op_finish(out, bo, qe * 4);
}
}  // namespace

int xh_op_prompt_attn(float* out, const float* q, const uint16_t* k, const uint16_t* v, int n, int pos0, int head_dim,
                      int n_heads, int n_kv_heads, int mode, int nsplit) {
    return op_prompt_attn_any(out, q, k, v, n, pos0, head_dim, n_heads, n_kv_heads, mode, nsplit, XH_F16);
}
int xh_op_prompt_attn8(float* out, const float* q, const uint8_t* k, const uint8_t* v, int n, int pos0, int head_dim,
                       int n_heads, int n_kv_heads, int mode, int nsplit) {
    return op_prompt_attn_any(out, q, k, v, n, pos0, head_dim, n_heads, n_kv_heads, mode, nsplit, XH_F8_E4M3);
}

namespace {
// xh_op_prompt_attn_ring / xh_op_prompt_attn_ring8: every K/V buffer of element type kv_dt (fp16 bits, or
// one e4m3 code each)
int op_prompt_attn_ring_any(float* out, void* k_ring, void* v_ring, const float* q, const void* ks, const void* vs,
                            const void* sink_ver, int m, int p0, int max_seq_len, int n_heads, int n_kv_heads, int nsplit,
                            int kv_dt) {
    if (!out || !k_ring || !v_ring || !q || !ks || !vs || !sink_ver || nsplit < 0)
        return set_err(nullptr, XH_E_INVALID, "bad prompt_attn_ring args");
    if (n_kv_heads <= 0 || n_heads <= 0 || n_heads > 1024 || n_heads % n_kv_heads || !pf_attn_shape_ok(128, n_heads / n_kv_heads))
        return set_err(nullptr, XH_E_INVALID, "prompt_attn_ring: no ring attention for %d / %d heads", n_heads, n_kv_heads);
    const int W = max_seq_len - 2;
    if (max_seq_len > (1 << 24) || W < 2 || p0 < max_seq_len || m < 3 || m > W)
        return set_err(nullptr, XH_E_INVALID, "prompt_attn_ring: m %d at p0 %d over a ring of %d (3 <= m <= %d, p0 >= %d)", m,
                       p0, max_seq_len, W, max_seq_len);
    if (nsplit > 0 && !op_split_ok(nsplit, W))
        return set_err(nullptr, XH_E_INVALID, "prompt_attn_ring: %d splits over %d slots (at most %d)", nsplit, W,
                       pf_fa_split_max(W));
    const PfAttnDims d{128, n_heads, n_kv_heads};
    const size_t kv_dim = (size_t)n_kv_heads * 128, qe = (size_t)m * n_heads * 128, ring = (size_t)max_seq_len * kv_dim;
    const size_t esz = kv_dt == XH_F8_E4M3 ? 1 : 2;
    if (kv_dt == XH_F8_E4M3) {
        const struct { const char* what; const void* p; size_t n; } bufs[] = {
            {"k_ring", k_ring, ring}, {"v_ring", v_ring, ring}, {"ks", ks, m * kv_dim}, {"vs", vs, m * kv_dim},
            {"sink_ver", sink_ver, 2 * m * kv_dim}};
        for (const auto& b : bufs)
            for (size_t i = 0; i < b.n; i++)
                if (f8_special(((const uint8_t*)b.p)[i], false))
                    return set_err(nullptr, XH_E_INVALID, "prompt_attn_ring8: element %zu of %s is the NaN code", i, b.what);
    }
    int rc, n_cu = 0;
    if ((rc = op_n_cu(&n_cu))) return rc;
    if (nsplit == 0) nsplit = pf_fa_pick_nsplit(d, n_cu, m, W, SIZE_MAX);
    DevBuf bq, bk, bv, bks, bvs, bsv, bo, bp;
    if ((rc = op_alloc(bq, qe * 4, q)) || (rc = op_alloc(bk, ring * esz, k_ring)) || (rc = op_alloc(bv, ring * esz, v_ring)) ||
        (rc = op_alloc(bks, m * kv_dim * esz, ks)) || (rc = op_alloc(bvs, m * kv_dim * esz, vs)) ||
        (rc = op_alloc(bsv, 2 * m * kv_dim * esz, sink_ver)) || (rc = op_alloc(bo, qe * 4, nullptr)) ||
        (rc = op_alloc(bp, pf_fa_part_floats(d, nsplit, m) * 4, nullptr)))
        return rc;
    if (pf_ring_launch(d, kv_dt, (const float*)bq.p, (uint16_t*)bk.p, (uint16_t*)bv.p, (const uint16_t*)bks.p,
                       (const uint16_t*)bvs.p, (const uint16_t*)bsv.p, (float*)bo.p, m, p0, max_seq_len, nsplit, (float*)bp.p,
                       nullptr) < 0)
        return set_err(nullptr, XH_E_INVALID, "prompt_attn_ring: head shape not instantiated");
    if ((rc = op_finish(out, bo, qe * 4))) return rc;
    if (hipMemcpy(k_ring, bk.p, ring * esz, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(v_ring, bv.p, ring * esz, hipMemcpyDeviceToHost) != hipSuccess)
        return set_err(nullptr, XH_E_HIP, "hipMemcpy D2H failed");
    return 0;
}
}  // namespace

int xh_op_prompt_attn_ring(float* out, uint16_t* k_ring, uint16_t* v_ring, const float* q, const uint16_t* ks,
                           const uint16_t* vs, const uint16_t* sink_ver, int m, int p0, int max_seq_len, int n_heads,
                           int n_kv_heads, int nsplit) {
    return op_prompt_attn_ring_any(out, k_ring, v_ring, q, ks, vs, sink_ver, m, p0, max_seq_len, n_heads, n_kv_heads, nsplit,
                                   XH_F16);
}
int xh_op_prompt_attn_ring8(float* out, uint8_t* k_ring, uint8_t* v_ring, const float* q, const uint8_t* ks,
                            const uint8_t* vs, const uint8_t* sink_ver, int m, int p0, int max_seq_len, int n_heads,
                            int n_kv_heads, int nsplit) {
    return op_prompt_attn_ring_any(out, k_ring, v_ring, q, ks, vs, sink_ver, m, p0, max_seq_len, n_heads, n_kv_heads, nsplit,
                                   XH_F8_E4M3);
}

namespace {
// w in the file layout as the device rows of its decode form: the gguf blocks repacked (tmp), fp8
// with NaN / Inf codes as the _EXACT form.  XH_E_INVALID for an MXFP4 block with e = 255.
int op_weight_rows(const char* what, int dtype, const void* w, int rows, int K, std::vector<uint8_t>& tmp, const void** dev_rows,
                   int* dt, bool* wide) {
    *wide = false;
    if (gq_k(dtype) && K % 256) return set_err(nullptr, XH_E_INVALID, "%s: K %d is not in whole 256-element super-blocks", what, K);
    if (gq_mx(dtype)) {
        uint8_t lo, hi;
        mx_e_range((const uint8_t*)w, (size_t)rows * (K / 32), &lo, &hi);
        if (hi == 255) return set_err(nullptr, XH_E_INVALID, "%s: an MXFP4 block with e = 255 (NaN)", what);
        *wide = lo < MX_E_F16_LO || hi > MX_E_F16_HI;
    }
    *dev_rows = w;
    if (gq_dt(dtype)) {
        tmp.resize((size_t)rows * dev_row_bytes(dtype, K));
        gq_repack(dtype, (const uint8_t*)w, rows, K, tmp.data());
        *dev_rows = tmp.data();
    }
    bool special = false;
    if (dtype == XH_F8_E4M3 || dtype == XH_F8_E5M2)
        for (size_t i = 0; i < (size_t)rows * K && !special; i++) special = f8_special(((const uint8_t*)w)[i], dtype == XH_F8_E5M2);
    *dt = kdt(dtype, special);
    return 0;
}
}  // namespace

int xh_op_prompt_matmul(float* y, const float* x, const void* w, int dtype, int rows, int K, int n, int mode, int ks,
                        int* route_out) {
    if (!y || !x || !w || !route_out || rows <= 0 || K <= 0 || n <= 0 || n > 2048 || rows > (1 << 20) || K > (1 << 20) ||
        ks < 0 || ks > 64)
        return set_err(nullptr, XH_E_INVALID, "bad prompt_matmul args");
    if (mode < 1 || mode > 3) return set_err(nullptr, XH_E_INVALID, "prompt_matmul: mode %d (1, 2 or 3)", mode);
    if (!matrix_dtype_ok(dtype)) return set_err(nullptr, XH_E_INVALID, "prompt_matmul: no prompt GEMM for dtype %d", dtype);
    // pf_supported: every GEMM's K in whole chunk pairs of its decoder (the split kernels' 8s follow)
    if (K % (2 * pf_elems(dtype)))
        return set_err(nullptr, XH_E_INVALID, "prompt_matmul: K %d is not in whole chunk pairs of dtype %d", K, dtype);
    std::vector<uint8_t> tmp;
    PfGemmPlan p{};
    const void* hw = nullptr;
    int rc;
    if ((rc = op_weight_rows("prompt_matmul", dtype, w, rows, K, tmp, &hw, &p.dt, &p.wide))) return rc;
    p.mode = mode; p.K = K; p.rows = rows; p.n = n; p.ks = ks;
    if ((rc = op_n_cu(&p.n_cu))) return rc;
    const int route = pf_gemm_route(p);
    if (route != 0 && n > 64) return set_err(nullptr, XH_E_INVALID, "prompt_matmul: %d tokens off the row-major route (at most 64)", n);
    // room for any slicing the route's picker may take (two images of 8 slices; 64 slices)
    p.part_floats = (size_t)(route == 0 ? 16 : 64) * n * rows;
    if (ks > 0 && !pf_gemm_ks_ok(p, route))
        return set_err(nullptr, XH_E_INVALID, "prompt_matmul: %d slices of K %d over %d rows on route %d", ks, K, rows, route);
    const size_t xe = (size_t)n * K, pad = (size_t)32 * ((n + 31) / 32) * K;
    const size_t images = route == 0 && p.dt != XH_F16 ? (gq_dt(p.dt) && !gq_mx(p.dt) ? 2 : 1) : 0;
    DevBuf bw, bx, bxh, bxl, bxs, bq, bp, bo;
    if ((rc = op_alloc(bw, (size_t)rows * dev_row_bytes(dtype, K), hw)) || (rc = op_alloc(bx, xe * 4, x)) ||
        (rc = op_alloc(bxh, (route == 0 ? 2 * xe : route > 0 ? pad : 0) * 2, nullptr)) ||
        (rc = op_alloc(bxl, (route > 0 ? pad : 0) * 2, nullptr)) || (rc = op_alloc(bxs, (size_t)n * 4, nullptr)) ||
        (rc = op_alloc(bq, images * rows * K * 2, nullptr)) || (rc = op_alloc(bp, p.part_floats * 4, nullptr)) ||
        (rc = op_alloc(bo, (size_t)n * rows * 4, nullptr)))
        return rc;
    const PfGemmIo io{bw.p, (const float*)bx.p, (uint16_t*)bxh.p, (uint16_t*)bxl.p, (float*)bxs.p, (uint16_t*)bq.p,
                      images * rows * K, (float*)bp.p};
    int nks = 0;
    if (route >= 0) pf_split_launch(io.x, K, n, route, io.xh, pf_split_lo(route, n, K, io.xh, io.xl), io.xs, nullptr);
    if (route == 0) {
        const uint16_t *w_hi = nullptr, *w_lo = nullptr;
        if (!(rc = pf_gemm_images(p, io, &w_hi, &w_lo, nullptr))) rc = pf_gemm_rowmajor(p, io, w_hi, w_lo, &nks, nullptr);
    } else {
        rc = route > 0 ? pf_gemm_frag(p, io, route, &nks, nullptr) : pf_gemm_f32(p, io, &nks, nullptr);
    }
    if (rc) {
        hipDeviceSynchronize();
        return set_err(nullptr, XH_E_INVALID, "prompt_matmul: the launch code refused the GEMM (%d)", rc);
    }
    // the row-major partials are unscaled: the epilogue multiplies by 1 / s_t, as a pass's
    pf_epi_plain_launch(io.part, route == 0 ? io.xs : nullptr, nks, n, rows, EPI_STORE, (float*)bo.p, 0, 0, nullptr);
    *route_out = route;
    return op_finish(y, bo, (size_t)n * rows * 4);
}

int xh_op_prompt_weight_image(int dtype, const void* w, int rows, int K, uint16_t* hi_out, uint16_t* lo_out, int max_groups) {
    const bool one = dtype == XH_F8_E4M3 || dtype == XH_F8_E5M2 || dtype == XH_MXFP4;
    const bool two = dtype == XH_Q8_0 || dtype == XH_Q4_0 || dtype == XH_Q5_0;
    if (!w || !hi_out || rows <= 0 || K <= 0 || K % 32 || rows > (1 << 20) || K > (1 << 20) || max_groups < 0)
        return set_err(nullptr, XH_E_INVALID, "bad prompt_weight_image args");
    if (!(one || two) || (two && !lo_out) || (one && lo_out))
        return set_err(nullptr, XH_E_INVALID, "prompt_weight_image: dtype %d has %s", dtype,
                       one ? "one image (lo_out NULL)" : two ? "two images" : "no f16 image");
    std::vector<uint8_t> tmp;
    PfGemmPlan p{};
    const void* hw = nullptr;
    int rc;
    if ((rc = op_weight_rows("prompt_weight_image", dtype, w, rows, K, tmp, &hw, &p.dt, &p.wide))) return rc;
    if (p.wide || p.dt != dtype)
        return set_err(nullptr, XH_E_INVALID, "prompt_weight_image: the matrix has no exact f16 image (%s)",
                       p.wide ? "an MXFP4 scale outside the f16 range" : "a NaN / Inf code");
    p.mode = 1; p.K = K; p.rows = rows; p.max_groups = max_groups;
    const size_t we = (size_t)rows * K, images = two ? 2 : 1;
    DevBuf bw, bq;
    if ((rc = op_alloc(bw, (size_t)rows * dev_row_bytes(dtype, K), hw)) || (rc = op_alloc(bq, images * we * 2, nullptr))) return rc;
    const PfGemmIo io{bw.p, nullptr, nullptr, nullptr, nullptr, (uint16_t*)bq.p, images * we, nullptr};
    const uint16_t *w_hi = nullptr, *w_lo = nullptr;
    if ((rc = pf_gemm_images(p, io, &w_hi, &w_lo, nullptr)))
        return set_err(nullptr, XH_E_INVALID, "prompt_weight_image: the launch code refused the image (%d)", rc);
    if ((rc = op_finish(hi_out, bq, we * 2))) return rc;
    if (two && hipMemcpy(lo_out, w_lo, we * 2, hipMemcpyDeviceToHost) != hipSuccess)
        return set_err(nullptr, XH_E_HIP, "hipMemcpy D2H failed");
    return 0;
}

int xh_op_prompt_stage(int kind, const float* part, int ks, const float* part_s, float* x, int n, int dim, const void* norm_w,
                       int norm_dtype, float eps, int act, int layout, size_t out_stride, float* y_out, float* inv_s_out,
                       uint16_t* hi_out, uint16_t* lo_out, int* pad_out) {
    const bool store = kind == XH_STAGE_STORE;
    const bool from_x = kind == XH_STAGE_SPLIT || kind == XH_STAGE_NORM_SPLIT;
    const bool resid = kind == XH_STAGE_RESID_NORM_SPLIT || kind == XH_STAGE_RESID_THEN_NORM_SPLIT;
    const bool glu = kind == XH_STAGE_GLU_SPLIT || kind == XH_STAGE_GLU_THEN_SPLIT;
    const bool normed = kind == XH_STAGE_NORM_SPLIT || resid;
    if (!(store || from_x || resid || glu) || n <= 0 || n > 2048 || dim <= 0 || dim > 16000 || ks < 1 || ks > 64)
        return set_err(nullptr, XH_E_INVALID, "bad prompt_stage args");
    if ((!from_x && !part) || ((from_x || resid) && !x) || (normed && !norm_w) || (store && !y_out) ||
        (!store && (!inv_s_out || !hi_out || !lo_out || !pad_out)))
        return set_err(nullptr, XH_E_INVALID, "prompt_stage: a buffer of kind %d is NULL", kind);
    if (normed && !(norm_dtype == XH_F32 || norm_dtype == XH_BF16))
        return set_err(nullptr, XH_E_INVALID, "prompt_stage: norm weight dtype %d", norm_dtype);
    // the producers move 8 elements at a time; a fragment layout holds whole chunk pairs
    if (!store && (!(layout == 0 || layout == 8 || layout == 16) || dim % (layout ? 2 * layout : 8)))
        return set_err(nullptr, XH_E_INVALID, "prompt_stage: rows of %d in layout %d (0, 8 or 16; whole 8s / chunk pairs)", dim,
                       layout);
    if (store && out_stride && out_stride < (size_t)dim) return set_err(nullptr, XH_E_INVALID, "prompt_stage: out_stride < rows");
    if (glu && act != XH_ACT_SILU && act != XH_ACT_GELU) return set_err(nullptr, XH_E_INVALID, "prompt_stage: act %d", act);
    const size_t prow = glu ? 2 * (size_t)dim : (size_t)dim;  // a row of the partials
    const size_t ne = (size_t)n * dim, stride = out_stride ? out_stride : (size_t)dim;
    const int tpad = layout ? 32 * ((n + 31) / 32) : n;
    const size_t he = (size_t)tpad * dim;  // f16 per half
    DevBuf bp, bps, bx, bw, bh, bxh, bxl, bxs, by;
    int rc;
    if ((rc = op_alloc(bp, from_x ? 0 : (size_t)ks * n * prow * 4, from_x ? nullptr : part)) ||
        (rc = op_alloc(bps, (size_t)n * 4, part_s)) || (rc = op_alloc(bx, ne * 4, from_x || resid ? x : nullptr)) ||
        (rc = op_alloc(bw, normed ? (size_t)dim * dtype_size(norm_dtype) : 0, normed ? norm_w : nullptr)) ||
        (rc = op_alloc(bh, ne * 4, nullptr)) || (rc = op_alloc(bxh, (layout ? he : 2 * he) * 2, nullptr)) ||
        (rc = op_alloc(bxl, he * 2, nullptr)) || (rc = op_alloc(bxs, (size_t)n * 4, nullptr)) ||
        (rc = op_alloc(by, store ? (size_t)n * stride * 4 : 0, store ? y_out : nullptr)))
        return rc;
    // halves start as all ones: a padding row the producer does not zero shows in *pad_out
    if (hipMemset(bxh.p, 0xff, (layout ? he : 2 * he) * 2) != hipSuccess || hipMemset(bxl.p, 0xff, he * 2) != hipSuccess)
        return set_err(nullptr, XH_E_HIP, "hipMemset failed");
    const float* ps = part_s ? (const float*)bps.p : nullptr;
    float* dx = (float*)bx.p;
    uint16_t* xh = (uint16_t*)bxh.p;
    uint16_t* xl = pf_split_lo(layout, n, dim, xh, (uint16_t*)bxl.p);
    float* xs = (float*)bxs.p;
    switch (kind) {
        case XH_STAGE_SPLIT: pf_split_launch(dx, dim, n, layout, xh, xl, xs, nullptr); break;
        case XH_STAGE_NORM_SPLIT: pf_norm_split_launch(dx, dim, bw.p, norm_dtype, eps, n, layout, xh, xl, xs, nullptr); break;
        case XH_STAGE_RESID_NORM_SPLIT:
            pf_resid_norm_split_launch((const float*)bp.p, ks, ps, dx, dim, bw.p, norm_dtype, eps, n, layout, xh, xl, xs, nullptr);
            break;
        case XH_STAGE_RESID_THEN_NORM_SPLIT:
            pf_epi_plain_launch((const float*)bp.p, ps, ks, n, dim, EPI_RESID, dx, 0, 0, nullptr);
            pf_norm_split_launch(dx, dim, bw.p, norm_dtype, eps, n, layout, xh, xl, xs, nullptr);
            break;
        case XH_STAGE_GLU_SPLIT:
            pf_glu_split_launch((const float*)bp.p, ks, ps, n, dim, act, layout, xh, xl, xs, nullptr);
            break;
        case XH_STAGE_GLU_THEN_SPLIT:
            pf_epi_plain_launch((const float*)bp.p, ps, ks, n, 2 * dim, EPI_GLU, (float*)bh.p, 0, act, nullptr);
            pf_split_launch((const float*)bh.p, dim, n, layout, xh, xl, xs, nullptr);
            break;
        default:
            pf_epi_plain_launch((const float*)bp.p, ps, ks, n, dim, EPI_STORE, (float*)by.p, out_stride, 0, nullptr);
            return op_finish(y_out, by, (size_t)n * stride * 4);
    }
    if ((rc = op_finish(inv_s_out, bxs, (size_t)n * 4))) return rc;
    if (resid && hipMemcpy(x, bx.p, ne * 4, hipMemcpyDeviceToHost) != hipSuccess)
        return set_err(nullptr, XH_E_HIP, "hipMemcpy D2H failed");
    std::vector<uint16_t> hh(he), hl(he);
    if (hipMemcpy(hh.data(), xh, he * 2, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(hl.data(), xl, he * 2, hipMemcpyDeviceToHost) != hipSuccess)
        return set_err(nullptr, XH_E_HIP, "hipMemcpy D2H failed");
    int padnz = 0;
    for (int t = 0; t < tpad; t++)
        for (int k = 0; k < dim; k += 8) {
            const size_t o = pf_split_index(t, k, dim, layout);
            for (int j = 0; j < 8; j++) {
                if (t < n) {
                    hi_out[(size_t)t * dim + k + j] = hh[o + j];
                    lo_out[(size_t)t * dim + k + j] = hl[o + j];
                } else {
                    padnz += (hh[o + j] != 0) + (hl[o + j] != 0);
                }
            }
        }
    *pad_out = padnz;
    return 0;
}

int xh_prompt_gemm_tile(int route) { return pf_gemm_row_tile(route); }

// ---------------------------------------------------------------------------------------
// timing hooks for bench.py
// ---------------------------------------------------------------------------------------
int xh_time_kernel(xh_ctx* ctx, int which, int iters, float* avg_us) {
    if (!ctx || !avg_us || iters <= 0 || which < 0 || which > 11) return XH_E_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->dev));
    int rc = check_ready(ctx);
    if (rc) return rc;
    // the constrained head reads its tables through the block xh_decode_sample_dfa writes
    if (which == 8 && !(ctx->dfa_vocab_set && ctx->dfa_n_states && ctx->dfa_block_valid))
        return set_err(ctx, XH_E_STATE, "xh_time_kernel 8: no xh_decode_sample_dfa call under the current constraint");
    // likewise the adaptive head, its constraint included when the last call had one
    if (which == 10 && !(ctx->adapt_valid && (!ctx->adapt_constrain ||
                                              (ctx->dfa_vocab_set && ctx->dfa_n_states && ctx->dfa_block_valid))))
        return set_err(ctx, XH_E_STATE, "xh_time_kernel 10: no xh_decode_sample_adapt call under the current constraint");
    // the sequence-aware head reads ctx->adapt and ctx->dfa too: the constraint that counts is the one
    // last written to ctx->adapt, by either loop
    if (which == 11 && !(ctx->seq_valid && (!(ctx->seq_constrain || ctx->adapt_constrain) ||
                                            (ctx->dfa_vocab_set && ctx->dfa_n_states && ctx->dfa_block_valid))))
        return set_err(ctx, XH_E_STATE, "xh_time_kernel 11: no xh_decode_sample_seq call under the current constraint");
    if (which == 9 && ctx->top_n <= 0) return set_err(ctx, XH_E_STATE, "xh_time_kernel 9: xh_set_top_logprobs is 0");
    const int mb = ctx->max_gemv_waves;
    // launches rotate over the layers, so a repeat never finds its weights in the 256 MB
    // Infinity Cache (a decode step streams every layer once)
    int rot = 0;
    auto launch = [&]() -> bool {
        const int l = rot++ % ctx->c.n_layers;
        switch (which) {
            case 0: return launch_gemv(GEMV_GLU, kdt(ctx->L[l].w13_dt, ctx->L[l].w13_x), w13_args(ctx, l), ctx->stream, mb);
            case 1: return launch_gemv(qkv_role(ctx), kdt(ctx->L[l].qkv_dt, ctx->L[l].qkv_x), qkv_args(ctx, l), ctx->stream,
                                                             qkv_launch_waves(ctx, l));
            case 2: return launch_gemv(GEMV_RESID, kdt(ctx->L[l].wo_dt, ctx->L[l].wo_x), wo_args(ctx, l), ctx->stream, mb);
            case 3: return launch_gemv(GEMV_RESID, kdt(ctx->L[l].w2_dt, ctx->L[l].w2_x), w2_args(ctx, l), ctx->stream, mb);
            case 4: return launch_gemv(GEMV_LOGITS, kdt(ctx->wcls_dt, ctx->wcls_x), cls_args(ctx), ctx->stream, mb);
            case 6: time_head(ctx, STEP_SAMPLE); return true;
            case 7: time_head(ctx, STEP_SAMPLE_EXT); return true;
            case 8: time_head(ctx, STEP_SAMPLE_DFA); return true;
            case 9: time_top_logprobs(ctx); return true;
            case 10: time_head(ctx, STEP_SAMPLE_ADAPT); return true;
            case 11: time_head(ctx, STEP_SAMPLE_SEQ); return true;
            default:
                return launch_attn(attn_args(ctx, l), ctx->c.head_dim, ctx->qpk, ctx->c.n_kv_heads, ctx->t_max,
                                   ctx->stream, ctx->kv_dt);
        }
    };
    hipEvent_t e0, e1;
    HIP_TRY(ctx, hipEventCreate(&e0));
    HIP_TRY(ctx, hipEventCreate(&e1));
    for (int i = 0; i < 3; i++) launch();
    HIP_TRY(ctx, hipEventRecord(e0, ctx->stream));
    for (int i = 0; i < iters; i++) launch();
    HIP_TRY(ctx, hipEventRecord(e1, ctx->stream));
    HIP_TRY(ctx, hipEventSynchronize(e1));
    float ms = 0.f;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, e0, e1));
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    HIP_TRY(ctx, hipGetLastError());
    *avg_us = ms * 1000.f / (float)iters;
    return 0;
}

size_t xh_kernel_bytes(const xh_ctx* ctx, int which, int kv_len) {
    if (!ctx) return 0;
    const xh_config& c = ctx->c;
    const LayerW& w = ctx->L[0];
    const size_t vec = 4;
    switch (which) {
        case 0: return (size_t)2 * c.hidden_dim * file_row_bytes(w.w13_dt, c.dim) + c.dim * (vec + dtype_size(w.fn_dt)) +
                       (size_t)c.hidden_dim * vec;
        case 1: return (size_t)(ctx->q_dim + 2 * ctx->kv_dim) * file_row_bytes(w.qkv_dt, c.dim) +
                       c.dim * (vec + dtype_size(w.an_dt)) + (size_t)ctx->q_dim * vec + 2 * ctx->kv_dim * ctx->kv_esz();
        case 2: return (size_t)c.dim * file_row_bytes(w.wo_dt, ctx->q_dim) + ctx->q_dim * vec + 2 * c.dim * vec;
        case 3: return (size_t)c.dim * file_row_bytes(w.w2_dt, c.hidden_dim) + c.hidden_dim * vec + 2 * c.dim * vec;
        case 4: return (size_t)c.vocab_size * file_row_bytes(ctx->wcls ? ctx->wcls_dt : ctx->embed_dt, c.dim) +
                       c.dim * (vec + dtype_size(ctx->final_norm_dt)) + (size_t)c.vocab_size * vec;
        case 6: return (size_t)c.vocab_size * vec + file_row_bytes(ctx->embed_dt, c.dim) + c.dim * vec;
        case 7: return (size_t)2 * c.vocab_size * vec + file_row_bytes(ctx->embed_dt, c.dim) + c.dim * vec;
        case 9: return (size_t)c.vocab_size * vec + (size_t)2 * ctx->top_n * vec;
        default: return (size_t)2 * kv_len * ctx->kv_dim * ctx->kv_esz() + 2 * (size_t)ctx->q_dim * vec;
    }
}

}  // extern "C"
