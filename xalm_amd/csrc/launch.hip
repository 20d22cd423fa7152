// launch.hip — launch dispatch of the decode kernels: every gemv_kernel (gemv.h) and
// attn_split_kernel (attention.h) instantiation lives in this translation unit.
#include <hip/hip_runtime.h>

#include <mutex>
#include <set>

#include "ctx.h"

using namespace xalm;

// the attribute belongs to the device current at the call; a failure is not recorded, so the
// next launch tries again
bool xalm::ensure_lds(const void* fn, const int bytes) {
    static std::mutex mu;
    static std::set<std::pair<const void*, int>> done;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return false;
    std::lock_guard<std::mutex> g(mu);
    if (done.count({fn, dev})) return true;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return false;
    done.insert({fn, dev});
    return true;
}

namespace {

constexpr int ROWS = 2;  // rows per wave (even: rope pairs, gate/up pairs)
constexpr int UNROLL = 4;

// ---------------------------------------------------------------------------------------
// gemv launch dispatch
// ---------------------------------------------------------------------------------------
// Shapes, chosen with tools/gemv_bench.hip and tools/chain_bench.hip on MI355X
// (profiles/r01_gemv_bench.txt, profiles/r01_chain_bench.txt): 512-thread blocks (8 waves share
// one x image), 2 rows x 4 chunks in flight per wave, non-temporal weight loads, 16 waves per
// CU.  PF shapes hold x in registers (XN float4 per thread) and request the first weight chunks
// inside the prologue (-5.7 % per decode layer); the plain shape covers every other n.
using ShapeShort = GemvShape<512, ROWS, UNROLL, true, 4, false>;
using ShapeLong = GemvShape<512, ROWS, UNROLL, true, 4, false>;
// MXFP4 on the staged shapes: 2 chunks in flight.  A chunk is 32 converted values against 32 x
// floats per row; at 4 chunks x 2 rows the instantiation needs more than the 128 VGPRs of 4 waves
// per SIMD (hipcc: 24 - 31 spilled), at 2 it takes 106 - 126 and spills none.
// The K-quants (Q4_K / Q6_K) take it too: at 4 chunks hipcc spills 44 - 64 (Q4_K: the unpacked
// {d*sc, -dmin*mn} per chunk and row) and 148 - 164 bytes per lane (Q6_K: two scales and two plane
// words), at 2 chunks none (Q4_K 106 - 116 VGPRs, Q6_K 123 - 126).
using ShapeStagedMx = GemvShape<512, ROWS, 2, true, 4, false>;
using ShapePF2 = GemvShape<512, ROWS, UNROLL, true, 4, true, 2>;  // n <= 4096
using ShapePF8 = GemvShape<512, ROWS, UNROLL, true, 4, true, 8>;  // n <= 16384 (W2 / Wo inputs)

template <int DT, int PRO, int EPI, class S>
bool launch_gemv_s(const GemvArgs& a, hipStream_t s, int max_waves) {
    const size_t smem = gemv_smem_bytes<DT, S>(a.n);
    const int blocks = gemv_blocks<S>(a.rows, max_waves / S::WAVES);
    auto k = gemv_kernel<DT, PRO, EPI, S>;
    if (smem > GEMV_LDS_MAX) return false;  // xh_create refuses such a config (gemv_lds_bytes)
    if (smem > 64 * 1024 && !ensure_lds((const void*)k)) return false;
    hipLaunchKernelGGL(k, dim3(blocks), dim3(S::THREADS), smem, s, a);
    return true;
}

// pipelined PF shape (gemv_rows_pipe: the next row step requested before the current one is
// multiplied, across row groups too) for the qkv and W1/W3 launches: fp8 Mistral-7B decode
// 568 -> 584 tok/s (their 4 KiB rows are one step per group, so a wave drained to zero at
// every group), f16 unchanged (383 / 383); W2, Wo and lm_head unchanged either way
using ShapePF2P = GemvShape<512, ROWS, UNROLL, true, 4, true, 2, 2>;  // n <= 4096
// qkv with 2-byte weights (QKV_T384): 384-thread workgroups, two per CU, every wave ONE row group
// at 3072 waves (tools/gemv_bench GB_BAL: 10.29 -> 9.95 us f16; fp8 rows are one step: no gain)
using ShapeQ384 = GemvShape<384, ROWS, UNROLL, true, 3, true, 3, 2>;  // n <= 4608
#ifndef QKV_T384
#define QKV_T384 1
#endif
// W2-long rows of one-byte weights (W2_T1024): one 1024-thread workgroup per CU, one row per
// wave, hb in 4 float4 per thread (tools/gemv_bench GB_W2, fp8 Mistral W2: 12.58 -> 11.99 us;
// f16 no gain)
using ShapeW2K = GemvShape<1024, 1, UNROLL, true, 4, true, 4, 1>;  // n <= 16384
#ifndef W2_T1024
#define W2_T1024 1
#endif
#ifndef GEMV_BAL_GQ_GLU
#define GEMV_BAL_GQ_GLU 1
#endif
#ifndef GEMV_BAL_FP8_QKV
#define GEMV_BAL_FP8_QKV 1
#endif


// The launch shape of one (dtype, prologue, epilogue) at input length n: the one selection, read by
// the launcher below and by xh_gemv_shape.  HAS_*: the shapes this instance can take at all (the
// launcher instantiates no others).
enum {
    SH_Q384 = XH_SHAPE_Q384, SH_PF2PB = XH_SHAPE_PF2PB, SH_PF2P = XH_SHAPE_PF2P, SH_GQ = XH_SHAPE_GQ, SH_GQL = XH_SHAPE_GQL,
    SH_PF2 = XH_SHAPE_PF2, SH_W2K = XH_SHAPE_W2K, SH_PF8 = XH_SHAPE_PF8, SH_SHORT = XH_SHAPE_SHORT, SH_LONG = XH_SHAPE_LONG
};
template <int DT, int PRO, int EPI>
struct ShapeSel {
    static constexpr int E = WDec<DT>::E;
    static constexpr bool GQ = gq_dt(DT);
    static constexpr bool HAS_PF2P = (epi_qkv(EPI) || EPI == EPI_GLU) && !GQ;
    static constexpr bool HAS_Q384 = HAS_PF2P && epi_qkv(EPI) && E <= 8 && QKV_T384;
    static constexpr bool HAS_PF2PB = HAS_PF2P && epi_qkv(EPI) && E >= 16 && GEMV_BAL_FP8_QKV;
    static constexpr bool HAS_GQL = GQ && PRO == PRO_PLAIN;
    static constexpr bool HAS_W2K = PRO == PRO_PLAIN && EPI == EPI_RESID && E >= 16 && W2_T1024;
    static constexpr bool HAS_PF8 = PRO == PRO_PLAIN && !HAS_W2K;
    static constexpr bool HAS_SHORT = PRO != PRO_PLAIN;
    // gguf blocks take the staged shapes (4 rows per wave measured slower: Q8_0 442 -> 303 tok/s,
    // Q4_0 560 -> 506): the nibble types (Q4_0, Q4_1, Q5_0, Q5_1) hold 32 elements per chunk.
    // Q4_0 rows of a 4096-wide input are 2 chunks, so 2 chunks per step; W2-long inputs (14336:
    // 14 / 7 chunks per row) step by 2 (Q8_0) / 1 (Q4_0) chunks
    static constexpr int UG = E == 32 ? 2 : UNROLL;
    static constexpr int UL = E == 32 ? 1 : 2;

    static int pick(const int n) {
        // PF needs whole first chunks (n >= 64 E U) and x in XN float4 per thread
        const bool pf = !GQ && n % 4 == 0 && n >= 64 * E * UNROLL;
        if constexpr (HAS_PF2P) {
            const bool whole = pf && n % (64 * E * UNROLL) == 0;
            if constexpr (HAS_Q384) {
                if (whole && n / 4 <= 3 * 384) return SH_Q384;
            }
            if constexpr (HAS_PF2PB) {
                if (whole && n / 4 <= 2 * 512) return SH_PF2PB;
            }
            if (whole && n / 4 <= 2 * 512) return SH_PF2P;
        }
        if constexpr (GQ) {
            if (n % 4 == 0 && n / 4 <= 2 * 512 && n % (64 * E * UG) == 0) return SH_GQ;
            if constexpr (HAS_GQL) {
                if (n % 4 == 0 && n / 4 <= 8 * 512 && n % (64 * E * UL) == 0) return SH_GQL;
            }
        }
        if (pf && n / 4 <= 2 * 512) return SH_PF2;
        if constexpr (HAS_W2K) return pf && n / 4 <= 4 * 1024 ? SH_W2K : SH_LONG;
        else if constexpr (PRO == PRO_PLAIN) return pf && n / 4 <= 8 * 512 ? SH_PF8 : SH_LONG;
        else return gemv_smem_bytes<DT, ShapeShort>(n) <= 40 * 1024 ? SH_SHORT : SH_LONG;
    }
};

template <int DT, int PRO, int EPI>
bool launch_gemv_t(const GemvArgs& a, hipStream_t s, int max_waves) {
    using Sel = ShapeSel<DT, PRO, EPI>;
    switch (Sel::pick(a.n)) {
        case SH_Q384:
            if constexpr (Sel::HAS_Q384) return launch_gemv_s<DT, PRO, EPI, ShapeQ384>(a, s, 3 * (max_waves / 2));
            break;
        case SH_PF2PB:
            if constexpr (Sel::HAS_PF2PB) {
                // one-byte qkv rows: 3072 one-step groups, 512 workgroups of 6 busy waves (fp8 qkv
                // 7.3 -> 7.1 us, decode +0.5 %, profiles/r06_decode_ab.txt ab9)
                using ShapePF2PB = GemvShape<512, ROWS, UNROLL, true, 4, true, 2, 2, true>;
                return launch_gemv_s<DT, PRO, EPI, ShapePF2PB>(a, s, max_waves);
            }
            break;
        case SH_PF2P:
            if constexpr (Sel::HAS_PF2P) return launch_gemv_s<DT, PRO, EPI, ShapePF2P>(a, s, max_waves);
            break;
        case SH_GQ:
            if constexpr (Sel::GQ) {
                // gguf blocks: the pipelined PF shapes with the block scales loaded beside the codes.
                // W1/W3 (GEMV_BAL_GQ_GLU): balanced grid, Q4_0 15.0 -> 14.0 us (profiles/r06_decode_ab.txt ab8)
                using ShapeGQ = GemvShape<512, ROWS, Sel::UG, true, 4, true, 2, 2, EPI == EPI_GLU && GEMV_BAL_GQ_GLU>;
                return launch_gemv_s<DT, PRO, EPI, ShapeGQ>(a, s, max_waves);
            }
            break;
        case SH_GQL:
            if constexpr (Sel::HAS_GQL) {
                using ShapeGQL = GemvShape<512, ROWS, Sel::UL, true, 4, true, 8, 2>;
                return launch_gemv_s<DT, PRO, EPI, ShapeGQL>(a, s, max_waves);
            }
            break;
        case SH_PF2: return launch_gemv_s<DT, PRO, EPI, ShapePF2>(a, s, max_waves);
        case SH_W2K:
            if constexpr (Sel::HAS_W2K) return launch_gemv_s<DT, PRO, EPI, ShapeW2K>(a, s, max_waves);
            break;
        case SH_PF8:
            if constexpr (Sel::HAS_PF8) return launch_gemv_s<DT, PRO, EPI, ShapePF8>(a, s, max_waves);
            break;
        case SH_SHORT:
            if constexpr (Sel::HAS_SHORT) return launch_gemv_s<DT, PRO, EPI, std::conditional_t<gq_mx(DT) || gq_k(DT), ShapeStagedMx, ShapeShort>>(a, s, max_waves);
            break;
        case SH_LONG: return launch_gemv_s<DT, PRO, EPI, std::conditional_t<gq_mx(DT) || gq_k(DT), ShapeStagedMx, ShapeLong>>(a, s, max_waves);
    }
    return false;
}

// what launch_gemv_dt does with a (dtype, length): F = Launch (run it) or Pick (name its shape)
template <int PRO, int EPI>
struct Launch {
    const GemvArgs& a; hipStream_t s; int max_waves;
    template <int DT> int run() const { return launch_gemv_t<DT, PRO, EPI>(a, s, max_waves) ? 1 : 0; }
};
template <int PRO, int EPI>
struct Pick {
    int n;
    template <int DT> int run() const {
        const size_t smem = gemv_smem_bytes<DT, ShapeLong>(n);  // the same for every shape
        if (smem > GEMV_LDS_MAX) return -1;
        return ShapeSel<DT, PRO, EPI>::pick(n) | (smem > 64 * 1024 ? XH_SHAPE_BIG_LDS : 0);
    }
};
// every role as its (prologue, epilogue) pair
template <template <int, int> class F, class... A>
int for_role(int role, int dt, A... args) {
    switch (role) {
        case GEMV_QKV: return for_dt(dt, F<PRO_RMSNORM, EPI_QKV>{args...});
        case GEMV_GLU: return for_dt(dt, F<PRO_RMSNORM, EPI_GLU>{args...});
        case GEMV_RESID: return for_dt(dt, F<PRO_PLAIN, EPI_RESID>{args...});
        case GEMV_LOGITS: return for_dt(dt, F<PRO_RMSNORM, EPI_LOGITS>{args...});
        case GEMV_STORE: return for_dt(dt, F<PRO_PLAIN, EPI_STORE>{args...});
        case GEMV_QKV8: return for_dt(dt, F<PRO_RMSNORM, EPI_QKV8>{args...});
    }
    return -1;
}

}  // namespace

bool xalm::launch_gemv(GemvRole role, int dt, const GemvArgs& a, hipStream_t s, int max_waves) {
    return for_role<Launch, const GemvArgs&, hipStream_t, int>(role, dt, a, s, max_waves) == 1;
}

int xalm::gemv_shape(int role, int dt, int n) {
    if (n <= 0 || n % 32) return -1;
    return for_role<Pick, int>(role, dt, n);
}

namespace {

// ---------------------------------------------------------------------------------------
// attention launch dispatch
// ---------------------------------------------------------------------------------------
template <int HD, int QPK, int KV>
void launch_attn_t(const AttnArgs& a, int n_kv_heads, int t_max, hipStream_t s) {
    const size_t smem = attn_smem_bytes(HD, QPK, t_max, a.nsplit);
    auto k = attn_split_kernel<HD, QPK, KV>;
    if (smem > 64 * 1024) ensure_lds((const void*)k);
    hipLaunchKernelGGL(k, dim3(n_kv_heads, a.nsplit), dim3(ATTN_THREADS), smem, s, a);
}

template <int HD, int KV>
bool launch_attn_hd(const AttnArgs& a, int qpk, int n_kv_heads, int t_max, hipStream_t s) {
    return for_qpk(qpk, [&](auto Q) {
        launch_attn_t<HD, decltype(Q)::value, KV>(a, n_kv_heads, t_max, s);
        return 0;
    }) == 0;
}
template <int KV>
bool launch_attn_kv(const AttnArgs& a, int hd, int qpk, int n_kv_heads, int t_max, hipStream_t s) {
    switch (hd) {
        case 16: return launch_attn_hd<16, KV>(a, qpk, n_kv_heads, t_max, s);
        case 32: return launch_attn_hd<32, KV>(a, qpk, n_kv_heads, t_max, s);
        case 64: return launch_attn_hd<64, KV>(a, qpk, n_kv_heads, t_max, s);
        case 128: return launch_attn_hd<128, KV>(a, qpk, n_kv_heads, t_max, s);
        case 256: return launch_attn_hd<256, KV>(a, qpk, n_kv_heads, t_max, s);
        default: return false;
    }
}

}  // namespace

bool xalm::launch_attn(const AttnArgs& a, int hd, int qpk, int n_kv_heads, int t_max, hipStream_t s, int kv_dt) {
    return kv_dt == XH_F8_E4M3 ? launch_attn_kv<XH_F8_E4M3>(a, hd, qpk, n_kv_heads, t_max, s)
                               : launch_attn_kv<XH_F16>(a, hd, qpk, n_kv_heads, t_max, s);
}

int xalm::attn_nsplit(int n_kv_heads, int max_seq_len) {
    // one split workgroup per CU at the longest context (tools/attn_bench.hip, 32k: 32 splits
    // per KV head 34.9 us vs 64 splits 39.0 us)
#ifndef ATTN_SPLIT_WGS
#define ATTN_SPLIT_WGS 256
#endif
    int ns = ATTN_SPLIT_WGS / n_kv_heads;
    if (ns > 128) ns = 128;  // the merge holds <= 2 partials per lane
#ifndef ATTN_CAP_T
#define ATTN_CAP_T ATTN_MIN_T
#endif
    const int cap = (max_seq_len + ATTN_CAP_T - 1) / ATTN_CAP_T;
    if (ns > cap) ns = cap;
    return ns < 1 ? 1 : ns;
}
