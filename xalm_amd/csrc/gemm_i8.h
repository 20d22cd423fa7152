// gemm_i8.h — the integer prompt-pass GEMM for the 32-element gguf block weights Q8_0 / Q4_0 / Q4_1 / Q5_0 /
// Q5_1 against activations quantised per block to int8 (XH_OPT_PREFILL_I8), beside gemm_gq.h.  Where gemm_gq.h
// widens the codes to f16 and multiplies them by the f16 hi + lo halves (two v_mfma_f32_16x16x32_f16 per
// block), this family rounds the activations to 8 bits per block (ggml's Q8_1) and multiplies in integers: one
// v_mfma_i32_16x16x32_i8, exactly one block deep, from a zero C.  It changes the math beyond f32 rounding.
//
// The quantiser (prefill_quant_q8_kernel), per token t and block b of the layout-0 halves xh, xl under the
// power-of-two row scale s_t, every operation one IEEE f32 operation, none contracted:
//   v_k = xh + xl (exact)   amax = max |v_k|   inv = amax > 0 ? 127.0f / amax : 0
//   qx_k = (int8) rintf(v_k * inv) clamped to +-127   dx = amax / 127.0f   sx = dx * (float) sum_k qx_k
// A token row of its output: the int8 codes [K], then {dx, sx} per block as f32 (pitch K + K / 4 bytes).  Two
// lanes per block, 16 elements each: four 16-byte loads, one 16-byte store of codes, amax and the integer sum
// through one cross-lane exchange each.  It runs once per GEMM input of a pass, on the pass's stream.
//
// The GEMM, per weight row r, token t, K slice, blocks in ascending order, from acc = 0:
//   Q8_0, Q4_0, Q5_0   acc = fmaf(d_w * dx, (float) sum_k (q_k - bias) qx_k, acc)                  bias 0, 8, 16
//   Q4_1, Q5_1         acc = fmaf(d_w * dx, (float) sum_k q_k qx_k, fmaf(m_w, sx, acc))
// The integer sum is exact (|sum| <= 32 * 128 * 127 < 2^19); d_w * dx is one rounded product.  The slices are
// summed in slice order by prefill_epi_kernel, times 1 / s_t, unchanged.  The order is fixed by the tiling (no
// atomics): the same inputs give the same bits on every run.
//
// Outer shape as the family's (mm_pick_ks, split-K partials [slice][t][r], the grouped XCD-major tile order, rows
// and tokens past the end clamped on the load and masked on the store): a workgroup owns 256 weight rows x 128
// tokens and one K slice; 512 threads = 8 waves as 2 (tokens) x 4 (rows), each wave 64 x 64 = 4 x 4 tiles.
//
// Inner design, this family's own:
//   * K step 64 = TWO blocks per barrier.  At 1 B per code a 64-deep image row is the 64 B that gemm_gq.h spends
//     on 32: the same swizzle (chunk c of row r at position c ^ ((r >> 2) & 3)), half the barriers per K.
//   * Weights: thread t owns row t >> 1 and block t & 1 of the step, loads raw one step ahead of the multiply and
//     decodes to int8 with the bias already subtracted, 1 B per code, 32 B per thread and step (two
//     ds_write_b128): nibbles by mask and shift, the 5-bit formats' qh bits by one multiply
//     ((x * 0x00204081) & 0x01010101), the bias per byte without borrows (((x | 0x80) - bias) ^ 0x80), Q8_0 as
//     stored.  d (and m) go as f32 into the stage's PLANAR scale tables [block][row].
//   * Tokens: int8 codes by global_load_lds_dwordx4, one wave-instruction per wave and step (64 B per token);
//     the two blocks' {dx, sx} of a token are one 16-byte chunk, so the token scale table is DMA'd too (waves 0
//     and 1, 64 tokens each).  Nothing on the activation side passes through registers.
//   * MFMA: v_mfma_i32_16x16x32_i8 with A = weight rows, B = tokens (lane l: row / token l & 15, k = 8 (l >> 4)
//     + 0 .. 7, one ds_read_b64 per operand, tile and block).  D lane l = token l & 15, rows 4 (l >> 4) + reg:
//     a lane owns ONE token and FOUR ADJACENT weight rows per tile (gemm_gq.h: one row, four tokens).  So the
//     token's {dx, sx} is one scalar pair per lane, the rows' d (and m) one ds_read_b128 from the planar table,
//     the products d_w * dx and the multiply-adds run on adjacent pairs (v_pk_mul_f32 / v_pk_fma_f32), and the
//     partials leave as 16-byte stores (rows % 4 == 0; scalar stores otherwise).
//   * Two stages of 30 KiB: codes 16 KiB + 8 KiB, token scales 2 KiB, d and m 2 KiB each.  Pipeline as
//     gemm_gq.h: token DMA and raw weight registers of step kt + 1 in flight under step kt's multiply.
//   * Budget (the compiler's report for gfx950 at -O3, per instantiation; LDS 61440 B = 2 stages of 30 KiB for all;
//     256-VGPR bound, one 8-wave workgroup per CU as far as registers go):
//         Q8_0  139 VGPRs, no AGPRs, scratch 0
//         Q4_0  135 VGPRs, no AGPRs, scratch 0
//         Q4_1  148 VGPRs, no AGPRs, scratch 0
//         Q5_0  139 VGPRs, no AGPRs, scratch 0
//         Q5_1  155 VGPRs, no AGPRs, scratch 0
//     prefill_quant_q8_kernel: 39 VGPRs, scratch 0, no LDS.  The multiply loop holds no vmcnt wait (the token DMA
//     of the next step stays in flight under it), 32 MFMAs, 128 v_cvt_f32_i32 and the packed f32 multiplies and
//     multiply-adds per step.
//   * Compared (whole prompts only, profiles/i8_prompt_time.txt: Mistral-7B shapes, 8 layers, median of 7, spreads
//     <= 2.8 %, quantiser launches included), 2048 tokens, this route / gemm_gq.h / neither option, ms: Q8_0 16.9 /
//     20.9 / 27.8, Q4_0 17.5 / 20.3 / 26.9, Q4_1 19.5 / 25.4 / 134.3, Q5_0 18.1 / 24.1 / 27.2, Q5_1 20.0 / 27.0 /
//     143.2; f16 weights on gemm16.h 14.2.  256 tokens: 0.81 - 0.85 of gemm_gq.h's time.  NOT compared: the 32x32x32
//     MFMA, a 128-VGPR build (two workgroups per CU), three stages or a 256-token tile in the LDS the 1-byte codes
//     free, a per-kernel profile.  What bounds it has not been measured; per 16 x 16 tile and block the VALU work
//     (4 conversions, 2 packed products, 2 - 4 packed multiply-adds) is of the order of the MFMA's own time.
// Any rows >= 1 and n >= 1.  The passes route only GEMMs over more than 64 tokens here (prefill.hip, pf_i8_route).
#pragma once

#include "gemm16.h"

namespace xalm {

constexpr int MI_BR = 256;       // weight rows per workgroup
constexpr int MI_BT = 128;       // tokens per workgroup
constexpr int MI_THREADS = 512;  // 8 waves
constexpr int MI_BK = 64;        // k per stage: two blocks
constexpr int MI_NS = 2;         // stages
constexpr int MI_RB = MI_BK;     // image row bytes (1 B per code)
constexpr int MI_X_OFF = MI_BR * MI_RB;              // token codes behind the weight codes (16 KiB)
constexpr int MI_XS_OFF = MI_X_OFF + MI_BT * MI_RB;  // token scales [token][block]{dx, sx} (8 KiB on)
constexpr int MI_WD_OFF = MI_XS_OFF + MI_BT * 16;    // d [block][row] f32
constexpr int MI_WM_OFF = MI_WD_OFF + 2 * MI_BR * 4; // m likewise
constexpr int MI_STAGE = MI_WM_OFF + 2 * MI_BR * 4;  // 30 KiB
constexpr int MI_LDS = MI_NS * MI_STAGE;
static_assert(MI_BT * MI_RB == 8 * 1024, "8 waves fill a token tile with one wave-instruction each");
static_assert(2 * MI_LDS <= 160 * 1024, "two workgroups per CU");

typedef int mi_i32x4 __attribute__((ext_vector_type(4)));
typedef float mi_f32x2 __attribute__((ext_vector_type(2)));

constexpr bool mi_dt(const int dt) { return dt == XH_Q8_0 || dt == XH_Q4_0 || dt == XH_Q4_1 || dt == XH_Q5_0 || dt == XH_Q5_1; }
// bytes of one quantised token row: the codes, then {dx, sx} per block
__host__ __device__ constexpr size_t mi_xpitch(const size_t K) { return K + K / 4; }

struct MiArgs {
    const uint8_t* w;    // planar device rows (common.h)
    const int8_t* xq;    // [n] rows of mi_xpitch(K): codes, then {dx, sx} per block
    float* out;          // [ks][n][rows]
    size_t pitch;        // gq_pitch(dt, K)
    int rows, K, n, ks;  // K % (ks * 64) == 0 (host-checked)
    int n_rt, n_tt;      // tiles: ceil(rows / MI_BR), ceil(n / MI_BT)
};

inline int mi_pick_ks(const int rows, const int K, const int n, const size_t max_floats, const int n_cu) {
    return mm_pick_ks(rows, K, n, max_floats, n_cu, MI_BT);
}

__device__ __forceinline__ uint32_t mi_off(const int r, const int c) { return (uint32_t)(r * MI_RB + 16 * (c ^ ((r >> 2) & 3))); }

// four code bytes (each < 32) minus BIAS as four int8: no borrow leaves a byte (128 + x - BIAS >= 112)
template <int BIAS>
__device__ __forceinline__ uint32_t mi_codes4(const uint32_t m) {
    if constexpr (BIAS == 0) return m;
    else return ((m | 0x80808080u) - BIAS * 0x01010101u) ^ 0x80808080u;
}

// xh, xl [n][K] f16 bits -> q [n] rows of mi_xpitch(K).  One lane per 16 elements, two lanes per block.
__global__ __launch_bounds__(256) void prefill_quant_q8_kernel(const uint16_t* __restrict__ xh, const uint16_t* __restrict__ xl,
                                                                int8_t* __restrict__ q, const int K, const int n) {
    const size_t per_row = (size_t)K / 16;  // even: both lanes of a block leave together
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= (size_t)n * per_row) return;
    const size_t t = g / per_row, c = g - t * per_row;
    const size_t src = t * (size_t)K + 16 * c;
    const u32x4 h0 = *(const u32x4*)(xh + src), h1 = *(const u32x4*)(xh + src + 8);
    const u32x4 l0 = *(const u32x4*)(xl + src), l1 = *(const u32x4*)(xl + src + 8);
    const uint32_t hw[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
    const uint32_t lw[8] = {l0.x, l0.y, l0.z, l0.w, l1.x, l1.y, l1.z, l1.w};
    float v[16];
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        v[2 * i] = (float)__builtin_bit_cast(_Float16, (uint16_t)(hw[i] & 0xffffu)) +
                   (float)__builtin_bit_cast(_Float16, (uint16_t)(lw[i] & 0xffffu));
        v[2 * i + 1] = (float)__builtin_bit_cast(_Float16, (uint16_t)(hw[i] >> 16)) +
                       (float)__builtin_bit_cast(_Float16, (uint16_t)(lw[i] >> 16));
        amax = fmaxf(amax, fmaxf(fabsf(v[2 * i]), fabsf(v[2 * i + 1])));
    }
    amax = fmaxf(amax, __shfl_xor(amax, 1));
    const float inv = amax > 0.f ? 127.0f / amax : 0.f;
    uint32_t cw[4] = {0u, 0u, 0u, 0u};
    int sum = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const int qi = max(-127, min(127, (int)rintf(v[k] * inv)));
        sum += qi;
        cw[k >> 2] |= (uint32_t)(qi & 0xff) << (8 * (k & 3));
    }
    sum += __shfl_xor(sum, 1);
    int8_t* row = q + t * mi_xpitch((size_t)K);
    *(u32x4*)(row + 16 * c) = u32x4{cw[0], cw[1], cw[2], cw[3]};
    if (!(c & 1)) {
        const float dx = amax / 127.0f;
        *(mi_f32x2*)(row + K + (c >> 1) * 8) = mi_f32x2{dx, dx * (float)sum};
    }
}

template <int DT>
__global__ __launch_bounds__(MI_THREADS, 2) void mm_i8_kernel(const MiArgs a) {
    static_assert(mi_dt(DT), "the 32-element gguf blocks");
    constexpr bool AFF = gq_has_m(DT), QH = gq_has_qh(DT), Q8 = DT == XH_Q8_0;
    constexpr int BIAS = gq_bias(DT);
    constexpr int WL = (Q8 ? 2 : 1) + (QH ? 1 : 0) + 1 + (AFF ? 1 : 0);  // this thread's register loads per step
    extern __shared__ __attribute__((aligned(16))) char mi_smem[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    // bijective XCD-major order, then groups of 8 (row tile x slice) x n_tt token tiles, as gemm16.h
    const int nb = gridDim.x, b = blockIdx.x;
    const int q = nb >> 3, rem = nb & 7, xcd = b & 7;
    const int L = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + (b >> 3);
    constexpr int GR = 8;
    const int n_R = a.n_rt * a.ks, per_group = GR * a.n_tt;
    const int grp = L / per_group, in = L - grp * per_group;
    const int gr = min(n_R - grp * GR, GR);
    const int R = grp * GR + in % gr, tt = in / gr;
    const int s = R % a.ks, rt = R / a.ks;
    const int row0 = rt * MI_BR, t0 = tt * MI_BT;
    const int kslice = a.K / a.ks, kbeg = s * kslice, nk = kslice / MI_BK;
    const size_t K = (size_t)a.K, xp = mi_xpitch(K);

    // token DMA sources.  Codes: image row 16 wv + lane / 4, chunk position lane % 4 holding source chunk
    // (lane % 4) ^ f(row).  Scales (waves 0, 1): token 64 wv + lane, the step's two {dx, sx}.  Tokens past the
    // end clamped.
    const int8_t *xsrc, *ssrc;
    {
        const int r = wv * 16 + (lane >> 2);
        const int c = (lane & 3) ^ ((r >> 2) & 3);
        xsrc = a.xq + (size_t)min(t0 + r, a.n - 1) * xp + kbeg + 16 * c;
        ssrc = a.xq + (size_t)min(t0 + (wv & 1) * 64 + lane, a.n - 1) * xp + K + (size_t)(kbeg / 32) * 8;
    }
    auto issue_x = [&](const int stage, const int kt) {
        char* base = mi_smem + stage * MI_STAGE;
        __builtin_amdgcn_global_load_lds((const void*)(xsrc + kt * MI_BK), (mm_lds_ptr)(base + MI_X_OFF + wv * 1024), 16, 0, 0);
        if (wv < 2)
            __builtin_amdgcn_global_load_lds((const void*)(ssrc + kt * 16), (mm_lds_ptr)(base + MI_XS_OFF + wv * 1024), 16, 0, 0);
    };

    // weight decode: row wrow of the tile (past the end clamped), block wb of the step
    const int wrow = threadIdx.x >> 1, wb = threadIdx.x & 1;
    const char* wbase = (const char*)a.w + (size_t)min(row0 + wrow, a.rows - 1) * a.pitch;
    const int blk0 = kbeg / 32 + wb;  // step kt: block blk0 + 2 kt
    const char* wq = wbase + (size_t)blk0 * (Q8 ? 32 : 16);
    const char* wqh = wbase + gq_qbytes(DT, K) + (size_t)blk0 * 4;
    const char* wd = wbase + gq_d_off(DT, K) + (size_t)blk0 * 2;
    const char* wm = wbase + gq_m_off(DT, K) + (size_t)blk0 * 2;
    // raw loads only (WL of them), a step ahead: the unpacking waits for them in store_w, after the multiply
    u32x4 wr0, wr1;
    uint32_t wqw = 0u;
    uint16_t wd16, wm16 = 0;
    auto load_w = [&](const int kt) {
        if constexpr (QH) wqw = *(const uint32_t*)(wqh + (size_t)kt * 8);
        wd16 = *(const uint16_t*)(wd + (size_t)kt * 4);
        if constexpr (AFF) wm16 = *(const uint16_t*)(wm + (size_t)kt * 4);
        wr0 = *(const u32x4*)(wq + (size_t)kt * (Q8 ? 64 : 32));
        if constexpr (Q8) wr1 = *(const u32x4*)(wq + (size_t)kt * 64 + 16);
    };
    const uint32_t wst = mi_off(wrow, 2 * wb);
    auto store_w = [&](const int stage) {
        char* base = mi_smem + stage * MI_STAGE;
        u32x4 lo, hi;  // elements 0 .. 15 and 16 .. 31 of the block
        if constexpr (Q8) {
            lo = wr0;
            hi = wr1;
        } else {
            const uint32_t w4[4] = {wr0.x, wr0.y, wr0.z, wr0.w};
            uint32_t c[8];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                uint32_t ml = w4[i] & 0x0f0f0f0fu, mh = (w4[i] >> 4) & 0x0f0f0f0fu;
                if constexpr (QH) {
                    ml |= ((((wqw >> (4 * i)) & 15u) * 0x00204081u) & 0x01010101u) << 4;
                    mh |= ((((wqw >> (16 + 4 * i)) & 15u) * 0x00204081u) & 0x01010101u) << 4;
                }
                c[i] = mi_codes4<BIAS>(ml);
                c[4 + i] = mi_codes4<BIAS>(mh);
            }
            lo = u32x4{c[0], c[1], c[2], c[3]};
            hi = u32x4{c[4], c[5], c[6], c[7]};
        }
        *(u32x4*)(base + wst) = lo;
        *(u32x4*)(base + (wst ^ 16u)) = hi;  // chunk 2 wb + 1: position ^ 1
        *(float*)(base + MI_WD_OFF + 4 * (wb * MI_BR + wrow)) = (float)__builtin_bit_cast(_Float16, wd16);
        if constexpr (AFF) *(float*)(base + MI_WM_OFF + 4 * (wb * MI_BR + wrow)) = (float)__builtin_bit_cast(_Float16, wm16);
    };

    const int wt = wv >> 2, wr = wv & 3;  // this wave's 64 tokens / 64 rows of the tile
    const int lr = lane & 15, lc = lane >> 4;
    // image offsets of tile 0, block 0: the lane's 8 bytes are half lc & 1 of chunk lc >> 1; tile j / i lies
    // 16 rows = 1 KiB on (16 rows leave the swizzle alone), block 1 two chunks on (position ^ 2)
    const uint32_t wo = mi_off(64 * wr + lr, lc >> 1) + 8 * (lc & 1);
    const uint32_t xo = MI_X_OFF + mi_off(64 * wt + lr, lc >> 1) + 8 * (lc & 1);
    mm_f32x4 acc[4][4];  // [token tile][row tile], the lane's four rows
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = mm_f32x4{};
    auto compute = [&](const int stage) {
        const char* img = mi_smem + stage * MI_STAGE;
#pragma unroll
        for (int blk = 0; blk < 2; blk++) {
            long aw[4];
            mm_f32x4 dw[4];
            [[maybe_unused]] mm_f32x4 mw[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                aw[j] = *(const long*)(img + ((wo + j * 16 * MI_RB) ^ (32u * blk)));
                const int ro = 4 * (blk * MI_BR + 64 * wr + 16 * j + 4 * lc);
                dw[j] = *(const mm_f32x4*)(img + MI_WD_OFF + ro);
                if constexpr (AFF) mw[j] = *(const mm_f32x4*)(img + MI_WM_OFF + ro);
            }
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const long bx = *(const long*)(img + ((xo + i * 16 * MI_RB) ^ (32u * blk)));
                const mi_f32x2 sc = *(const mi_f32x2*)(img + MI_XS_OFF + 16 * (64 * wt + 16 * i + lr) + 8 * blk);
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const mi_i32x4 qs = __builtin_amdgcn_mfma_i32_16x16x32_i8(aw[j], bx, mi_i32x4{}, 0, 0, 0);
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        const float p = dw[j][e] * sc.x;
                        if constexpr (AFF) acc[i][j][e] = fmaf(p, (float)qs[e], fmaf(mw[j][e], sc.y, acc[i][j][e]));
                        else acc[i][j][e] = fmaf(p, (float)qs[e], acc[i][j][e]);
                    }
                }
                // pin the tile row's multiply-adds here, as gemm_gq.h: sunk behind the next decode they keep
                // every block sum live
                asm volatile("" : "+v"(acc[i][0]), "+v"(acc[i][1]), "+v"(acc[i][2]), "+v"(acc[i][3]));
            }
        }
    };

    // two stages, as gemm_gq.h.  VMEM order per thread: ... W(kt + 1), X(kt + 1), W(kt + 2) ...
    issue_x(0, 0);
    load_w(0);
    store_w(0);
    asm volatile("" ::: "memory");
    if (nk > 1) load_w(1);
    asm volatile("" ::: "memory");
    for (int kt = 0; kt < nk; kt++) {
        // X(kt) landed; W(kt + 1)'s loads, issued after it, may stay in flight
        if (kt + 1 < nk) mm_wait_vm<WL>();
        else mm_wait_vm<0>();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // own ds_writes of W(kt) / ds_reads of step kt - 1 retired
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (kt + 1 < nk) issue_x((kt + 1) & 1, kt + 1);
        compute(kt & 1);
        asm volatile("" ::: "memory");
        if (kt + 1 < nk) store_w((kt + 1) & 1);
        asm volatile("" ::: "memory");
        if (kt + 2 < nk) load_w(kt + 2);
        asm volatile("" ::: "memory");
    }

    float* out = a.out + (size_t)s * a.n * a.rows;
    const bool vec = (a.rows & 3) == 0;  // then every row quad is whole and 16-byte aligned
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int t = t0 + 64 * wt + 16 * i + lr;
        if (t >= a.n) continue;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int r = row0 + 64 * wr + 16 * j + 4 * lc;
            float* o = out + (size_t)t * a.rows + r;
            if (vec) {
                if (r < a.rows) *(mm_f32x4*)o = acc[i][j];
            } else {
#pragma unroll
                for (int e = 0; e < 4; e++)
                    if (r + e < a.rows) o[e] = acc[i][j][e];
            }
        }
    }
}

}  // namespace xalm
