// gemm_gq.h — the prompt-pass GEMM for the 32-element gguf block weights Q8_0 / Q4_0 / Q4_1 / Q5_0 / Q5_1
// (XH_OPT_PREFILL_GQ), beside gemm16.h, gemm_bf16.h and gemm_kq.h.  Like gemm_kq.h it multiplies the CODES
// and applies the scales to the per-block sums, so no f16 image of the matrix is built (the hi + lo images of
// Q8_0 / Q4_0 / Q5_0 cost 4 B of traffic per weight per pass and two GEMMs; Q4_1 / Q5_1 have no exact f16
// pair at all and ran on the f32-input kernel in 64-token passes).  Per 32-element block b of weight row r,
// from a zero C:
//
//   Q8_0, Q4_0, Q5_0   acc = fmaf(d_b, sum_k (q_k - bias) X[t][k], acc)                    bias 0, 8, 16
//   Q4_1, Q5_1         acc = fmaf(d_b, sum_k q_k X[t][k], fmaf(m_b, sum_k X[t][k], acc))
//
// X = Xh + Xl: the row-major f16 hi + lo halves of the activation rows under the power-of-two row scale
// s_t, gemm16.h's input from the same layout-0 producers; the epilogue kernel multiplies by 1 / s_t.
//   * A code (-128 .. 127, -8 .. 7, -16 .. 15, 0 .. 15, 0 .. 31) is exact in f16; code x half products are
//     exact in the f32 accumulator of v_mfma_f32_16x16x32_f16; hi and lo accumulate into the SAME
//     accumulator.  A block is exactly one such instruction deep: one pair (hi, then lo) from a zero C gives
//     the block's sum.  The affine formats' sum of X is one more pair per token tile against an all-ones B
//     fragment, shared by the wave's four row tiles (as gemm_kq.h does for Q4_K).
//   * Only the multiply-adds above and the sums inside a block round.  The order is fixed by the tiling
//     (no atomics, no run-time algorithm choice): the same inputs give the same bits on every run.
//   * One-hot exactness: for an input row that is zero but for one power of two x, every other block
//     leaves acc unchanged, m_b * x is exact, and the code term enters by the one fused multiply-add: the
//     result is x * d (q - bias) (exact in f32) or x * fmaf(d, q, m) bit for bit, dec_row's weight (common.h).
//
// Outer shape as gemm16.h / gemm_kq.h (K-slice pick, split-K partials [slice][t][r], epilogue kernel
// unchanged): a workgroup owns 256 weight rows x 128 tokens and one K slice; 512 threads = 8 waves as
// 2 (tokens) x 4 (rows), each wave 64 x 64 = 4 x 4 tiles of 16 x 16; the grouped XCD-major tile order;
// token tiles by global_load_lds_dwordx4 into the swizzled 32-deep image under counted vmcnt waits; rows
// and tokens past the end clamped on the load and masked on the store.  The stage geometry, MkArgs and the
// helpers mk_off / mk_codes4 are gemm_kq.h's, by inclusion.
//
// Inner design, this family's own:
//   * K step 32 = one block per row per step; a K slice is a multiple of 64 (mm_pick_ks).
//   * Device rows are the planar ones of common.h: [codes][qh][d][m].  Thread t owns row t >> 1 and half
//     h = t & 1 (16 elements) of the row's block, loads raw one step ahead of the multiply and decodes on
//     the way into LDS:
//       nibble formats  the block's 16 B hold element j in byte j's low nibble, j + 16 in the high one, so
//                       half h takes all 16 bytes shifted by 4 h;
//       5-bit formats   also the block's qh word: bits 16 h + 4 i .. + 3 are spread into bit 4 of word i's
//                       four codes by one multiply ((x * 0x00204081) & 0x01010101: bit k lands in byte k);
//       Q8_0            its own 16 B of int8, as (b ^ 0x80) | 0x6400 (1024 + 128 + b) minus 1152;
//       the 4- and 5-bit codes by mk_codes4's 0x6400 | n and one packed subtract of 1024 + bias.
//     Two ds_write_b128 per thread and step, as gemm_kq.h.
//   * Scales: a per-stage LDS table read per lane (in the 16x16x32 D layout a lane owns ONE weight row per
//     row tile): {d, m}, 8 B per row, written by the row's two threads (h = 0: d, h = 1: m) for the affine
//     formats; d alone, 4 B per row, for the symmetric ones.  Every thread issues the same number of
//     register loads per step (the counted wait's bound): codes, qh where the format has it, and one
//     2-byte scale (h picks d or m; the symmetric formats' h = 1 loads d and drops it).
//     The table is read by a ds_read in inline assembly for gemm_kq.h's reason (a ds_read the compiler
//     sees makes it wait for the next step's token DMA).
//   * Budget (the compiler's report for gfx950 at -O3, per instantiation; LDS 69632 B = 2 stages of 34 KiB
//     for all, so the stage fits a CU's 160 KiB twice):
//         Q8_0  124 VGPRs, no AGPRs, scratch 0   (128-VGPR bound: 4 waves per SIMD, two workgroups per CU)
//         Q4_0  124 VGPRs, no AGPRs, scratch 0   (128-VGPR bound likewise)
//         Q5_0  140 VGPRs, no AGPRs, scratch 0   (256-VGPR bound; asked for 128 it spills 12 B per lane: not taken)
//         Q4_1  144 VGPRs, no AGPRs, scratch 0   (256-VGPR bound: 3 waves per SIMD fit, one 8-wave workgroup per CU)
//         Q5_1  151 VGPRs, no AGPRs, scratch 0   (256-VGPR bound)
//     Two things brought the symmetric formats from 182 - 190 VGPRs down: the multiply-adds are pinned inside
//     the multiply (an empty asm on the tile row's accumulators; the compiler otherwise sinks all 64 behind
//     the next step's decode and keeps every block sum live), and each operand has ONE image offset with the
//     other tiles as immediate ds_read offsets.  Q5_0 is 12 registers short (the qh word, its pointer and
//     the spread's temporaries); the affine formats carry the second scale, the ones fragment and sum(x).
//   * Compared (whole prompts only, profiles/gq_prompt_time.txt: Mistral-7B shapes, 8 layers, 2048 tokens,
//     median of 7, spreads <= 2.5 %): option 1 against 0 in one run: Q8_0 20.9 ms against 27.8, Q4_0 20.0 / 26.7,
//     Q5_0 23.7 / 27.1, Q4_1 25.4 / 134.1, Q5_1 26.9 / 142.9; f16 weights on gemm16.h 14.2.  The 128-VGPR build
//     of Q8_0 / Q4_0 against their 256-VGPR build (-DMG_WAVES_128=2; profiles/gq_prompt_time_256vgpr.txt): 20.86
//     against 20.87 and 20.03 against 20.01 ms, no difference: the second workgroup per CU buys nothing
//     measurable at these shapes, so the kernel is not latency-bound there.  The bound is kept (scratch 0).
//     NOT compared: stage count, K step, tile shapes, a smaller wave tile, folding the bias into the
//     ones-MFMA, 16-deep MFMAs, a per-kernel profile.  They are the design's starting point, not the
//     winners of a search.
// Any rows >= 1 and n >= 1.  A GEMM over at most 64 tokens is not routed here (prefill.hip, pf_gq_route).
#pragma once

#include <type_traits>

#include "gemm_kq.h"

namespace xalm {

constexpr bool mg_dt(const int dt) { return dt == XH_Q8_0 || dt == XH_Q4_0 || dt == XH_Q4_1 || dt == XH_Q5_0 || dt == XH_Q5_1; }
// waves per SIMD asked of the compiler: 4 (128 VGPRs, two workgroups per CU) where the report shows no scratch
#ifndef MG_WAVES_128
#define MG_WAVES_128 4  // 2: the 256-VGPR build of the same instantiations, for a comparison
#endif
constexpr int mg_waves(const int dt) { return dt == XH_Q8_0 || dt == XH_Q4_0 ? MG_WAVES_128 : 2; }

// the K slicing: gemm16.h's pick over this kernel's token tile (slices of whole 64s: two blocks)
inline int mg_pick_ks(const int rows, const int K, const int n, const size_t max_floats, const int n_cu) {
    return mm_pick_ks(rows, K, n, max_floats, n_cu, MK_BT);
}

template <int DT>
__global__ __launch_bounds__(MK_THREADS, mg_waves(DT)) void mm_gq_kernel(const MkArgs a) {
    static_assert(mg_dt(DT), "the 32-element gguf blocks");
    constexpr bool AFF = gq_has_m(DT), QH = gq_has_qh(DT), Q8 = DT == XH_Q8_0;
    constexpr int BIAS = Q8 ? 128 : gq_bias(DT);  // Q8_0: of b ^ 0x80
    constexpr int WL = QH ? 3 : 2;                // this thread's register loads per step
    constexpr int SCB = AFF ? 8 : 4;              // scale table bytes per row
    extern __shared__ __attribute__((aligned(16))) char mg_smem[];
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
    const int row0 = rt * MK_BR, t0 = tt * MK_BT;
    const int kslice = a.K / a.ks, kbeg = s * kslice, nk = kslice / MK_BK;
    const size_t K = (size_t)a.K;

    // token DMA sources: image row 16 wv + lane / 4, chunk position lane % 4 holding source chunk
    // (lane % 4) ^ f(row); tokens past the end clamped
    const uint16_t *hsrc, *lsrc;
    {
        const int r = wv * 16 + (lane >> 2);
        const int c = (lane & 3) ^ ((r >> 2) & 3);
        const size_t o = (size_t)min(t0 + r, a.n - 1) * K + kbeg + 8 * c;
        hsrc = a.xh + o;
        lsrc = a.xl + o;
    }
    auto issue_x = [&](const int stage, const int kt) {
        char* base = mg_smem + stage * MK_STAGE + MK_W_BYTES + wv * 1024;
        __builtin_amdgcn_global_load_lds((const void*)(hsrc + kt * MK_BK), (mm_lds_ptr)base, 16, 0, 0);
        __builtin_amdgcn_global_load_lds((const void*)(lsrc + kt * MK_BK), (mm_lds_ptr)(base + MK_X_BYTES), 16, 0, 0);
    };

    // weight decode: row wrow of the tile (past the end clamped), half wh of its block
    const int wrow = threadIdx.x >> 1, wh = threadIdx.x & 1;
    const char* wbase = (const char*)a.w + (size_t)min(row0 + wrow, a.rows - 1) * a.pitch;
    const int blk0 = kbeg / 32;
    const char* wq = wbase + (Q8 ? (size_t)blk0 * 32 + 16 * wh : (size_t)blk0 * 16);  // this thread's 16 B of block blk0
    const char* wqh = wbase + gq_qbytes(DT, K) + (size_t)blk0 * 4;
    const char* wsc = wbase + (AFF && wh ? gq_m_off(DT, K) : gq_d_off(DT, K)) + (size_t)blk0 * 2;
    // raw loads only (WL of them), a step ahead: the unpacking waits for them in store_w, after the multiply
    u32x4 wreg;
    uint32_t wqw = 0u;
    uint16_t ws16;
    auto load_w = [&](const int kt) {
        if constexpr (QH) wqw = *(const uint32_t*)(wqh + (size_t)kt * 4);
        ws16 = *(const uint16_t*)(wsc + (size_t)kt * 2);
        wreg = *(const u32x4*)(wq + (size_t)kt * (Q8 ? 32 : 16));
    };
    const uint32_t wst = mk_off(wrow, 2 * wh);
    auto store_w = [&](const int stage) {
        char* base = mg_smem + stage * MK_STAGE;
        const uint32_t wd[4] = {wreg.x, wreg.y, wreg.z, wreg.w};
        uint2 c[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            uint32_t m;
            if constexpr (Q8) {
                m = wd[i] ^ 0x80808080u;  // elements 16 wh + 4 i .. + 3 as b + 128
            } else {
                m = (wd[i] >> (4 * wh)) & 0x0f0f0f0fu;
                if constexpr (QH) m |= ((((wqw >> (16 * wh + 4 * i)) & 15u) * 0x00204081u) & 0x01010101u) << 4;
            }
            c[i] = mk_codes4<BIAS>(m);
        }
        *(u32x4*)(base + wst) = u32x4{c[0].x, c[0].y, c[1].x, c[1].y};
        *(u32x4*)(base + (wst ^ 16u)) = u32x4{c[2].x, c[2].y, c[3].x, c[3].y};  // chunk 2 wh + 1: position ^ 1
        const float sc = (float)__builtin_bit_cast(_Float16, ws16);
        if constexpr (AFF) *(float*)(base + MK_SC_OFF + 8 * wrow + 4 * wh) = sc;
        else if (wh == 0) *(float*)(base + MK_SC_OFF + 4 * wrow) = sc;
    };

    const int wt = wv >> 2, wr = wv & 3;  // this wave's 64 tokens / 64 rows of the tile
    const int lr = lane & 15, lc = lane >> 4;
    // image offsets of tile 0; tile j / i lies 16 rows = 16 MK_RB bytes on (16 rows leave the swizzle alone),
    // an immediate offset of the ds_read
    const uint32_t wo = mk_off(64 * wr + lr, lc), xo = mk_off(64 * wt + lr, lc);
    mm_f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = mm_f32x4{};
    auto compute = [&](const int stage) {
        const char* w_img = mg_smem + stage * MK_STAGE;
        const char* xh_img = w_img + MK_W_BYTES;
        const char* xl_img = xh_img + MK_X_BYTES;
        mm_f16x8 bw[4];
        typename std::conditional<AFF, unsigned long long, uint32_t>::type scw[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            bw[j] = *(const mm_f16x8*)(w_img + wo + j * 16 * MK_RB);
            // the scales by a ds_read the compiler does not see: before one it sees, it would wait for the
            // token DMA of the next step (it cannot tell the two stages apart)
            const uint32_t sa = (uint32_t)(uintptr_t)(mm_lds_ptr)(w_img + MK_SC_OFF + SCB * (64 * wr + lr + 16 * j));
            if constexpr (AFF) asm volatile("ds_read_b64 %0, %1" : "=v"(scw[j]) : "v"(sa));
            else asm volatile("ds_read_b32 %0, %1" : "=v"(scw[j]) : "v"(sa));
        }
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(scw[0]), "+v"(scw[1]), "+v"(scw[2]), "+v"(scw[3]));
        [[maybe_unused]] float sd[4], sm[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            sd[j] = __uint_as_float((uint32_t)scw[j]);
            if constexpr (AFF) sm[j] = __uint_as_float((uint32_t)(scw[j] >> 32));
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t o = xo + i * 16 * MK_RB;
            const mm_f16x8 ah = *(const mm_f16x8*)(xh_img + o), al = *(const mm_f16x8*)(xl_img + o);
            mm_f32x4 sx;
            if constexpr (AFF) {
                const _Float16 one = (_Float16)1.f;
                const mm_f16x8 ones = {one, one, one, one, one, one, one, one};
                sx = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, ones, mm_f32x4{}, 0, 0, 0);
                sx = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, ones, sx, 0, 0, 0);
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                mm_f32x4 tq = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bw[j], mm_f32x4{}, 0, 0, 0);
                tq = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bw[j], tq, 0, 0, 0);
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    if constexpr (AFF) acc[i][j][e] = fmaf(sd[j], tq[e], fmaf(sm[j], sx[e], acc[i][j][e]));
                    else acc[i][j][e] = fmaf(sd[j], tq[e], acc[i][j][e]);
                }
            }
            // pin the tile row's multiply-adds here: left alone, the compiler sinks all 64 of them behind the
            // decode of the next step, which keeps every block sum live (+ 64 VGPRs) and off the MFMAs' shadow
            asm volatile("" : "+v"(acc[i][0]), "+v"(acc[i][1]), "+v"(acc[i][2]), "+v"(acc[i][3]));
        }
    };

    // two stages, as gemm_kq.h: the token DMA and the weight registers of step kt + 1 in flight under step
    // kt's multiply; the decoded weights of step kt + 1 written after it, into the stage every wave finished
    // reading before this step's barrier.  VMEM order per thread: ... W(kt + 1), X(kt + 1), W(kt + 2) ...
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
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int r = row0 + 64 * wr + 16 * j + lr;
        if (r >= a.rows) continue;
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int t = t0 + 64 * wt + 16 * i + 4 * lc + reg;
                if (t < a.n) out[(size_t)t * a.rows + r] = acc[i][j][reg];
            }
    }
}

}  // namespace xalm
