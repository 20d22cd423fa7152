// gemm_kq.h — the prompt-pass GEMM for gguf K-quant weights (XH_OPT_PREFILL_KQ), beside gemm16.h and
// gemm_bf16.h.  It multiplies the CODES and applies the scales to the sums, as the decode matvec does
// (gemv.h, gq_rows), because neither format has an exact f16 image:
//
//   Q4_K  Y[t][r] = sum_j ( (d*sc_j) * sum_{k in j} q_k X[t][k]  -  (dmin*mn_j) * sum_{k in j} X[t][k] )
//   Q6_K  Y[t][r] = sum_g ( (d*sc_g) * sum_{k in g} (q_k - 32) X[t][k] )
//
// j: the 32-element sub-blocks, g: the 16-element scale groups, X = Xh + Xl the row-major f16 hi + lo
// halves of the activation rows under the power-of-two row scale s_t: gemm16.h's input, from the same
// layout-0 producers, and the epilogue kernel multiplies by 1 / s_t as for gemm16.h.
//   * A code (0 .. 15, or -32 .. 31) is exact in f16; code x half products are exact in the f32
//     accumulator of v_mfma_f32_16x16x32_f16; hi and lo accumulate into the SAME accumulator.
//   * d*sc and dmin*mn are exact in f32 (11 x 6 or 11 x 8 significant bits; gq_ld_sc, common.h).
//   * Every scale group starts from a zero C: one matrix instruction pair (hi, then lo) covers exactly
//     one group, then per element   acc = fmaf(d*sc, tmp, fmaf(-(dmin*mn), S, acc))   (Q4_K; S = the
//     sub-block's sum of the same hi + lo halves, from one more MFMA pair per token tile against an
//     all-ones B fragment, shared by the wave's four row tiles) or
//     acc = fmaf(d*sc_a, tmp_a, fmaf(d*sc_b, tmp_b, acc))   (Q6_K, the chunk's two groups).
//     Only these multiply-adds and the sums inside a group round.
//   * One-hot exactness: for an input row that is zero but for one power of two x, every other group
//     leaves acc unchanged, the min term (-(dmin*mn)) * x is exact, and the product term enters by the
//     one fused multiply-add: the result is x * fmaf(d*sc, q, -(dmin*mn)) (Q4_K) or x * (d*sc) (q - 32)
//     (Q6_K) bit for bit, the dequantised weight of dec_row (common.h).
//   * Summation order is fixed by the tiling (no atomics, no run-time algorithm choice): the same
//     inputs give the same bits on every run.
//
// Outer shape as gemm16.h / gemm_bf16.h (their K-slice pick, split-K partials [slice][t][r] and epilogue
// kernel serve this kernel unchanged): a workgroup owns 256 weight rows x 128 tokens and one K slice;
// 512 threads = 8 waves as 2 (tokens) x 4 (rows), each wave 64 tokens x 64 rows = 4 x 4 tiles of
// 16 x 16; the grouped XCD-major tile order.
//   * K step: 32 = one 16-byte chunk of the planar device rows' nibble plane (common.h, kq_repack_sb) =
//     one Q4_K sub-block = two Q6_K scale groups.  A K slice is whole super-blocks (K % (256 ks) == 0).
//   * Token tiles (hi, lo: 128 rows x 64 B each) go L2 -> LDS by global_load_lds_dwordx4 into the
//     swizzled image of gemm16.h's 32-deep steps (chunk c of row r at position c ^ ((r >> 2) & 3)), one
//     wave-instruction per tile, wave and step, under a counted `s_waitcnt vmcnt` and a raw s_barrier.
//   * Weight tile: decoded on the way in.  Thread t owns row t >> 1 and half h = t & 1 of the row's chunk:
//     it loads the chunk's 16 B (and for Q6_K its plane word, for both the scale fields: gq_ld_sc, the
//     decode matvec's reader) into registers one step ahead of the multiply, expands its 16 codes to f16
//     by the 0x6400 | n bit trick (1024 + n, then one packed subtract of 1024, or of 1056 for Q6_K's
//     q - 32) and writes them with two ds_write_b128 into the same swizzled image; it also writes its
//     half of the row's scale pair ({d*sc, -(dmin*mn)} or {d*sc_a, d*sc_b}) into the stage's table.
//     Raw weight traffic per K step is a quarter of an f16 tile's.
//   * MFMA: v_mfma_f32_16x16x32_f16, A = tokens (lane: token l & 15, k = 8 (l >> 4) + j), B = weight rows
//     (same lane map), D lane l = row l & 15 for tokens 4 (l >> 4) + reg: a lane owns ONE weight row per
//     row tile, so a scale is one per-lane scalar per tile (a ds_read_b64 from the table).  Q6_K runs its
//     two 16-element groups as two half-masked 32-deep MFMAs (lanes 0-31 hold k 0-15, lanes 32-63 k 16-31:
//     the token fragments of one group are zeroed in the other group's lanes by v_cndmask), which shares the
//     fragment reads with Q4_K; 16-deep MFMAs in their place have NOT been measured, nor has folding sc
//     into the Q4_K codes.
//     The scale pair is read by a ds_read_b64 in inline assembly: before a ds_read it can see, the
//     compiler waits for every token DMA in flight (it cannot tell the two stages apart), which would
//     serialise the next step's DMA with this step's multiply.
//   * Budget.  LDS: a stage is 16 KiB of weights + 2 x 8 KiB of tokens + 2 KiB of scales = 34 KiB; two
//     stages = 68 KiB, which would let two workgroups share a CU's 160 KiB.  The registers do not: the
//     compiler's report (gfx950, -O3) is 206 VGPRs for Q4_K and 256 for Q6_K, no AGPRs, scratch 0, so ONE
//     8-wave workgroup runs per CU (2 waves per SIMD).  Asked for 4 waves per SIMD (128 VGPRs) the same
//     code spills (308 / 536 B of scratch per lane) and was not taken: 64 accumulators, 16 + 8 fragment
//     registers, the scale pairs, the ones fragment and the raw weight registers of the next step do not
//     fit 128 without a smaller wave tile.  That is the kernel's open end, with a deeper ring in the
//     92 KiB of LDS one workgroup per CU leaves unused.
//   * Measured: whole prompts only (profiles/kq_prompt_time.txt: Mistral-7B shapes, 8 layers, 2048 tokens:
//     23.9 ms for Q4_K, 31.1 for Q6_K, 26.0 for the q4_k_m mix, against 113 - 125 ms on the f32-input
//     kernel and 27.1 ms for Q4_0 on gemm16.h).  Stage count, K step, tile, the ones-MFMA for S and the
//     half-masked Q6_K MFMAs are the design's starting point, NOT the winners of a comparison.
// Any rows >= 1 and n >= 1: rows / tokens past the end are clamped on the load (valid memory whose
// products are never stored) and masked on the store.  A GEMM over at most 64 tokens is not routed
// here (prefill.hip, pf_kq_route): most of a 128-token tile would be padding.
#pragma once

#include "gemm16.h"

namespace xalm {

constexpr int MK_BR = 256;       // weight rows per workgroup
constexpr int MK_BT = 128;       // tokens per workgroup
constexpr int MK_THREADS = 512;  // 8 waves
constexpr int MK_BK = 32;        // k per stage: one chunk
constexpr int MK_NS = 2;         // stages
constexpr int MK_RB = MK_BK * 2;                 // image row bytes
constexpr int MK_W_BYTES = MK_BR * MK_RB;        // 16 KiB
constexpr int MK_X_BYTES = MK_BT * MK_RB;        // 8 KiB, hi and lo each
constexpr int MK_SC_OFF = MK_W_BYTES + 2 * MK_X_BYTES;
constexpr int MK_STAGE = MK_SC_OFF + MK_BR * 8;  // + the scale pairs: 34 KiB
constexpr int MK_LDS = MK_NS * MK_STAGE;
constexpr int MK_KMULT = 256;    // K (and every K slice) in whole super-blocks
static_assert(MK_X_BYTES == 8 * 1024, "8 waves fill a token tile with one wave-instruction each");
static_assert(2 * MK_LDS <= 160 * 1024, "two workgroups per CU");

typedef _Float16 mk_f16x2 __attribute__((ext_vector_type(2)));

struct MkArgs {
    const uint8_t* w;    // planar device rows of Q4_K / Q6_K
    const uint16_t* xh;  // [n][K] f16 bits
    const uint16_t* xl;  // [n][K]
    float* out;          // [ks][n][rows]
    size_t pitch;        // gq_pitch(dt, K)
    int rows, K, n, ks;  // K % (ks * 256) == 0 (host-checked)
    int n_rt, n_tt;      // tiles: ceil(rows / MK_BR), ceil(n / MK_BT)
};

// the K slicing: gemm16.h's pick, halved until a slice is whole super-blocks (K % 256 == 0: 1 always is)
inline int mk_pick_ks(const int rows, const int K, const int n, const size_t max_floats, const int n_cu) {
    if (K % MK_KMULT) return 0;
    int ks = mm_pick_ks(rows, K, n, max_floats, n_cu, MK_BT);
    while (ks > 1 && K % (ks * MK_KMULT)) ks /= 2;
    return ks;
}

__device__ __forceinline__ uint32_t mk_off(const int r, const int c) { return (uint32_t)(r * MK_RB + 16 * (c ^ ((r >> 2) & 3))); }

// four code bytes (each < 64) as four f16 values code - BIAS: 0x6400 | n is 1024 + n
template <int BIAS>
__device__ __forceinline__ uint2 mk_codes4(const uint32_t m) {
    const uint32_t p0 = (m & 0xffu) | ((m & 0xff00u) << 8) | 0x64006400u;
    const uint32_t p1 = ((m >> 16) & 0xffu) | ((m >> 8) & 0xff0000u) | 0x64006400u;
    const mk_f16x2 off = {(_Float16)(1024 + BIAS), (_Float16)(1024 + BIAS)};
    const mk_f16x2 v0 = __builtin_bit_cast(mk_f16x2, p0) - off, v1 = __builtin_bit_cast(mk_f16x2, p1) - off;
    return uint2{__builtin_bit_cast(uint32_t, v0), __builtin_bit_cast(uint32_t, v1)};
}

template <int DT>
__global__ __launch_bounds__(MK_THREADS, 2) void mm_kq_kernel(const MkArgs a) {
    static_assert(DT == XH_Q4_K || DT == XH_Q6_K, "K-quants");
    constexpr bool Q6 = DT == XH_Q6_K;
    // this thread's register loads per step (gq_ld_sc and the chunk): the counted wait's lower bound
    constexpr int WL = Q6 ? 4 : 2;
    extern __shared__ __attribute__((aligned(16))) char mk_smem[];
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
        char* base = mk_smem + stage * MK_STAGE + MK_W_BYTES + wv * 1024;
        __builtin_amdgcn_global_load_lds((const void*)(hsrc + kt * MK_BK), (mm_lds_ptr)base, 16, 0, 0);
        __builtin_amdgcn_global_load_lds((const void*)(lsrc + kt * MK_BK), (mm_lds_ptr)(base + MK_X_BYTES), 16, 0, 0);
    };

    // weight decode: row wrow of the tile (past the end clamped), half wh of its chunk
    const int wrow = threadIdx.x >> 1, wh = threadIdx.x & 1;
    const char* wbase = (const char*)a.w + (size_t)min(row0 + wrow, a.rows - 1) * a.pitch;
    const char* wtail = wbase + K / 2;
    const int blk0 = kbeg / 32;
    // raw loads only (WL of them), a step ahead: the unpacking waits for them in store_w, after the multiply
    u32x4 wreg, whdr;         // the chunk; Q4_K: the super-block's {d, dmin, s[12]}
    uint32_t wpl;             // Q6_K: this half's plane word, its int8 scale and the super-block's d
    int8_t wsb;
    uint16_t wd16;
    auto load_w = [&](const int kt) {
        const int blk = blk0 + kt;
        if constexpr (Q6) {
            const size_t nb = K / 32;  // the planes behind the nibbles as gq_ld_sc reads them
            wpl = *(const uint32_t*)(wtail + (size_t)blk * 8 + 4 * wh);
            wsb = *(const int8_t*)(wtail + 8 * nb + (size_t)blk * 2 + wh);
            wd16 = *(const uint16_t*)(wtail + 10 * nb + (size_t)(blk >> 3) * 2);
        } else {
            whdr = *(const u32x4*)(wtail + (size_t)(blk >> 3) * 16);
        }
        wreg = *(const u32x4*)(wbase + (size_t)blk * 16);
    };
    auto store_w = [&](const int stage, const int kt) {
        char* base = mk_smem + stage * MK_STAGE;
        const uint32_t wd[4] = {wreg.x, wreg.y, wreg.z, wreg.w};
        uint2 c[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            uint32_t m = (wd[i] >> (4 * wh)) & 0x0f0f0f0fu;  // elements 16 wh + 4 i .. + 3
            if constexpr (Q6) {
                m |= ((wpl >> (2 * i)) & 0x03030303u) << 4;
                c[i] = mk_codes4<32>(m);
            } else {
                c[i] = mk_codes4<0>(m);
            }
        }
        *(u32x4*)(base + mk_off(wrow, 2 * wh)) = u32x4{c[0].x, c[0].y, c[1].x, c[1].y};
        *(u32x4*)(base + mk_off(wrow, 2 * wh + 1)) = u32x4{c[2].x, c[2].y, c[3].x, c[3].y};
        float sc;
        if constexpr (Q6) {
            sc = (float)__builtin_bit_cast(_Float16, wd16) * (float)wsb;
        } else {
            // gq_ld_sc<XH_Q4_K>'s unpacking of sub-block j: word 1 = s[0..3], 2 = s[4..7], 3 = s[8..11]
            const int j = (blk0 + kt) & 7, sh = 8 * (j & 3);
            const uint32_t sa = whdr.y >> sh, sb = whdr.z >> sh, sd = whdr.w >> sh;
            const uint32_t lo6 = (wh ? sb : sa) & 63u;
            const uint32_t hi6 = ((wh ? sd >> 4 : sd) & 15u) | (((wh ? sb : sa) >> 2) & 0x30u);
            const float f = (float)__builtin_bit_cast(_Float16, (uint16_t)(wh ? whdr.x >> 16 : whdr.x & 0xffffu));
            const float v = f * (float)(j < 4 ? lo6 : hi6);
            sc = wh ? -v : v;
        }
        *(float*)(base + MK_SC_OFF + 8 * wrow + 4 * wh) = sc;
    };

    const int wt = wv >> 2, wr = wv & 3;  // this wave's 64 tokens / 64 rows of the tile
    const int lr = lane & 15, lc = lane >> 4;
    mm_f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = mm_f32x4{};
    const _Float16 one = (_Float16)1.f;
    const mm_f16x8 ones = {one, one, one, one, one, one, one, one};
    auto compute = [&](const int stage) {
        const char* w_img = mk_smem + stage * MK_STAGE;
        const char* xh_img = w_img + MK_W_BYTES;
        const char* xl_img = xh_img + MK_X_BYTES;
        mm_f16x8 bw[4];
        unsigned long long scw[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int r = 64 * wr + 16 * j + lr;
            bw[j] = *(const mm_f16x8*)(w_img + mk_off(r, lc));
            // the scale pair by a ds_read the compiler does not see: before one it sees, it would wait
            // for the token DMA of the next step (it cannot tell the two stages apart)
            const uint32_t sa = (uint32_t)(uintptr_t)(mm_lds_ptr)(w_img + MK_SC_OFF + 8 * r);
            asm volatile("ds_read_b64 %0, %1" : "=v"(scw[j]) : "v"(sa));
        }
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(scw[0]), "+v"(scw[1]), "+v"(scw[2]), "+v"(scw[3]));
        float2 sc[4];
#pragma unroll
        for (int j = 0; j < 4; j++)
            sc[j] = float2{__uint_as_float((uint32_t)scw[j]), __uint_as_float((uint32_t)(scw[j] >> 32))};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t o = mk_off(64 * wt + 16 * i + lr, lc);
            const mm_f16x8 ah = *(const mm_f16x8*)(xh_img + o), al = *(const mm_f16x8*)(xl_img + o);
            if constexpr (Q6) {
                // lanes 0-31 hold k 0-15 (group a), lanes 32-63 k 16-31 (group b)
                const mm_f16x8 zero = {};
                const mm_f16x8 aha = lane < 32 ? ah : zero, ahb = lane < 32 ? zero : ah;
                const mm_f16x8 ala = lane < 32 ? al : zero, alb = lane < 32 ? zero : al;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    mm_f32x4 ta = __builtin_amdgcn_mfma_f32_16x16x32_f16(aha, bw[j], mm_f32x4{}, 0, 0, 0);
                    mm_f32x4 tb = __builtin_amdgcn_mfma_f32_16x16x32_f16(ahb, bw[j], mm_f32x4{}, 0, 0, 0);
                    ta = __builtin_amdgcn_mfma_f32_16x16x32_f16(ala, bw[j], ta, 0, 0, 0);
                    tb = __builtin_amdgcn_mfma_f32_16x16x32_f16(alb, bw[j], tb, 0, 0, 0);
#pragma unroll
                    for (int e = 0; e < 4; e++) acc[i][j][e] = fmaf(sc[j].x, ta[e], fmaf(sc[j].y, tb[e], acc[i][j][e]));
                }
            } else {
                mm_f32x4 sx = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, ones, mm_f32x4{}, 0, 0, 0);
                sx = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, ones, sx, 0, 0, 0);
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    mm_f32x4 tq = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bw[j], mm_f32x4{}, 0, 0, 0);
                    tq = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bw[j], tq, 0, 0, 0);
#pragma unroll
                    for (int e = 0; e < 4; e++) acc[i][j][e] = fmaf(sc[j].x, tq[e], fmaf(sc[j].y, sx[e], acc[i][j][e]));
                }
            }
        }
    };

    // two stages: the token DMA and the weight registers of step kt + 1 in flight under step kt's
    // multiply; the decoded weights of step kt + 1 written after it, into the stage every wave finished
    // reading before this step's barrier.  VMEM order per thread: ... W(kt + 1), X(kt + 1), W(kt + 2) ...
    issue_x(0, 0);
    load_w(0);
    store_w(0, 0);
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
        if (kt + 1 < nk) store_w((kt + 1) & 1, kt + 1);
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
