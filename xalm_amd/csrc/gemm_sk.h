// gemm_sk.h — the weight-streaming code GEMM for SHORT prompt passes (1 .. 64 tokens; XH_OPT_PREFILL_SHORT)
// over the gguf block formats Q8_0 / Q4_0 / Q4_1 / Q5_0 / Q5_1 and the K-quants Q4_K / Q6_K, beside gemm_gq.h
// and gemm_kq.h, whose 256 x 128 tiles start above 64 tokens.  At these lengths the matrix work is small and
// every weight byte is needed by exactly one wave, so the weights never touch LDS: HBM -> VGPR -> MFMA operand.
//
// Arithmetic: gemm_gq.h's and gemm_kq.h's, unchanged.  Codes (exact in f16) times the row-major f16 hi + lo
// activation halves under the row scale s_t, every scale group from a zero C (hi, then lo), then
//   Q8_0, Q4_0, Q5_0   acc = fmaf(d, sum (q - bias) x, acc)                       per 32-element block
//   Q4_1, Q5_1         acc = fmaf(d, sum q x, fmaf(m, sum x, acc))                per block
//   Q4_K               acc = fmaf(d*sc, sum q x, fmaf(-(dmin*mn), sum x, acc))    per 32-element sub-block
//   Q6_K               acc = fmaf(d*sc_a, sum_a (q - 32) x, fmaf(d*sc_b, sum_b (q - 32) x, acc))
//                                                                                 per chunk = two 16-element groups
// so their exactness argument holds: only these multiply-adds and the sums inside a group round, a one-hot
// power-of-two input returns x times dec_row's weight bit for bit, the order is fixed by the tiling (no atomics)
// and prefill_epi_kernel multiplies by 1 / s_t.  sum x comes from one more MFMA pair per token tile and block
// against an all-ones fragment, shared by the wave's row tiles.
//
// Work split: a wave owns SK_RT = 2 tiles of 16 weight rows times all TT token tiles (TT = ceil(n / 16), a
// template parameter: a 16-token pass does a quarter of a 64-token pass's matrix work); a workgroup is
// SK_WAVES = 4 such waves (SK_BR = 128 rows) over one K slice; grid = row tiles x slices, the slices of a row
// tile adjacent.  Partials [slice][t][r].  sk_pick_ks doubles the slices while the launch has fewer than
// SK_WG_PER_CU = 4 workgroups per CU (16 waves: the 128-VGPR bound), a slice keeps SK_MIN_SLICE = 256 columns
// (four steps, and whole super-blocks), there are at most SK_MAX_KS = 16 and the partials fit.
//
// Weight path, K step 64 = two blocks (two K-quant chunks) per row: lane l of a wave serves weight row l & 15 of
// each of its tiles and k group lc = l >> 4.  The MFMA (v_mfma_f32_16x16x32_f16, tokens as A, weight rows as B,
// so a D lane owns ONE weight row per tile and a scale is a per-lane scalar) lets the k order inside a block be
// permuted as long as both operands agree, so lane group lc takes
//   nibble formats   dword lc of the block's 16 B: elements 4 lc .. + 3 (low nibbles) and 16 + 4 lc .. + 3 (high)
//   Q8_0             bytes 8 lc .. + 7 of the block's 32: elements 8 lc .. + 7
// one global_load_dword (dwordx2) per block, loaded raw one step ahead and decoded in registers by the
// 0x6400 | n trick (mk_codes4); the fifth bits of lane group lc are bits 4 lc .. and 16 + 4 lc .. of the block's
// qh word, spread by one multiply; Q6_K's high bits are (plane word >> 2 lc) & 0x03030303 of the chunk's two
// plane words.  The scales come from registers too: the two blocks' d (and m) as one dword each, Q4_K's
// super-block header as one dwordx4, Q6_K's two plane words per chunk as one dwordx4, its four int8 scales as a
// dword and d as a ushort.  Q6_K's two groups per chunk are a lane's low and high nibbles, which is the operand
// layout of the 16-deep v_mfma_f32_16x16x16_f16 (k = 4 lc + j): two of those per chunk in place of gemm_kq.h's
// half-masked 32-deep ones, no masking.
//
// Token path: the hi and lo token tiles of a step (TT x 16 rows x 128 B each) are shared by the four waves:
// global_load_lds_dwordx4 (TT wave-instructions per wave and step) into a two-stage ring of the swizzled image
// of gemm16.h's 64-deep steps (chunk c of row r at position c ^ ((r >> 1) & 7)), tokens past n clamped, under a
// counted s_waitcnt vmcnt that leaves the next step's weight registers in flight, and a raw s_barrier.  A lane
// reads its fragment as two 8-byte pieces (the permutation above).  Rows and tokens past the end are masked on
// the store.
//
// Compiler report (gfx950, -O3, __launch_bounds__(256, 4); LDS 8 / 16 / 24 / 32 KiB for TT 1 / 2 / 3 / 4; scratch 0
// and no AGPRs for every one of the 28 instantiations), VGPRs for TT = 1 / 2 / 3 / 4:
//   Q8_0 72 / 80 / 90 / 100    Q4_0 66 / 76 / 84 / 94     Q4_1 82 / 86 / 98 / 108    Q5_0 75 / 87 / 97 / 107
//   Q5_1 86 / 105 / 115 / 124  Q4_K 79 / 89 / 108 / 118   Q6_K 98 / 107 / 119 / 124
// all under the 128-VGPR bound (four workgroups per CU).  Two things got them there from up to 128 VGPRs with
// 20 - 252 B of scratch: the multiply-adds are pinned behind each token tile's MFMAs (gemm_gq.h's empty asm), and
// the fragment pieces are read by ds_read_b64 in inline assembly (seen by the compiler, they made it drain the next
// step's DMA and weight loads with an s_waitcnt vmcnt(0) in front of the multiply).
// Measured (whole prompts only, profiles/sk_prompt_time.txt: Mistral-7B shapes, 8 layers, median of 7, spreads
// <= 2.7 % but one 2080-token outlier), option 1 against 0 in one run, ms.  32 tokens: Q8_0 1.88 / 4.97, Q4_0 1.81 /
// 5.07, Q5_0 2.05 / 5.06, Q4_1 2.09 / 2.46, Q5_1 2.40 / 2.79, Q4_K 1.89 / 2.46, Q6_K 2.33 / 2.67; f16 weights 1.90.
// 64 tokens: 2.00 - 2.70 against 3.65 - 5.25; f16 1.99.  8 tokens: 1.59 - 2.28 against 2.29 - 4.87; f16 1.80.  So the
// image formats drop to f16's time and the others gain 13 - 25 % at 32 tokens, but nothing comes near a small
// multiple of a decode step (about 0.38 ms): f16 weights on their own kernel take 1.80 ms for 8 tokens, a floor the
// pass shares that is not this GEMM's weight stream (about 25 launches a layer, the attention, the epilogues).
// NOT compared: SK_RT 1 or 4, 2 or 8 waves per workgroup, a deeper stage ring, weight registers more than one
// step ahead (one step leaves about rows x slices x 32 B of weights in flight, little for a 4096-row matrix),
// a 128- or 256-deep step, other slice bounds, half-masked 32-deep MFMAs for Q6_K, weights as the A operand,
// a per-kernel profile.  They are the design's starting point, not the winners of a search.
#pragma once

#include "gemm_kq.h"

namespace xalm {

constexpr int SK_RT = 2;                       // 16-row tiles per wave
constexpr int SK_WAVES = 4;                    // waves per workgroup
constexpr int SK_THREADS = 64 * SK_WAVES;
constexpr int SK_BR = 16 * SK_RT * SK_WAVES;   // weight rows per workgroup
constexpr int SK_BK = 64;                      // k per step: two blocks
constexpr int SK_NS = 2;                       // token stages
constexpr int SK_TOK = 64;                     // most tokens of a GEMM (PF_TOK)
constexpr int SK_MAX_KS = 16;                  // most K slices
constexpr int SK_MIN_SLICE = 256;              // least columns of a slice the picker leaves
constexpr int SK_WG_PER_CU = 4;                // workgroups per CU the picker asks for
constexpr int SK_RB = SK_BK * 2;               // image row bytes
__host__ __device__ constexpr int sk_stage_bytes(const int tt) { return 2 * tt * 16 * SK_RB; }  // hi + lo
__host__ __device__ constexpr int sk_lds(const int tt) { return SK_NS * sk_stage_bytes(tt); }

constexpr bool sk_dt(const int dt) {
    return dt == XH_Q8_0 || dt == XH_Q4_0 || dt == XH_Q4_1 || dt == XH_Q5_0 || dt == XH_Q5_1 || dt == XH_Q4_K || dt == XH_Q6_K;
}
// K, and every K slice, in whole multiples of this
constexpr int sk_kmult(const int dt) { return gq_k(dt) ? 256 : 64; }
// this thread's register loads per step and row tile: the counted wait's bound
constexpr int sk_loads(const int dt) {
    return dt == XH_Q6_K ? 5 : 3 + (gq_has_qh(dt) ? 1 : 0) + (gq_has_m(dt) ? 1 : 0);
}

// the K slicing: a power of two, slices of whole sk_kmult and at least SK_MIN_SLICE columns, doubled while the
// launch has fewer than SK_WG_PER_CU workgroups per CU and the partials fit; 0 if K does not fit the format
inline int sk_pick_ks(const int dt, const int rows, const int K, const int n, const size_t max_floats, const int n_cu) {
    const int km = sk_kmult(dt);
    if (K < km || K % km) return 0;
    const int n_rt = (rows + SK_BR - 1) / SK_BR;
    int ks = 1;
    while (2 * ks <= SK_MAX_KS && n_rt * ks < SK_WG_PER_CU * n_cu && K % (2 * ks * km) == 0 && K / (2 * ks) >= SK_MIN_SLICE &&
           (size_t)2 * ks * n * rows <= max_floats)
        ks *= 2;
    return ks;
}

typedef _Float16 sk_f16x4 __attribute__((ext_vector_type(4)));

// the raw registers of one row tile's step: which fields a format loads is sk_loads' count
struct SkRaw {
    uint2 qa, qb;   // the two blocks' codes of this lane group (.x alone for the nibble formats)
    uint2 qh;       // Q5_0 / Q5_1: the two blocks' qh words
    uint32_t d2;    // the two blocks' f16 d; Q6_K: the two chunks' four int8 scales
    uint32_t m2;    // Q4_1 / Q5_1: the two blocks' f16 m
    u32x4 hd;       // Q4_K: the super-block's {d, dmin, s[12]}; Q6_K: the two chunks' plane words
    uint16_t d16;   // Q6_K: the super-block's d
};

template <int DT, int TT>
__global__ __launch_bounds__(SK_THREADS, 4) void mm_sk_kernel(const MkArgs a) {
    static_assert(sk_dt(DT) && TT >= 1 && TT <= 4, "seven formats, 1 .. 4 token tiles");
    constexpr bool Q8 = DT == XH_Q8_0, K4 = DT == XH_Q4_K, K6 = DT == XH_Q6_K;
    constexpr bool AFF = gq_has_m(DT) || K4, QH = gq_has_qh(DT);
    constexpr int BIAS = Q8 ? 128 : K6 ? 32 : gq_bias(DT);  // Q8_0: of b ^ 0x80
    constexpr int WL = SK_RT * sk_loads(DT);
    constexpr int STAGE = sk_stage_bytes(TT), LO = TT * 16 * SK_RB;
    extern __shared__ __attribute__((aligned(16))) char sk_smem[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int lr = lane & 15, lc = lane >> 4;
    const int s = blockIdx.x % a.ks, rt = blockIdx.x / a.ks;
    const int row0 = rt * SK_BR + wv * 16 * SK_RT;
    const int kslice = a.K / a.ks, kbeg = s * kslice, nk = kslice / SK_BK;
    const size_t K = (size_t)a.K;

    // token DMA: wave-instruction q = wv TT + j fills image rows 8 q .. + 7 (rows [0, 16 TT) hi, then lo); lane:
    // row 8 q + lane / 8, chunk position lane % 8 holding source chunk (lane % 8) ^ f(row); tokens past n clamped
    const uint16_t* xsrc[TT];
#pragma unroll
    for (int j = 0; j < TT; j++) {
        const int R = 8 * (wv * TT + j) + (lane >> 3);
        const int lo = R >= 16 * TT, t = R - lo * 16 * TT;
        const int c = (lane & 7) ^ ((R >> 1) & 7);
        xsrc[j] = (lo ? a.xl : a.xh) + (size_t)min(t, a.n - 1) * K + kbeg + 8 * c;
    }
    auto issue_x = [&](const int stage, const int kt) {
        char* base = sk_smem + stage * STAGE + wv * TT * 1024;
#pragma unroll
        for (int j = 0; j < TT; j++)
            __builtin_amdgcn_global_load_lds((const void*)(xsrc[j] + kt * SK_BK), (mm_lds_ptr)(base + j * 1024), 16, 0, 0);
    };

    // weights: raw loads only (WL of them), one step ahead; decoded into the B fragments at the top of their step
    const char* wrow[SK_RT];
#pragma unroll
    for (int j = 0; j < SK_RT; j++) wrow[j] = (const char*)a.w + (size_t)min(row0 + 16 * j + lr, a.rows - 1) * a.pitch;
    const int blk0 = kbeg / 32;
    SkRaw raw[SK_RT];
    auto load_w = [&](const int kt) {
        const size_t blk = (size_t)(blk0 + 2 * kt);
#pragma unroll
        for (int j = 0; j < SK_RT; j++) {
            const char* r = wrow[j];
            if constexpr (Q8) {
                raw[j].qa = *(const uint2*)(r + blk * 32 + 8 * lc);
                raw[j].qb = *(const uint2*)(r + blk * 32 + 32 + 8 * lc);
            } else {
                raw[j].qa.x = *(const uint32_t*)(r + blk * 16 + 4 * lc);
                raw[j].qb.x = *(const uint32_t*)(r + blk * 16 + 16 + 4 * lc);
            }
            if constexpr (QH) raw[j].qh = *(const uint2*)(r + K / 2 + blk * 4);
            if constexpr (K4) {
                raw[j].hd = *(const u32x4*)(r + K / 2 + (blk >> 3) * 16);
            } else if constexpr (K6) {
                raw[j].hd = *(const u32x4*)(r + K / 2 + blk * 8);
                raw[j].d2 = *(const uint32_t*)(r + kq6_sc_off(K) + blk * 2);
                raw[j].d16 = *(const uint16_t*)(r + kq6_d_off(K) + (blk >> 3) * 2);
            } else {
                raw[j].d2 = *(const uint32_t*)(r + gq_d_off(DT, K) + blk * 2);
                if constexpr (gq_has_m(DT)) raw[j].m2 = *(const uint32_t*)(r + gq_m_off(DT, K) + blk * 2);
            }
        }
    };
    // the B fragments of a step: [block][row tile], elements in this lane group's order, and the scale pair
    // {d, m} (Q4_K: {d*sc, -(dmin*mn)}; Q6_K: {d*sc_a, d*sc_b}; the symmetric formats: d alone)
    uint2 bq[2][SK_RT][2];
    float sd[2][SK_RT];
    [[maybe_unused]] float sm[2][SK_RT];
    auto f16f = [](const uint32_t h) { return (float)__builtin_bit_cast(_Float16, (uint16_t)h); };
    auto decode = [&](const int kt) {
#pragma unroll
        for (int bl = 0; bl < 2; bl++)
#pragma unroll
            for (int j = 0; j < SK_RT; j++) {
                const SkRaw& w = raw[j];
                uint32_t lo4, hi4;
                if constexpr (Q8) {
                    const uint2 v = bl ? w.qb : w.qa;
                    lo4 = v.x ^ 0x80808080u;  // elements 8 lc .. + 3 as b + 128
                    hi4 = v.y ^ 0x80808080u;
                } else {
                    const uint32_t v = bl ? w.qb.x : w.qa.x;
                    lo4 = v & 0x0f0f0f0fu;         // elements 4 lc .. + 3
                    hi4 = (v >> 4) & 0x0f0f0f0fu;  // elements 16 + 4 lc .. + 3
                    if constexpr (QH) {
                        const uint32_t qh = bl ? w.qh.y : w.qh.x;
                        lo4 |= ((((qh >> (4 * lc)) & 15u) * 0x00204081u) & 0x01010101u) << 4;  // bit k into byte k
                        hi4 |= ((((qh >> (16 + 4 * lc)) & 15u) * 0x00204081u) & 0x01010101u) << 4;
                    }
                    if constexpr (K6) {
                        lo4 |= (((bl ? w.hd.z : w.hd.x) >> (2 * lc)) & 0x03030303u) << 4;
                        hi4 |= (((bl ? w.hd.w : w.hd.y) >> (2 * lc)) & 0x03030303u) << 4;
                    }
                }
                bq[bl][j][0] = mk_codes4<BIAS>(lo4);
                bq[bl][j][1] = mk_codes4<BIAS>(hi4);
                if constexpr (K4) {
                    // gq_ld_sc<XH_Q4_K>'s unpacking of sub-block jj (a slice starts on a super-block)
                    const int jj = (2 * kt + bl) & 7, sh = 8 * (jj & 3);
                    const uint32_t ua = w.hd.y >> sh, ub = w.hd.z >> sh, uc = w.hd.w >> sh;
                    const uint32_t sc = jj < 4 ? ua & 63u : (uc & 15u) | ((ua >> 2) & 0x30u);
                    const uint32_t mn = jj < 4 ? ub & 63u : ((uc >> 4) & 15u) | ((ub >> 2) & 0x30u);
                    sd[bl][j] = f16f(w.hd.x & 0xffffu) * (float)sc;
                    sm[bl][j] = -(f16f(w.hd.x >> 16) * (float)mn);
                } else if constexpr (K6) {
                    const uint32_t s2 = w.d2 >> (16 * bl);
                    const float d = f16f(w.d16);
                    sd[bl][j] = d * (float)(int8_t)(s2 & 0xffu);
                    sm[bl][j] = d * (float)(int8_t)((s2 >> 8) & 0xffu);
                } else {
                    sd[bl][j] = f16f(bl ? w.d2 >> 16 : w.d2 & 0xffffu);
                    if constexpr (gq_has_m(DT)) sm[bl][j] = f16f(bl ? w.m2 >> 16 : w.m2 & 0xffffu);
                }
            }
    };

    // token fragment pieces of this lane: image row lr of tile 0 (tile i lies 16 rows on, which leaves the
    // swizzle alone: an immediate offset), block bl, piece p
    uint32_t xo[2][2];
#pragma unroll
    for (int bl = 0; bl < 2; bl++)
#pragma unroll
        for (int p = 0; p < 2; p++) {
            const int c = Q8 ? 4 * bl + lc : 4 * bl + 2 * p + (lc >> 1);
            xo[bl][p] = (uint32_t)(lr * SK_RB + 16 * (c ^ ((lr >> 1) & 7)) + (Q8 ? 8 * p : 8 * (lc & 1)));
        }
    mm_f32x4 acc[TT][SK_RT];
#pragma unroll
    for (int i = 0; i < TT; i++)
#pragma unroll
        for (int j = 0; j < SK_RT; j++) acc[i][j] = mm_f32x4{};
    auto compute = [&](const int stage) {
        const uint32_t img = (uint32_t)(uintptr_t)(mm_lds_ptr)(sk_smem + stage * STAGE);
#pragma unroll
        for (int bl = 0; bl < 2; bl++)
#pragma unroll
            for (int i = 0; i < TT; i++) {
                // the fragment pieces by ds_reads the compiler does not see (gemm_kq.h's reason: before one it
                // sees, it waits for the next step's token DMA and weight registers, which it cannot tell from
                // this stage's), with their own wait
                unsigned long long f[4];
                const uint32_t a0 = img + xo[bl][0], a1 = img + xo[bl][1];
                asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(f[0]) : "v"(a0), "n"(i * 16 * SK_RB));
                asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(f[1]) : "v"(a1), "n"(i * 16 * SK_RB));
                asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(f[2]) : "v"(a0), "n"(i * 16 * SK_RB + LO));
                asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(f[3]) : "v"(a1), "n"(i * 16 * SK_RB + LO));
                asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]));
                const uint2 h0 = __builtin_bit_cast(uint2, f[0]), h1 = __builtin_bit_cast(uint2, f[1]);
                const uint2 l0 = __builtin_bit_cast(uint2, f[2]), l1 = __builtin_bit_cast(uint2, f[3]);
                if constexpr (K6) {
                    // group a: this lane's low nibbles against piece 0, group b: the high ones against piece 1
                    const sk_f16x4 ah = __builtin_bit_cast(sk_f16x4, h0), bh = __builtin_bit_cast(sk_f16x4, h1);
                    const sk_f16x4 al = __builtin_bit_cast(sk_f16x4, l0), bl4 = __builtin_bit_cast(sk_f16x4, l1);
#pragma unroll
                    for (int j = 0; j < SK_RT; j++) {
                        const sk_f16x4 wa = __builtin_bit_cast(sk_f16x4, bq[bl][j][0]), wb = __builtin_bit_cast(sk_f16x4, bq[bl][j][1]);
                        mm_f32x4 ta = __builtin_amdgcn_mfma_f32_16x16x16f16(ah, wa, mm_f32x4{}, 0, 0, 0);
                        mm_f32x4 tb = __builtin_amdgcn_mfma_f32_16x16x16f16(bh, wb, mm_f32x4{}, 0, 0, 0);
                        ta = __builtin_amdgcn_mfma_f32_16x16x16f16(al, wa, ta, 0, 0, 0);
                        tb = __builtin_amdgcn_mfma_f32_16x16x16f16(bl4, wb, tb, 0, 0, 0);
#pragma unroll
                        for (int e = 0; e < 4; e++) acc[i][j][e] = fmaf(sd[bl][j], ta[e], fmaf(sm[bl][j], tb[e], acc[i][j][e]));
                    }
                } else {
                    const mm_f16x8 ah = __builtin_bit_cast(mm_f16x8, u32x4{h0.x, h0.y, h1.x, h1.y});
                    const mm_f16x8 al = __builtin_bit_cast(mm_f16x8, u32x4{l0.x, l0.y, l1.x, l1.y});
                    [[maybe_unused]] mm_f32x4 sx;
                    if constexpr (AFF) {
                        const _Float16 one = (_Float16)1.f;
                        const mm_f16x8 ones = {one, one, one, one, one, one, one, one};
                        sx = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, ones, mm_f32x4{}, 0, 0, 0);
                        sx = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, ones, sx, 0, 0, 0);
                    }
#pragma unroll
                    for (int j = 0; j < SK_RT; j++) {
                        const mm_f16x8 bw = __builtin_bit_cast(mm_f16x8, u32x4{bq[bl][j][0].x, bq[bl][j][0].y, bq[bl][j][1].x, bq[bl][j][1].y});
                        mm_f32x4 tq = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bw, mm_f32x4{}, 0, 0, 0);
                        tq = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bw, tq, 0, 0, 0);
#pragma unroll
                        for (int e = 0; e < 4; e++) {
                            if constexpr (AFF) acc[i][j][e] = fmaf(sd[bl][j], tq[e], fmaf(sm[bl][j], sx[e], acc[i][j][e]));
                            else acc[i][j][e] = fmaf(sd[bl][j], tq[e], acc[i][j][e]);
                        }
                    }
                }
                // pin the token tile's multiply-adds here (gemm_gq.h's reason: sunk behind the next step's loads
                // they keep every block sum live)
                asm volatile("" : "+v"(acc[i][0]), "+v"(acc[i][1]));
            }
    };

    // two token stages.  VMEM order per thread: X(0) W(0) | W(1) X(1) | W(2) X(2) ...: at the top of step kt
    // the decode waits for W(kt), the raw registers take W(kt + 1), and the counted wait leaves those WL loads
    // in flight while X(kt), issued before them, has landed.  X(kt + 1) goes into the stage every wave finished
    // reading (step kt - 1) before this step's barrier.
    issue_x(0, 0);
    load_w(0);
    asm volatile("" ::: "memory");
    for (int kt = 0; kt < nk; kt++) {
        decode(kt);
        asm volatile("" ::: "memory");
        if (kt + 1 < nk) {
            load_w(kt + 1);
            asm volatile("" ::: "memory");
            mm_wait_vm<WL>();
        } else {
            mm_wait_vm<0>();
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // own ds_reads of step kt - 1 retired
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (kt + 1 < nk) issue_x((kt + 1) & 1, kt + 1);
        compute(kt & 1);
        asm volatile("" ::: "memory");
    }

    float* out = a.out + (size_t)s * a.n * a.rows;
#pragma unroll
    for (int j = 0; j < SK_RT; j++) {
        const int r = row0 + 16 * j + lr;
        if (r >= a.rows) continue;
#pragma unroll
        for (int i = 0; i < TT; i++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int t = 16 * i + 4 * lc + reg;
                if (t < a.n) out[(size_t)t * a.rows + r] = acc[i][j][reg];
            }
    }
}

}  // namespace xalm
