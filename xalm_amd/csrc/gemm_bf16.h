// gemm_bf16.h — the prompt-pass GEMM for bf16 weights (XH_OPT_PREFILL_BF16), beside gemm16.h, and the
// producers of its input.
//
//   Y[t][r] = sum_k W[r][k] * (X0[t][k] + X1[t][k] + X2[t][k])
//
// W is a bf16 matrix as uploaded ([rows][K]): no image pass, no transient buffer, no range rule (a bf16
// weight has f32's exponent range, so a matrix with one weight below 2^-17 or above 65504 has no exact
// f16 image and cannot take gemm16.h).  X0 .. X2 are three bf16 pieces of the f32 activation, each
// rounded to nearest even, each residual exact in f32:
//   b0 = bf16(x), b1 = bf16(x - b0), b2 = bf16((x - b0) - b1),   b0 + b1 + b2 == x exactly
// (8 + 8 + 8 significant bits cover f32's 24; the third piece is never below 2^-24 |x|, so all pieces
// are normal bf16 for x = 0 or 2^-100 <= |x| < 2^127: the range this contract covers.  How the matrix
// core treats SUBNORMAL bf16 inputs has not been measured here: that case is outside the contract.
// Two pieces would leave 2^-17 relative, coarser than the f16 route's 2^-22.)  There is no row scale
// and no 1 / s in the epilogue: the partials are unscaled.  A bf16 x bf16 product has at most 16
// significant bits and is exact in the f32 accumulator; the three pieces accumulate into the SAME
// accumulator, per 32-deep k step in piece order.  The order is fixed by the tiling (no atomics, no
// run-time algorithm choice): the same inputs give the same bits on every run.
//
// Outer shape as gemm16.h (its pass code, split-K partials [slice][t][r] and epilogue kernel serve
// this kernel unchanged): a workgroup owns 256 weight rows x 128 tokens and one K slice; 512 threads =
// 8 waves as 2 (tokens) x 4 (rows), each wave 64 tokens x 64 rows.  What differs is the budget:
//   * LDS: a K step carries one weight tile and THREE token tiles, (256 + 3 x 128) rows.  At BK = 64
//     that is 80 KiB per stage and two stages are the whole 160 KiB: not viable.  At BK = 32 a stage is
//     40 KiB.  The compiler's report (gfx950, every instantiation: scratch 0, no AGPRs) is 108 / 109
//     VGPRs at 16 x 16 x 32 tiles with three / two stages and 103 at 32 x 32 x 16: below 128, so two
//     8-wave workgroups fit a CU's registers, and two stages (80 KiB) let both fit its LDS.  Measured
//     (tools/gemm_bf16_bench, profiles/gemm_bf16_bench.txt, 2048 tokens, Mistral-7B shapes): two
//     stages x two workgroups per CU beat three stages x one on the launches with more than one
//     workgroup per CU (qkv 270 vs 304 us, W1/W3 1035 vs 1194) and on Wo (187 vs 193); on W2 (one
//     workgroup per CU, 448 K steps) three stages win by 2 % (631 vs 644).  A layer: 2136 vs 2322
//     us.  The product instantiates two stages: a second workgroup hides a barrier better than a
//     deeper ring does.  16 x 16 x 32 tiles beat 32 x 32 x 16 at either depth (2136 vs 2326 us).
//   * L2 -> LDS by global_load_lds_dwordx4 (1 KiB = 16 image rows per wave-instruction; 5 per wave and
//     stage: 2 of W, 1 of each piece), counted `s_waitcnt vmcnt` + raw s_barrier as gemm16.h.
//   * LDS image: rows of 32 bf16 = 64 B = four 16-B chunks, chunk c of row r at position
//     c ^ ((r >> 2) & 3): a ds_read_b128 lane group (16 rows, one chunk) covers 16 distinct 16-B bank
//     slots (slot = 4 (r & 3) + position).  The DMA writes lane-linearly, so the permutation is
//     applied to the per-lane SOURCE address.
//   * MFMA: one weight fragment read from LDS feeds three MFMAs, one per piece: 16 ds_read_b128 per
//     48 MFMAs and wave (gemm16.h: 12 per 32), 1.5x gemm16.h's MFMA work per weight element.
//     MF = 16: v_mfma_f32_16x16x32_bf16, 4 x 4 tiles per wave, A = tokens (lane: token l & 15,
//     k = 8 (l >> 4) + j), B = weight rows (same lane map), D lane l = row l & 15 for tokens
//     4 (l >> 4) + reg.  MF = 32: v_mfma_f32_32x32x16_bf16, 2 x 2 tiles, two 16-deep steps per stage,
//     lane maps as gemm16.h's 32 x 32 path.  The product instantiates MF = 16 (measured, above).
//     The balance did move to the matrix cores: 1.1 - 1.4 PFLOP/s of MFMA work at 1.34 - 1.60 times
//     gemm16.h's time on the same shape (arithmetic alone says 1.5).  A GEMM over at most 64 tokens
//     is not routed here (prefill.hip, pf_bf16_route): most of a 128-token tile would be padding.
//   * workgroup -> tile: gemm16.h's grouped, XCD-major order.
//   * K slices: mm_pick_ks (gemm16.h): K in whole 64-deep multiples per slice, ks <= 8, the partials
//     bound; the epilogue sums the slices in slice order.
// Any rows >= 1 and n >= 1: rows / tokens past the end are clamped on the load (valid memory whose
// products are never stored) and masked on the store.
#pragma once

#include "gemm16.h"
#include "gemv.h"

namespace xalm {

constexpr int MB_BR = 256;       // weight rows per workgroup
constexpr int MB_BT = 128;       // tokens per workgroup
constexpr int MB_THREADS = 512;  // 8 waves
constexpr int MB_BK = 32;        // k per stage
constexpr int MB_NS = 2;         // stages of the product's instantiation (80 KiB: two workgroups per CU)
constexpr int MB_MF = 16;        // its MFMA tile
constexpr int MB_RB = MB_BK * 2;                        // image row bytes
constexpr int MB_STAGE = (MB_BR + 3 * MB_BT) * MB_RB;   // 40 KiB
constexpr int MB_WI = MB_BR * MB_RB / 1024 / 8;         // W DMA instructions per wave and stage (2)
constexpr int MB_XI = MB_BT * MB_RB / 1024 / 8;         // ... of each piece (1)
constexpr int MB_LPS = MB_WI + 3 * MB_XI;
static_assert(MB_XI == 1 && MB_WI == 2, "8 waves fill a stage with whole wave-instructions");
__host__ __device__ constexpr int mb_lds(const int ns) { return ns * MB_STAGE; }

typedef __bf16 mb_bf16x8 __attribute__((ext_vector_type(8)));

struct MbArgs {
    const uint16_t* w;   // [rows][K] bf16 bits
    const uint16_t* x;   // [3][n][K] bf16 bits: the pieces, plane after plane
    float* out;          // [ks][n][rows]
    int rows, K, n, ks;  // K % (ks * 64) == 0 (host-checked)
    int n_rt, n_tt;      // tiles: ceil(rows / MB_BR), ceil(n / MB_BT)
};

__device__ __forceinline__ uint32_t mb_off(const int r, const int c) { return (uint32_t)(r * MB_RB + 16 * (c ^ ((r >> 2) & 3))); }

template <int NS, int MF>
__global__ __launch_bounds__(MB_THREADS, 2) void mm_bf16_kernel_t(const MbArgs a) {
    static_assert(NS >= 2 && NS * MB_STAGE <= 160 * 1024, "stages");
    static_assert(MF == 16 || MF == 32, "MFMA tile");
    extern __shared__ __attribute__((aligned(16))) char mb_smem[];
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
    const int row0 = rt * MB_BR, t0 = tt * MB_BT;
    const int kslice = a.K / a.ks, kbeg = s * kslice, nk = kslice / MB_BK;
    const size_t K = (size_t)a.K, plane = (size_t)a.n * K;

    // this lane's DMA sources: image row r0 + lane / 4, chunk position lane % 4 holding source chunk
    // (lane % 4) ^ f(row); rows / tokens past the end clamped
    const uint16_t* wsrc[MB_WI];
#pragma unroll
    for (int i = 0; i < MB_WI; i++) {
        const int r = (wv * MB_WI + i) * 16 + (lane >> 2);
        const int c = (lane & 3) ^ ((r >> 2) & 3);
        wsrc[i] = a.w + (size_t)min(row0 + r, a.rows - 1) * K + kbeg + 8 * c;
    }
    const uint16_t* xsrc;
    {
        const int r = wv * 16 + (lane >> 2);
        const int c = (lane & 3) ^ ((r >> 2) & 3);
        xsrc = a.x + (size_t)min(t0 + r, a.n - 1) * K + kbeg + 8 * c;
    }
    auto issue = [&](const int stage, const int kt) {
        char* base = mb_smem + stage * MB_STAGE;
        const int k = kt * MB_BK;
#pragma unroll
        for (int i = 0; i < MB_WI; i++)
            __builtin_amdgcn_global_load_lds((const void*)(wsrc[i] + k), (mm_lds_ptr)(base + (wv * MB_WI + i) * 1024), 16,
                                             0, 0);
#pragma unroll
        for (int p = 0; p < 3; p++)
            __builtin_amdgcn_global_load_lds((const void*)(xsrc + p * plane + k),
                                             (mm_lds_ptr)(base + (MB_BR + p * MB_BT) * MB_RB + wv * 1024), 16, 0, 0);
    };

    const int wt = wv >> 2, wr = wv & 3;  // this wave's 64 tokens / 64 rows of the tile
    constexpr int NT = 64 / MF;           // MF-wide tiles per wave along either side
    constexpr int KQ = MF == 16 ? 1 : 2;  // MFMA k steps per stage (32- / 16-deep)
    const int lr = lane & (MF - 1), lc = lane / MF;  // fragment row and chunk within a k step
    typedef float acc_t __attribute__((ext_vector_type(MF == 16 ? 4 : 16)));
    acc_t acc[NT][NT];
#pragma unroll
    for (int i = 0; i < NT; i++)
#pragma unroll
        for (int j = 0; j < NT; j++) acc[i][j] = acc_t{};
    auto compute = [&](const int stage) {
        const char* w_img = mb_smem + stage * MB_STAGE;
        const char* x_img = w_img + MB_BR * MB_RB;
#pragma unroll
        for (int kq = 0; kq < KQ; kq++) {
            const int c = (4 / KQ) * kq + lc;
            mb_bf16x8 bw[NT], ax[3][NT];
#pragma unroll
            for (int j = 0; j < NT; j++) bw[j] = *(const mb_bf16x8*)(w_img + mb_off(64 * wr + MF * j + lr, c));
#pragma unroll
            for (int p = 0; p < 3; p++)
#pragma unroll
                for (int i = 0; i < NT; i++)
                    ax[p][i] = *(const mb_bf16x8*)(x_img + p * MB_BT * MB_RB + mb_off(64 * wt + MF * i + lr, c));
            // piece-outer: the three MFMAs into one accumulator are NT * NT instructions apart
#pragma unroll
            for (int p = 0; p < 3; p++)
#pragma unroll
                for (int i = 0; i < NT; i++)
#pragma unroll
                    for (int j = 0; j < NT; j++) {
                        if constexpr (MF == 16)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ax[p][i], bw[j], acc[i][j], 0, 0, 0);
                        else
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ax[p][i], bw[j], acc[i][j], 0, 0, 0);
                    }
        }
    };

    // ring of NS stages, NS - 1 steps of DMA ahead of the multiply
#pragma unroll
    for (int d = 0; d < NS - 1; d++)
        if (d < nk) issue(d, d);
    for (int kt = 0; kt < nk; kt++) {
        mm_wait_ahead<MB_LPS, NS>(min(NS - 2, nk - 1 - kt));  // this wave's DMA of step kt landed
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    // own ds_reads of the refilled stage retired
        __builtin_amdgcn_s_barrier();                          // ... every wave's; stage kt - 1 read
        asm volatile("" ::: "memory");
        if (kt + NS - 1 < nk) issue((kt + NS - 1) % NS, kt + NS - 1);
        compute(kt % NS);
    }

    float* out = a.out + (size_t)s * a.n * a.rows;
#pragma unroll
    for (int j = 0; j < NT; j++) {
        const int r = row0 + 64 * wr + MF * j + lr;
        if (r >= a.rows) continue;
#pragma unroll
        for (int i = 0; i < NT; i++)
#pragma unroll
            for (int reg = 0; reg < (MF == 16 ? 4 : 16); reg++) {
                // D: 16 x 16: tokens 4 (l >> 4) + reg; 32 x 32: (reg & 3) + 8 (reg >> 2) + 4 (l >> 5)
                const int tl = MF == 16 ? 4 * lc + reg : (reg & 3) + 8 * (reg >> 2) + 4 * lc;
                const int t = t0 + 64 * wt + MF * i + tl;
                if (t < a.n) out[(size_t)t * a.rows + r] = acc[i][j][reg];
            }
    }
}

#define mm_bf16_kernel mm_bf16_kernel_t<MB_NS, MB_MF>

// ---- the piece producers: one workgroup per token row, 16-byte stores ------------------------------
// round to nearest even on the bits (a NaN keeps its top bits and stays a NaN)
__device__ __forceinline__ uint32_t bf16_rne(const float f) {
    const uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
// 8 elements as three bf16 pieces at element offset o of each plane
__device__ __forceinline__ void bf16_split_store8(const float (&v)[8], const size_t o, const size_t plane, uint16_t* x3) {
    uint32_t pk[3][4] = {};
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint32_t b0 = bf16_rne(v[j]);
        const float r1 = v[j] - __uint_as_float(b0 << 16);
        const uint32_t b1 = bf16_rne(r1);
        const float r2 = r1 - __uint_as_float(b1 << 16);
        const uint32_t b2 = bf16_rne(r2);
        const int sh = 16 * (j & 1);
        pk[0][j >> 1] |= b0 << sh;
        pk[1][j >> 1] |= b1 << sh;
        pk[2][j >> 1] |= b2 << sh;
    }
#pragma unroll
    for (int p = 0; p < 3; p++) *(u32x4*)(x3 + p * plane + o) = u32x4{pk[p][0], pk[p][1], pk[p][2], pk[p][3]};
}

// the three row-major bf16 planes [3][n][K] of x [n][K] (K % 8 == 0)
__global__ __launch_bounds__(256) void prefill_split_bf16_kernel(const float* x, int K, int n, uint16_t* x3) {
    const int t = blockIdx.x;
    const float* xr = x + (size_t)t * K;
    for (int i = threadIdx.x; i < K / 8; i += 256) {
        const float4 a = *(const float4*)(xr + 8 * i), b = *(const float4*)(xr + 8 * i + 4);
        const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        bf16_split_store8(v, (size_t)t * K + 8 * i, (size_t)n * K, x3);
    }
}

// rmsnorm of each token row (as prefill_rmsnorm_kernel: x * scale * w, the same reduction) written
// straight into the planes: prefill_rmsnorm_split_kernel's structure without the max reduction
__global__ __launch_bounds__(256) void prefill_rmsnorm_split_bf16_kernel(const float* x, int dim, const void* w, int wdt,
                                                                         float eps, int n, uint16_t* x3) {
    __shared__ float red[4];
    const int t = blockIdx.x;
    const float* xr = x + (size_t)t * dim;
    const float scale = block_rms_scale<256>(xr, dim, eps, red);
    for (int i = threadIdx.x; i < dim / 8; i += 256) {
        const float4 a = ((const float4*)xr)[2 * i], b = ((const float4*)xr)[2 * i + 1];
        const float4 wa = load_norm4(w, wdt, 2 * i), wb = load_norm4(w, wdt, 2 * i + 1);
        const float v[8] = {a.x * scale * wa.x, a.y * scale * wa.y, a.z * scale * wa.z, a.w * scale * wa.w,
                            b.x * scale * wb.x, b.y * scale * wb.y, b.z * scale * wb.z, b.w * scale * wb.w};
        bf16_split_store8(v, (size_t)t * dim + 8 * i, (size_t)n * dim, x3);
    }
}

}  // namespace xalm
