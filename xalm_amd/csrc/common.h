// common.h — device-side element decode and wave/block reductions for gfx950.
//
// Decode semantics are the reference's (jubruckne/Xalm src/types.h), bit for bit:
//   f16   : IEEE binary16 -> f32 (ARM float16_t promotion)
//   bf16  : bits << 16                                   (bf16_to_f32, src/types.h:322-325)
//   e4m3  : ((b&0x80)<<24 | (b&0x7f)<<20) * 2^120        (f8_t::to_float, src/types.h:302-314)
//   e5m2  : ((b&0x80)<<24 | (b&0x7f)<<21) * 2^112        (same, M=2)
//   q8    : (1.f/100.f) * (float)int8                    (Type::Q8, src/types.h:423-424)
// The fp8 bit forms equal OCP e4m3fn / e5m2 for every finite code and give the reference's
// finite values for the NaN/Inf codes (e4m3 0x7F -> 480), which the hardware converter would
// not: matrices use the converter unless they hold such a code (WDec<*_EXACT>).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/xalm_hip.h"

namespace xalm {

typedef _Float16 h2_t __attribute__((ext_vector_type(2)));
typedef float f2_t __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));  // native vector: nontemporal loads

__device__ __forceinline__ float bits_f32(uint32_t u) { return __builtin_bit_cast(float, u); }

// 16 bytes of weights -> E floats.  E = 16 / sizeof(element).
template <int DT> struct WDec;

template <> struct WDec<XH_F32> {
    static constexpr int E = 4;
    __device__ __forceinline__ static void dec(const u32x4 v, float* f) {
        f[0] = bits_f32(v.x); f[1] = bits_f32(v.y); f[2] = bits_f32(v.z); f[3] = bits_f32(v.w);
    }
};

template <> struct WDec<XH_F16> {
    static constexpr int E = 8;
    __device__ __forceinline__ static void dec(const u32x4 v, float* f) {
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const f2_t p = __builtin_convertvector(__builtin_bit_cast(h2_t, w[i]), f2_t);
            f[2 * i] = p.x;
            f[2 * i + 1] = p.y;
        }
    }
};

template <> struct WDec<XH_BF16> {
    static constexpr int E = 8;
    __device__ __forceinline__ static void dec(const u32x4 v, float* f) {
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            f[2 * i] = bits_f32(w[i] << 16);
            f[2 * i + 1] = bits_f32(w[i] & 0xffff0000u);
        }
    }
};

template <int SHIFT, int SCALE_EXP>
__device__ __forceinline__ void dec_f8_word(const uint32_t w, float* f) {
    // byte k of w -> sign to bit 31, low 7 bits to the top of the f32 exponent field
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t b = (w >> (8 * k)) & 0xffu;
        const uint32_t u = ((b & 0x80u) << 24) | ((b & 0x7fu) << SHIFT);
        f[k] = bits_f32(u) * __builtin_bit_cast(float, (uint32_t)((127 + SCALE_EXP) << 23));
    }
}

// fp8 with the gfx950 converter (v_cvt_pk_f32_fp8 / _bf8: OCP e4m3fn / e5m2, 2 elements per
// instruction).  Equal to the reference's bit form for every code except the NaN/Inf codes
// (e4m3 0x7F/0xFF; e5m2 exponent 31), which the host detects at upload: a matrix holding
// any of them is decoded with the *_EXACT forms below instead.
template <bool BF8>
__device__ __forceinline__ void dec_f8_hw(const u32x4 v, float* f) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const f2_t lo = BF8 ? __builtin_amdgcn_cvt_pk_f32_bf8(w[i], false) : __builtin_amdgcn_cvt_pk_f32_fp8(w[i], false);
        const f2_t hi = BF8 ? __builtin_amdgcn_cvt_pk_f32_bf8(w[i], true) : __builtin_amdgcn_cvt_pk_f32_fp8(w[i], true);
        f[4 * i + 0] = lo.x;
        f[4 * i + 1] = lo.y;
        f[4 * i + 2] = hi.x;
        f[4 * i + 3] = hi.y;
    }
}
template <> struct WDec<XH_F8_E4M3> {
    static constexpr int E = 16;
    __device__ __forceinline__ static void dec(const u32x4 v, float* f) { dec_f8_hw<false>(v, f); }
};
template <> struct WDec<XH_F8_E5M2> {
    static constexpr int E = 16;
    __device__ __forceinline__ static void dec(const u32x4 v, float* f) { dec_f8_hw<true>(v, f); }
};

// internal kernel dtypes: fp8 matrices that hold NaN/Inf codes, decoded bit-exactly as the
// reference (f8_t::to_float, src/types.h:302-314: finite values for every code)
constexpr int XH_F8_E4M3_EXACT = 106;
constexpr int XH_F8_E5M2_EXACT = 107;
template <> struct WDec<XH_F8_E4M3_EXACT> {
    static constexpr int E = 16;
    __device__ __forceinline__ static void dec(const u32x4 v, float* f) {
        dec_f8_word<20, 120>(v.x, f);
        dec_f8_word<20, 120>(v.y, f + 4);
        dec_f8_word<20, 120>(v.z, f + 8);
        dec_f8_word<20, 120>(v.w, f + 12);
    }
};
template <> struct WDec<XH_F8_E5M2_EXACT> {
    static constexpr int E = 16;
    __device__ __forceinline__ static void dec(const u32x4 v, float* f) {
        dec_f8_word<21, 112>(v.x, f);
        dec_f8_word<21, 112>(v.y, f + 4);
        dec_f8_word<21, 112>(v.z, f + 8);
        dec_f8_word<21, 112>(v.w, f + 12);
    }
};
// the code's NaN/Inf pattern under OCP (where the hardware converter and the reference differ)
__host__ __device__ inline bool f8_special(const uint8_t b, const bool e5m2) {
    return e5m2 ? (b & 0x7Cu) == 0x7Cu : (b & 0x7Fu) == 0x7Fu;
}

template <> struct WDec<XH_Q8> {
    static constexpr int E = 16;
    __device__ __forceinline__ static void dec(const u32x4 v, float* f) {
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int8_t q = (int8_t)((w[i] >> (8 * k)) & 0xffu);
                f[4 * i + k] = (1.f / 100.f) * (float)q;
            }
    }
};

// ---- gguf blocks (XH_Q8_0, XH_Q4_0; quants.py Q8_0 :438-454, Q4_0 :281-311) --------------
// Device rows are planar: [quant bytes][f16 scale per 32 elements], pitch a multiple of 16 B,
// so a 16-B load is 16 int8 (Q8_0, half a block) or 32 nibbles (Q4_0, one block) and the
// scales of a wave's chunks are one coalesced read.  WDec decodes the codes (q, q - 8); the
// matvec multiplies each chunk's partial dot product by its block's d.
//
// The affine and 5-bit blocks (XH_Q4_1 / XH_Q5_0 / XH_Q5_1; quants.py :316-438) keep the planar
// idea, two properties deciding the planes of a row:
//   [nibbles: n/2 B][qh: 4 B per block, gq_has_qh][d: 2 B per block][m: 2 B per block, gq_has_m]
// so a 16-B load is still one whole block of nibbles, and qh, d and m of a wave's chunks are
// coalesced reads.  A weight's value is fmaf(d, q, m) (one f32 rounding, m = 0 without the plane).
__host__ __device__ constexpr bool gq_has_qh(const int dt) { return dt == XH_Q5_0 || dt == XH_Q5_1; }  // fifth-bit plane
__host__ __device__ constexpr bool gq_has_m(const int dt) { return dt == XH_Q4_1 || dt == XH_Q5_1; }   // affine: d*q + m
// gguf K-quants (XH_Q4_K / XH_Q6_K): super-blocks of 256 elements, still streamed as 32-element
// chunks of Q4_0-ordered nibbles, so every launch shape of the nibble blocks serves.  Planar rows:
//   Q4_K [nibbles: n/2 B][16 B per super-block: f16 d, f16 dmin, s[12] as in the file]
//        a chunk's lane reads its super-block's 16 B in one load (the eight lanes of a super-block
//        the same address) and unpacks sub-block j = blk & 7 to {d*sc, -(dmin*mn)}: from there on
//        the Q4_1 form, fmaf(d_eff, q, m_eff).
//   Q6_K [nibbles: n/2 B][2-bit plane: 8 B per chunk][int8 sc: 2 B per chunk][f16 d per super-block]
//        the low nibbles of a chunk are one 16-element scale group and the high nibbles the next;
//        the 2-bit plane holds, per chunk, one u32 for each: element 4w + k of the group at bits
//        8k + 2w, so (u32 >> 2w) & 0x03030303 lines the high bits of word w's four codes up with
//        its bytes.  A weight is (d*sc) * (q - 32), exact.
__host__ __device__ constexpr bool gq_k(const int dt) { return dt == XH_Q4_K || dt == XH_Q6_K; }
// affine in the matvec: d_eff * sum(q x) + m_eff * sum(x) per chunk (gq_rows)
__host__ __device__ constexpr bool gq_affine(const int dt) { return gq_has_m(dt) || dt == XH_Q4_K; }
__host__ __device__ constexpr bool gq_ext(const int dt) { return gq_has_qh(dt) || gq_has_m(dt) || dt == XH_Q4_K; }
// OCP microscaling FP4 (XH_MXFP4): the planar row is [e2m1 nibbles: n/2 B][e: 1 B per block], the
// nibble order Q4_0's, the scale the E8M0 byte (2^(e - 127)) in place of an f16 d.  The hardware
// converter decodes the codes (WDec<XH_MXFP4>); the scale multiplies in f32.
__host__ __device__ constexpr bool gq_mx(const int dt) { return dt == XH_MXFP4; }
__host__ __device__ constexpr bool gq_dt(const int dt) { return dt == XH_Q8_0 || dt == XH_Q4_0 || gq_ext(dt) || gq_mx(dt) || gq_k(dt); }
// elements a row must hold whole multiples of
__host__ __device__ constexpr int gq_group(const int dt) { return gq_k(dt) ? 256 : 32; }
// the code the scale multiplies is q - gq_bias (Q8_0: the int8 itself)
__host__ __device__ constexpr int gq_bias(const int dt) { return dt == XH_Q4_0 ? 8 : dt == XH_Q5_0 ? 16 : 0; }
__host__ __device__ constexpr size_t gq_qbytes(const int dt, const size_t n) { return dt == XH_Q8_0 ? n : n / 2; }
// byte offsets of the planes behind the codes
__host__ __device__ constexpr size_t gq_d_off(const int dt, const size_t n) {
    return gq_qbytes(dt, n) + (gq_has_qh(dt) ? n / 8 : 0);
}
__host__ __device__ constexpr size_t gq_m_off(const int dt, const size_t n) { return gq_d_off(dt, n) + n / 16; }
// Q6_K: the planes behind the 2-bit plane (the int8 scales, then d per super-block)
__host__ __device__ constexpr size_t kq6_sc_off(const size_t n) { return n / 2 + n / 4; }
__host__ __device__ constexpr size_t kq6_d_off(const size_t n) { return n / 2 + n / 4 + n / 16; }
__host__ __device__ constexpr size_t gq_pitch(const int dt, const size_t n) {
    if (dt == XH_Q4_K) return n / 2 + n / 16;  // 144 B per super-block
    if (dt == XH_Q6_K) return (kq6_d_off(n) + n / 128 + 15) & ~(size_t)15;
    return (gq_d_off(dt, n) + (gq_mx(dt) ? n / 32 : gq_has_m(dt) ? n / 8 : n / 16) + 15) & ~(size_t)15;
}
// K-quants: one file super-block `in` into the planar row `out` (n columns) at super-block index sb:
// the one statement of the device layout, for the host repack and the synthetic fill kernel
__host__ __device__ inline void kq_repack_sb(const int dt, const uint8_t* in, uint8_t* out, const size_t n, const size_t sb) {
    uint8_t q[256];
    if (dt == XH_Q4_K) {
        for (int e = 0; e < 256; e++) q[e] = (in[16 + 32 * (e >> 6) + (e & 31)] >> (4 * ((e >> 5) & 1))) & 15u;
        for (int k = 0; k < 16; k++) out[n / 2 + 16 * sb + k] = in[k];  // d, dmin, s[12]
    } else {
        for (int e = 0; e < 256; e++) {
            const int h = e >> 7, k = (e >> 5) & 3, l = e & 31;
            q[e] = (uint8_t)(((in[64 * h + 32 * (k & 1) + l] >> (4 * (k >> 1))) & 15u) | (((in[128 + 32 * h + l] >> (2 * k)) & 3u) << 4));
        }
        for (int j = 0; j < 8; j++) {  // the chunk's two plane words: element 4w + k at bits 8k + 2w
            uint32_t pl[2] = {0u, 0u};
            for (int i = 0; i < 32; i++) pl[i >> 4] |= (uint32_t)(q[32 * j + i] >> 4) << (8 * (i & 3) + 2 * ((i >> 2) & 3));
            for (int k = 0; k < 8; k++) out[n / 2 + 8 * (8 * sb + j) + k] = (uint8_t)(pl[k >> 2] >> (8 * (k & 3)));
        }
        for (int k = 0; k < 16; k++) out[kq6_sc_off(n) + 16 * sb + k] = in[192 + k];
        out[kq6_d_off(n) + 2 * sb] = in[208];
        out[kq6_d_off(n) + 2 * sb + 1] = in[209];
    }
    for (int j = 0; j < 8; j++)
        for (int i = 0; i < 16; i++) out[128 * sb + 16 * j + i] = (uint8_t)((q[32 * j + i] & 15u) | ((q[32 * j + 16 + i] & 15u) << 4));
}
// bytes of one block in the file: d, m, qh, codes (MXFP4: e, codes)
__host__ __device__ constexpr size_t gq_block_bytes(const int dt) {
    if (gq_k(dt)) return dt == XH_Q4_K ? 144 : 210;  // per super-block (gq_group elements)
    return dt == XH_Q8_0 ? 34 : gq_mx(dt) ? 17 : 18 + (gq_has_qh(dt) ? 4 : 0) + (gq_has_m(dt) ? 2 : 0);
}
// bytes in front of a file block's codes (d, m, qh; MXFP4: e)
__host__ __device__ constexpr size_t gq_head_bytes(const int dt) {
    return gq_mx(dt) ? 1 : 2 + (gq_has_qh(dt) ? 4 : 0) + (gq_has_m(dt) ? 2 : 0);
}
// MXFP4: 2^(e - 127) as an f32, exact for every e < 255 (e = 0: the subnormal 2^-127), and the
// e-range whose weights (0.5 .. 6 times the scale) are all normal f16
constexpr int MX_E_F16_LO = 114, MX_E_F16_HI = 140;
__host__ __device__ inline float mx_scale(const uint32_t e) {
    const uint32_t u = e ? e << 23 : 0x00400000u;
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_bit_cast(float, u);
#else
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
#endif
}
// every block dtype carries one scale set per 32 elements (BLOCK: elements per scale, 0: none)
template <int DT> struct WScale { static constexpr int BLOCK = gq_dt(DT) ? 32 : 0; };
// What the matvec holds per chunk beside the codes: the block's d, and for the affine / 5-bit
// blocks m and qh too (a field the dtype lacks is never read and costs no register)
struct GqScX { float d, m; uint32_t qh; };
// Q6_K: d*sc of the chunk's two 16-element groups and their high-bit words
struct GqSc6 { float d0, d1; uint32_t qa, qb; };
template <int DT, bool X = gq_ext(DT)> struct GqSc { typedef float T; };
template <int DT> struct GqSc<DT, true> { typedef GqScX T; };
template <> struct GqSc<XH_Q6_K, false> { typedef GqSc6 T; };
// ... read from a row's planes (tail: the row's first byte behind the codes, qbytes: the codes'
// bytes, n / 2 for the nibble types, so a row has qbytes / 16 blocks)
template <int DT>
__device__ __forceinline__ typename GqSc<DT>::T gq_ld_sc(const char* tail, const size_t qbytes, const int blk) {
    if constexpr (DT == XH_Q4_K) {
        // the super-block's {d, dmin, s[12]}: word 1 = s[0..3], 2 = s[4..7], 3 = s[8..11]
        const u32x4 t = *(const u32x4*)(tail + (size_t)(blk >> 3) * 16);
        const int j = blk & 7, sh = 8 * (j & 3);
        const uint32_t a = t.y >> sh, b = t.z >> sh, c = t.w >> sh;
        const uint32_t sc = j < 4 ? a & 63u : (c & 15u) | ((a >> 2) & 0x30u);
        const uint32_t mn = j < 4 ? b & 63u : ((c >> 4) & 15u) | ((b >> 2) & 0x30u);
        GqScX s;
        s.d = (float)__builtin_bit_cast(_Float16, (uint16_t)(t.x & 0xffffu)) * (float)sc;
        s.m = -((float)__builtin_bit_cast(_Float16, (uint16_t)(t.x >> 16)) * (float)mn);
        s.qh = 0u;
        return s;
    } else if constexpr (DT == XH_Q6_K) {
        const size_t nb = qbytes / 16;
        const uint2 q = *(const uint2*)(tail + (size_t)blk * 8);
        const uint32_t s2 = *(const uint16_t*)(tail + 8 * nb + (size_t)blk * 2);
        const float d = (float)__builtin_bit_cast(_Float16, *(const uint16_t*)(tail + 10 * nb + (size_t)(blk >> 3) * 2));
        GqSc6 s;
        s.d0 = d * (float)(int8_t)(s2 & 0xffu);
        s.d1 = d * (float)(int8_t)(s2 >> 8);
        s.qa = q.x;
        s.qb = q.y;
        return s;
    } else if constexpr (gq_ext(DT)) {
        const size_t nb = qbytes / 16;
        const char* dp = tail + (gq_has_qh(DT) ? 4 * nb : 0);
        GqScX s;
        s.d = (float)__builtin_bit_cast(_Float16, *(const uint16_t*)(dp + blk * 2));
        s.m = gq_has_m(DT) ? (float)__builtin_bit_cast(_Float16, *(const uint16_t*)(dp + 2 * nb + blk * 2)) : 0.f;
        s.qh = gq_has_qh(DT) ? *(const uint32_t*)(tail + blk * 4) : 0u;
        return s;
    } else if constexpr (gq_mx(DT)) {
        return mx_scale(*(const uint8_t*)(tail + blk));
    } else {
        return (float)__builtin_bit_cast(_Float16, *(const uint16_t*)(tail + blk * 2));
    }
}

template <> struct WDec<XH_Q8_0> {
    static constexpr int E = 16;
    __device__ __forceinline__ static void dec(const u32x4 v, float* f) {
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int k = 0; k < 4; k++) f[4 * i + k] = (float)(int8_t)((w[i] >> (8 * k)) & 0xffu);
    }
};
template <> struct WDec<XH_Q4_0> {
    static constexpr int E = 32;
    __device__ __forceinline__ static void dec(const u32x4 v, float* f) {
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t b = (w[i] >> (8 * k)) & 0xffu;
                f[4 * i + k] = (float)((int)(b & 15u) - 8);        // element j = 4i + k
                f[16 + 4 * i + k] = (float)((int)(b >> 4) - 8);    // element j + 16
            }
    }
};

// MXFP4: the 32 e2m1 values of a block by v_cvt_scalef32_pk_f32_fp4 (one byte, two codes, per
// instruction: the low nibble is element j, the high one j + 16), under the neutral scale 1.0;
// the block's own scale multiplies afterwards (gq_vals, gq_rows), which also covers e = 0
template <> struct WDec<XH_MXFP4> {
    static constexpr int E = 32;
    __device__ __forceinline__ static void dec(const u32x4 v, float* f) {
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const f2_t p0 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w[i], 1.0f, 0);
            const f2_t p1 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w[i], 1.0f, 1);
            const f2_t p2 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w[i], 1.0f, 2);
            const f2_t p3 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w[i], 1.0f, 3);
            f[4 * i + 0] = p0.x; f[16 + 4 * i + 0] = p0.y;
            f[4 * i + 1] = p1.x; f[16 + 4 * i + 1] = p1.y;
            f[4 * i + 2] = p2.x; f[16 + 4 * i + 2] = p2.y;
            f[4 * i + 3] = p3.x; f[16 + 4 * i + 3] = p3.y;
        }
    }
};

// The affine / 5-bit blocks' 16 B of nibbles: dec gives the plain nibbles (0..15; the fifth
// bits live in the qh plane), gq_vals the 32 weights of the block, fmaf(d, q - bias, m) with
// q = nibble | bit j of qh << 4 (quants.py dequantize_blocks; d*(q - bias) is exact).
template <int DT> struct WDecNib {
    static constexpr int E = 32;
    __device__ __forceinline__ static void dec(const u32x4 v, float* f) {
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t b = (w[i] >> (8 * k)) & 0xffu;
                f[4 * i + k] = (float)(b & 15u);
                f[16 + 4 * i + k] = (float)(b >> 4);
            }
    }
};
template <> struct WDec<XH_Q4_1> : WDecNib<XH_Q4_1> {};
template <> struct WDec<XH_Q5_0> : WDecNib<XH_Q5_0> {};
template <> struct WDec<XH_Q5_1> : WDecNib<XH_Q5_1> {};
template <> struct WDec<XH_Q4_K> : WDecNib<XH_Q4_K> {};
template <> struct WDec<XH_Q6_K> : WDecNib<XH_Q6_K> {};
// the two high bits of element e (0..31) of a Q6_K chunk (GqSc6's plane words)
__device__ __forceinline__ uint32_t kq6_hi(const uint32_t qa, const uint32_t qb, const int e) {
    return (((e & 16) ? qb : qa) >> (8 * (e & 3) + 2 * ((e >> 2) & 3))) & 3u;
}
// the weights of one chunk of a block dtype from its codes and scale set (sc: GqSc<DT>::T)
template <int DT, class SC>
__device__ __forceinline__ void gq_vals(const u32x4 v, const SC& sc, float* f) {
    WDec<DT>::dec(v, f);
    if constexpr (DT == XH_Q6_K) {
#pragma unroll
        for (int e = 0; e < 32; e++)
            f[e] = (e < 16 ? sc.d0 : sc.d1) * (f[e] + (float)(int)(kq6_hi(sc.qa, sc.qb, e) * 16u) - 32.f);  // exact
    } else if constexpr (gq_ext(DT)) {
#pragma unroll
        for (int e = 0; e < 32; e++) {
            const float q = f[e] + (float)(int)((gq_has_qh(DT) ? ((sc.qh >> e) & 1u) * 16u : 0u)) - (float)gq_bias(DT);
            f[e] = fmaf(sc.d, q, sc.m);
        }
    } else {
#pragma unroll
        for (int e = 0; e < WDec<DT>::E; e++) f[e] *= sc;
    }
}

// single-element decode (embedding gather, norm weights)
__device__ __forceinline__ float dec1(const int dtype, const void* p, const size_t i) {
    switch (dtype) {
        case XH_F32: return ((const float*)p)[i];
        case XH_F16: return (float)((const _Float16*)p)[i];
        case XH_BF16: return bits_f32((uint32_t)((const uint16_t*)p)[i] << 16);
        case XH_F8_E4M3: {
            const uint32_t b = ((const uint8_t*)p)[i];
            return bits_f32(((b & 0x80u) << 24) | ((b & 0x7fu) << 20)) * 0x1p120f;
        }
        case XH_F8_E5M2: {
            const uint32_t b = ((const uint8_t*)p)[i];
            return bits_f32(((b & 0x80u) << 24) | ((b & 0x7fu) << 21)) * 0x1p112f;
        }
        case XH_Q8: return (1.f / 100.f) * (float)((const int8_t*)p)[i];
        default: return __builtin_nanf("");
    }
}

// element i of row `row` of a [rows][n] matrix of `dtype` (gguf blocks: the planar device rows)
__device__ __forceinline__ float dec_row(const int dtype, const void* p, const size_t row, const int n, const int i) {
    if (!gq_dt(dtype)) return dec1(dtype, p, row * (size_t)n + i);
    const uint8_t* r = (const uint8_t*)p + row * gq_pitch(dtype, n);
    if (gq_mx(dtype)) {
        // the same converter and the same f32 product as the matvec's decode
        const uint32_t b = r[(i >> 5) * 16 + (i & 15)];
        const f2_t v = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(b, 1.0f, 0);
        return ((i & 16) ? v.y : v.x) * mx_scale(r[gq_d_off(dtype, n) + (i >> 5)]);
    }
    if (gq_k(dtype)) {
        // the chunk's scale set as the matvec reads it, then the one element
        const uint8_t b = r[(i >> 5) * 16 + (i & 15)];
        const float nib = (float)((i & 16) ? (b >> 4) : (b & 15u));
        const char* tail = (const char*)r + n / 2;
        if (dtype == XH_Q4_K) {
            const GqScX s = gq_ld_sc<XH_Q4_K>(tail, (size_t)n / 2, i >> 5);
            return fmaf(s.d, nib, s.m);
        }
        const GqSc6 s = gq_ld_sc<XH_Q6_K>(tail, (size_t)n / 2, i >> 5);
        return ((i & 16) ? s.d1 : s.d0) * (nib + (float)(int)(kq6_hi(s.qa, s.qb, i & 31) * 16u) - 32.f);
    }
    const float d = (float)__builtin_bit_cast(_Float16, *(const uint16_t*)(r + gq_d_off(dtype, n) + (i >> 5) * 2));
    if (dtype == XH_Q8_0) return d * (float)(int8_t)r[i];
    const uint8_t b = r[(i >> 5) * 16 + (i & 15)];
    if (dtype == XH_Q4_0) return d * (float)((int)((i & 16) ? (b >> 4) : (b & 15u)) - 8);
    // affine / 5-bit blocks: the planes behind the nibbles; exactly fmaf(d, q - bias, m)
    int q = (int)((i & 16) ? (b >> 4) : (b & 15u)) - gq_bias(dtype);
    if (gq_has_qh(dtype)) q += (int)((*(const uint32_t*)(r + gq_qbytes(dtype, n) + (i >> 5) * 4) >> (i & 31)) & 1u) << 4;
    const float m = gq_has_m(dtype) ? (float)__builtin_bit_cast(_Float16, *(const uint16_t*)(r + gq_m_off(dtype, n) + (i >> 5) * 2)) : 0.f;
    return fmaf(d, (float)q, m);
}

__device__ __forceinline__ uint16_t f32_to_f16_bits(const float f) {
    return __builtin_bit_cast(uint16_t, (_Float16)f);  // v_cvt_f16_f32, round-to-nearest-even
}
__device__ __forceinline__ float f16_bits_to_f32(const uint16_t h) {
    return (float)__builtin_bit_cast(_Float16, h);
}

// ---- the fp8 (e4m3) KV ring's element: what every K/V writer of an fp8 context stores ----
// The definition is xh_f8_e4m3_from_f32 (kv8.cpp, plain C++): clamp to [-448, 448] with f32
// min / max, then the nearest e4m3fn value, ties to the even mantissa, subnormals down to 2^-9,
// the sign kept.  On the device: the same clamp, then the gfx950 converter (v_cvt_pk_fp8_f32
// rounds to nearest even and keeps subnormals; without the clamp a magnitude past 448 would
// come out as the NaN code).  The pair (v0, v1) as two codes, v0's in the low byte.
__device__ __forceinline__ uint32_t kv8_pack(const float v0, const float v1) {
    const float c0 = fminf(fmaxf(v0, -448.f), 448.f), c1 = fminf(fmaxf(v1, -448.f), 448.f);
    return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(c0, c1, 0, false) & 0xffffu;
}
// the two codes of kv8_pack's result as their fp16 images (every e4m3 value is exact in fp16),
// the low code's in the low half
__device__ __forceinline__ uint32_t kv8_image_f16x2(const uint32_t codes) {
    const f2_t f = __builtin_amdgcn_cvt_pk_f32_fp8(codes, false);
    return (uint32_t)f32_to_f16_bits(f.x) | ((uint32_t)f32_to_f16_bits(f.y) << 16);
}

// ---- cross-lane reductions without LDS: DPP within 16-lane rows, permlane swaps across rows
// (v_permlane16/32_swap, gfx950; hipcc inserts the VALU->permlane wait states).  Every lane of
// the reduced group ends with the same value.
enum { DPP_XOR1 = 0xB1, DPP_XOR2 = 0x4E, DPP_ROW_ROR = 0x120, DPP_ROW_MIRROR = 0x140, DPP_ROW_HALF_MIRROR = 0x141 };
template <int CTRL>
__device__ __forceinline__ float dpp(const float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}
struct OpSum { __device__ static float f(float a, float b) { return a + b; } };
struct OpMax { __device__ static float f(float a, float b) { return fmaxf(a, b); } };
// combine the two rows of each row pair (1 with 0, 3 with 2) / the two half-waves
// The swaps are inline asm: hipcc (ROCm 7.2) takes the builtins' second result from the
// first operand's register (measured: permlane16_swap(x, y)[1] came back equal to [0]).  The
// s_nop 1 covers the "VALU write -> v_permlane read" hazard (cdna_hip_programming.md T21).
template <class Op>
__device__ __forceinline__ float rows_pair(const float v) {
    float a = v, b = v;
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
    return Op::f(a, b);
}
template <class Op>
__device__ __forceinline__ float halves(const float v) {
    float a = v, b = v;
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
    return Op::f(a, b);
}
// over aligned groups of G consecutive lanes (G = 2, 4, ..., 64)
template <int G, class Op = OpSum>
__device__ __forceinline__ float group_reduce(float v) {
    if (G >= 2) v = Op::f(v, dpp<DPP_XOR1>(v));
    if (G >= 4) v = Op::f(v, dpp<DPP_XOR2>(v));
    if (G >= 8) v = Op::f(v, dpp<DPP_ROW_HALF_MIRROR>(v));
    if (G >= 16) v = Op::f(v, dpp<DPP_ROW_MIRROR>(v));
    if (G >= 32) v = rows_pair<Op>(v);
    if (G >= 64) v = halves<Op>(v);
    return v;
}
// over the 64 / S lanes congruent mod S (S = 1, 2, 4, ..., 32): lanes l, l+S, l+2S, ...
template <int S, class Op = OpSum>
__device__ __forceinline__ float strided_reduce(float v) {
    if (S <= 1) v = Op::f(v, dpp<DPP_ROW_ROR + 1>(v));
    if (S <= 2) v = Op::f(v, dpp<DPP_ROW_ROR + 2>(v));
    if (S <= 4) v = Op::f(v, dpp<DPP_ROW_ROR + 4>(v));
    if (S <= 8) v = Op::f(v, dpp<DPP_ROW_ROR + 8>(v));
    if (S <= 16) v = rows_pair<Op>(v);
    v = halves<Op>(v);
    return v;
}
// Reduce-scatter of N per-lane values over the four 16-lane rows of a wave: on return v[0, N/4)
// of every lane of row r holds the 4-row sums of values [(r & 1) * N/2 + (r >> 1) * N/4, + N/4)
// (N/2 + N/4 swaps instead of 2 N for a full all-reduce of every value).
template <int N>
__device__ __forceinline__ void rows_reduce_scatter(float (&v)[N]) {
    static_assert(N % 4 == 0, "N must be a multiple of 4");
    // each swap carries its own s_nop 1: the operands may be fresh VALU copies (T21 hazard)
#pragma unroll
    for (int k = 0; k < N / 2; k++) {
        float x = v[k], y = v[N / 2 + k];
        asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(x), "+v"(y));
        v[k] = x + y;
    }
#pragma unroll
    for (int k = 0; k < N / 4; k++) {
        float x = v[k], y = v[N / 4 + k];
        asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(x), "+v"(y));
        v[k] = x + y;
    }
}

__device__ __forceinline__ float wave_sum(float v) { return group_reduce<64, OpSum>(v); }
__device__ __forceinline__ float wave_max(float v) { return group_reduce<64, OpMax>(v); }

// Orderable key of (logit, index) for Sampler::sample_argmax (src/sampler.cpp:19-30): a larger
// logit wins, then the smaller index (the first maximum); 0 = no candidate.
__device__ __forceinline__ unsigned long long argmax_key(const float v, const int idx) {
    uint32_t u = __builtin_bit_cast(uint32_t, v);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)u << 32) | (uint32_t)(~(uint32_t)idx);
}
__device__ __forceinline__ int argmax_key_index(const unsigned long long k) { return k ? (int)(~(uint32_t)k) : 0; }

// Per-token dynamic scalars, read by every kernel of a captured graph.
// kv_sink / kv_pos / kv_len follow src/infer.cpp:611-613.
struct StepParams {
    int token;
    int pos;
    int kv_sink;
    int kv_pos;
    int kv_len;
    int step;      // device decode loop: index into the token output buffer
    int pos_next;  // device decode loop: position of the next forward
    int max_seq_len;
};

__device__ __forceinline__ void step_positions(StepParams* sp, const int pos) {
    const int msl = sp->max_seq_len;
    const int kv_sink = pos >= msl ? 2 : 0;  // KV_SINKS, src/model.h:10
    sp->pos = pos;
    sp->kv_sink = kv_sink;
    sp->kv_pos = kv_sink + (pos - kv_sink) % (msl - kv_sink);
    sp->kv_len = pos >= msl ? msl : pos + 1;
}

// 16-byte sc1 load through a buffer descriptor (aux 16 = sc1, cdna_hip_programming.md T8 / G16)
__device__ __forceinline__ u32x4 ld_sc1_x4(const void* base, const uint32_t byte_off) {
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, 0x7fffffff, 0x00020000);
    return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)byte_off, 0, 16));
}

// silu / gelu exactly as src/infer.cpp:299-301
__device__ __forceinline__ float act_fn(const int act, const float x) {
    if (act == XH_ACT_SILU) return x / (1.0f + expf(-x));
    return 0.5f * x * (1.0f + tanhf(0.797885f * (x + 0.044715f * x * x * x)));
}

}  // namespace xalm
