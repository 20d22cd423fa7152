/*
 * xalm_synth.h — deterministic synthetic weights for benchmarks (no checkpoints offline).
 *
 * One definition, compiled by gcc (oracle / CPU baseline) and by hipcc (device fill kernel),
 * so a tensor generated on the GPU is bit-identical to the host copy the CPU baseline uses.
 * Value of element i: mean + std * sqrt(3) * (u0 + u1 + u2 + u3 - 2), u_k uniform [0,1) from
 * a splitmix64 hash of (seed, i, k) (Irwin-Hall, variance 1/3 -> scaled to 1): integer ops,
 * float adds and one explicit fmaf only, so no libm or contraction differences between
 * compilers.  Then rounded to the storage type with round-to-nearest-even (f16, bf16, and
 * OCP e4m3 / e5m2 with subnormals, saturating to the max finite value as a safety net).
 */
#ifndef XALM_SYNTH_H
#define XALM_SYNTH_H

#include <stdint.h>
#include <string.h>
#include <math.h>

#if defined(__HIPCC__)
#define XS_FN __host__ __device__ static inline
#else
#define XS_FN static inline
#endif

XS_FN uint64_t xs_mix(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

XS_FN float xs_u01(uint64_t h) { return (float)(uint32_t)(h >> 40) * (1.0f / 16777216.0f); }

XS_FN float xs_value(uint64_t seed, uint64_t i, float mean, float std) {
    const uint64_t h0 = xs_mix(seed ^ (i * 0xD1B54A32D192ED03ull));
    const uint64_t h1 = xs_mix(h0);
    const float u0 = xs_u01(h0), u1 = xs_u01(h0 << 24), u2 = xs_u01(h1), u3 = xs_u01(h1 << 24);
    const float s = ((u0 + u1) + (u2 + u3)) - 2.0f;
    return fmaf(s, std * 1.7320508f, mean);
}

XS_FN uint32_t xs_f32_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
XS_FN float xs_bits_f32(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

/* float -> bf16, RNE (finite inputs) */
XS_FN uint16_t xs_to_bf16(float f) {
    const uint32_t u = xs_f32_bits(f);
    return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

/* float -> IEEE half, RNE, finite inputs with |f| < 65504 (synthetic weights are small) */
XS_FN uint16_t xs_to_f16(float f) {
    const uint32_t x = xs_f32_bits(f);
    const uint16_t sign = (uint16_t)((x >> 16) & 0x8000u);
    const uint32_t a = x & 0x7FFFFFFFu;
    if (a >= 0x477FF000u) return (uint16_t)(sign | 0x7BFFu);          /* saturate */
    if (a < 0x38800000u) {                                            /* half subnormal / zero */
        const float m = xs_bits_f32(a) * 16777216.0f;                 /* |f| * 2^24, exact */
        /* RNE to integer without libm: add and subtract 2^23 */
        const float r = (m + 8388608.0f) - 8388608.0f;
        return (uint16_t)(sign | (uint16_t)r);
    }
    uint32_t m = a + 0xC8000000u;                                     /* rebias exponent 127 -> 15 */
    m = m + 0x0FFFu + ((m >> 13) & 1u);
    return (uint16_t)(sign | (uint16_t)(m >> 13));
}

/* float -> OCP fp8 with E exponent bits (4 or 5), M = 7 - E mantissa bits; RNE with
 * subnormals; saturates to the largest finite code (never produces NaN / Inf codes). */
XS_FN uint8_t xs_to_f8(float f, int E) {
    const int M = 7 - E;
    const int bias = (1 << (E - 1)) - 1;
    const uint32_t x = xs_f32_bits(f);
    const uint8_t sign = (uint8_t)((x >> 24) & 0x80u);
    const float a = xs_bits_f32(x & 0x7FFFFFFFu);
    const uint8_t maxcode = E == 4 ? 0x7E : 0x7B;
    const float maxval = E == 4 ? 448.0f : 57344.0f;
    if (!(a < maxval)) return (uint8_t)(sign | maxcode);
    const float min_normal = xs_bits_f32((uint32_t)(127 + 1 - bias) << 23);
    if (a < min_normal) {
        /* subnormal: value = q * 2^(1-bias-M), q in [0, 2^M]; RNE via 2^23 trick */
        const float scale = xs_bits_f32((uint32_t)(127 - (1 - bias - M)) << 23);
        const float q = (a * scale + 8388608.0f) - 8388608.0f;
        return (uint8_t)(sign | (uint8_t)q);  /* q == 2^M rolls into the first normal code */
    }
    uint32_t u = xs_f32_bits(a);
    const int sh = 23 - M;
    u = u + ((1u << (sh - 1)) - 1u) + ((u >> sh) & 1u);
    const int e = (int)(u >> 23) - 127 + bias;
    const uint32_t mant = (u >> sh) & ((1u << M) - 1u);
    uint32_t code = ((uint32_t)e << M) | mant;
    if (code > maxcode) code = maxcode;
    return (uint8_t)(sign | code);
}

/* ---- gguf blocks (XH_Q8_0 / XH_Q4_0): quantize 32 floats into one block of the converter's
 * file layout, restating quants.py (Q8_0.quantize_blocks :438-454, Q4_0.quantize_blocks
 * :283-299) with numpy's float32 semantics: a float32 op per numpy op, float16 by RNE,
 * np_roundf = round half away from zero, Q4_0's `trunc(float64(x) * float64(id) + 8.5)`
 * cast to float32 (the product of two floats is exact in double, so contraction cannot
 * change it). */
XS_FN float xs_roundf_away(float v) {
    const float a = fabsf(v);
    const float fl = floorf(a);
    const float b = fl + floorf(2.0f * (a - fl));
    return v < 0.0f ? -b : (v > 0.0f ? b : 0.0f * v);
}
/* out: 34 bytes, f16 d then 32 int8 */
XS_FN void xs_quant_q8_0(const float* v, uint8_t* out) {
    float amax = 0.0f;
    for (int k = 0; k < 32; k++) amax = fmaxf(amax, fabsf(v[k]));
    const float d = amax / 127.0f;
    const float id = d == 0.0f ? 0.0f : 1.0f / d;
    const uint16_t dh = xs_to_f16(d);
    out[0] = (uint8_t)(dh & 0xFFu);
    out[1] = (uint8_t)(dh >> 8);
    for (int k = 0; k < 32; k++) out[2 + k] = (uint8_t)(int8_t)xs_roundf_away(v[k] * id);
}
/* out: 18 bytes, f16 d then 16 bytes: byte j = q[j] | q[j+16] << 4 */
XS_FN void xs_quant_q4_0(const float* v, uint8_t* out) {
    int imax = 0;
    float amax = fabsf(v[0]);
    for (int k = 1; k < 32; k++)
        if (fabsf(v[k]) > amax) { amax = fabsf(v[k]); imax = k; }  /* argmax: the first maximum */
    const float d = v[imax] / -8.0f;
    const float id = d == 0.0f ? 0.0f : 1.0f / d;
    uint8_t q[32];
    for (int k = 0; k < 32; k++) {
        const float t = truncf((float)((double)v[k] * (double)id + 8.5));
        q[k] = (uint8_t)(t < 0.0f ? 0.0f : (t > 15.0f ? 15.0f : t));
    }
    const uint16_t dh = xs_to_f16(d);
    out[0] = (uint8_t)(dh & 0xFFu);
    out[1] = (uint8_t)(dh >> 8);
    for (int j = 0; j < 16; j++) out[2 + j] = (uint8_t)(q[j] | (q[j + 16] << 4));
}
/* ---- affine and 5-bit blocks (XH_Q4_1 / XH_Q5_0 / XH_Q5_1; quants.py Q4_1 :316-335, Q5_0
 * :353-374, Q5_1 :396-417).  numpy rounds `(v - min) * id` to float32 before it adds 0.5: the
 * product is formed in double (exact: 24 x 24 bits) and rounded once, and the sum likewise (a
 * double sum of two floats rounds to float as the float sum does), so no compiler can contract
 * the two into one fma. */
XS_FN float xs_mul_add_half(float a, float b) {
    const float p = (float)((double)a * (double)b);
    return (float)((double)p + 0.5);
}
XS_FN void xs_put_f16(uint8_t* out, float v) {
    const uint16_t h = xs_to_f16(v);
    out[0] = (uint8_t)(h & 0xFFu);
    out[1] = (uint8_t)(h >> 8);
}
/* codes q[32] (0..31) -> 16 bytes of nibbles (byte j = q[j] & 15 | q[j+16] << 4) and, when
 * qh != NULL, the 4 little-endian bytes of the fifth bits (bit j = q[j] >> 4) */
XS_FN void xs_pack_codes(const uint8_t* q, uint8_t* qh, uint8_t* qs) {
    for (int j = 0; j < 16; j++) qs[j] = (uint8_t)((q[j] & 15u) | ((q[j + 16] & 15u) << 4));
    if (qh) {
        uint32_t h = 0;
        for (int j = 0; j < 32; j++) h |= (uint32_t)(q[j] >> 4) << j;
        for (int k = 0; k < 4; k++) qh[k] = (uint8_t)(h >> (8 * k));
    }
}
/* min / max form, `levels` = 15 (Q4_1) or 31 (Q5_1): d = (max - min) / levels, m = min,
 * q = trunc((v - min) * id + 0.5) in float32, id = 0 when d == 0 */
XS_FN void xs_quant_affine(const float* v, int levels, float* d_out, float* m_out, uint8_t* q) {
    float mx = v[0], mn = v[0];
    for (int k = 1; k < 32; k++) { mx = fmaxf(mx, v[k]); mn = fminf(mn, v[k]); }
    const float d = (mx - mn) / (float)levels;
    const float id = d == 0.0f ? 0.0f : 1.0f / d;
    for (int k = 0; k < 32; k++) {
        const float t = truncf(xs_mul_add_half(v[k] - mn, id));
        q[k] = (uint8_t)(t < 0.0f ? 0.0f : (t > (float)levels ? (float)levels : t));
    }
    *d_out = d;
    *m_out = mn;
}
/* out: 20 bytes, f16 d, f16 m, 16 bytes of nibbles; value d*q + m */
XS_FN void xs_quant_q4_1(const float* v, uint8_t* out) {
    float d, m;
    uint8_t q[32];
    xs_quant_affine(v, 15, &d, &m, q);
    xs_put_f16(out, d);
    xs_put_f16(out + 2, m);
    xs_pack_codes(q, (uint8_t*)0, out + 4);
}
/* out: 22 bytes, f16 d, u32 qh (little endian), 16 bytes of nibbles; value d*(q - 16).
 * `trunc(float64(x) * float64(id) + 16.5)` cast to float32, as Q4_0's 8.5 */
XS_FN void xs_quant_q5_0(const float* v, uint8_t* out) {
    int imax = 0;
    float amax = fabsf(v[0]);
    for (int k = 1; k < 32; k++)
        if (fabsf(v[k]) > amax) { amax = fabsf(v[k]); imax = k; }  /* argmax: the first maximum */
    const float d = v[imax] / -16.0f;
    const float id = d == 0.0f ? 0.0f : 1.0f / d;
    uint8_t q[32];
    for (int k = 0; k < 32; k++) {
        const float t = truncf((float)((double)v[k] * (double)id + 16.5));
        q[k] = (uint8_t)(t < 0.0f ? 0.0f : (t > 31.0f ? 31.0f : t));
    }
    xs_put_f16(out, d);
    xs_pack_codes(q, out + 2, out + 6);
}
/* out: 24 bytes, f16 d, f16 m, u32 qh, 16 bytes of nibbles; value d*q + m, q = 0..31 */
XS_FN void xs_quant_q5_1(const float* v, uint8_t* out) {
    float d, m;
    uint8_t q[32];
    xs_quant_affine(v, 31, &d, &m, q);
    xs_put_f16(out, d);
    xs_put_f16(out + 2, m);
    xs_pack_codes(q, out + 4, out + 8);
}
/* ---- OCP microscaling FP4 (XH_MXFP4 = 25): 32 e2m1 codes under one E8M0 scale, 17 bytes: e, then
 * 16 bytes with element j in the low and j + 16 in the high nibble of byte j.  Code c is
 * (c >> 3 ? -1 : 1) * {0, 0.5, 1, 1.5, 2, 3, 4, 6}[c & 7], a weight value(c) * 2^(e - 127).
 * E = clamp(floor(log2(amax)) - 2, -127, 127) from the exponent bits (a subnormal amax by its
 * leading bit), so amax * 2^-E lies in [4, 8) unless E is clamped; every |v| * 2^-E is an exact
 * product (a power of two; where it would underflow it is far below the first threshold), and the
 * nearest magnitude is chosen by comparisons against the exact midpoints, ties to the even code. */
XS_FN uint8_t xs_e2m1_code(float v, float inv) {
    const uint32_t u = xs_f32_bits(v);
    const float t = xs_bits_f32(u & 0x7FFFFFFFu) * inv;
    const int c = (t > 0.25f) + (t >= 0.75f) + (t > 1.25f) + (t >= 1.75f) + (t > 2.5f) + (t >= 3.5f) + (t > 5.0f);
    return (uint8_t)((u >> 31) << 3 | (uint32_t)c);
}
/* out: 17 bytes */
XS_FN void xs_quant_mxfp4(const float* v, uint8_t* out) {
    uint32_t amax = 0;  /* |v| orders as its bits */
    for (int k = 0; k < 32; k++) {
        const uint32_t a = xs_f32_bits(v[k]) & 0x7FFFFFFFu;
        if (a > amax) amax = a;
    }
    if (amax == 0) {
        for (int k = 0; k < 17; k++) out[k] = 0;
        return;
    }
    int fl;  /* floor(log2(amax)) */
    if (amax >> 23) {
        fl = (int)(amax >> 23) - 127;
    } else {
        int top = 22;
        while (!((amax >> top) & 1u)) top--;
        fl = top - 149;
    }
    int E = fl - 2;
    if (E < -127) E = -127;
    if (E > 127) E = 127;
    /* 2^-E: normal for E <= 126; E = 127 (unreachable: fl <= 127) would be the subnormal 2^-127 */
    const float inv = xs_bits_f32(E <= 126 ? (uint32_t)(127 - E) << 23 : 0x00400000u);
    out[0] = (uint8_t)(E + 127);
    for (int j = 0; j < 16; j++) out[1 + j] = (uint8_t)(xs_e2m1_code(v[j], inv) | (xs_e2m1_code(v[j + 16], inv) << 4));
}
/* one block of `dtype` (20 Q8_0, 21 Q4_0, 22 Q4_1, 23 Q5_0, 24 Q5_1, 25 MXFP4) from 32 floats; returns the
 * block's bytes, 0 for another dtype */
XS_FN int xs_quant_block(int dtype, const float* v, uint8_t* out) {
    switch (dtype) {
        case 20: xs_quant_q8_0(v, out); return 34;
        case 21: xs_quant_q4_0(v, out); return 18;
        case 22: xs_quant_q4_1(v, out); return 20;
        case 23: xs_quant_q5_0(v, out); return 22;
        case 24: xs_quant_q5_1(v, out); return 24;
        case 25: xs_quant_mxfp4(v, out); return 17;
        default: return 0;
    }
}
/* synthetic block b of row r of a [rows][cols] tensor: the 32 values xs_value gives elements
 * r*cols + 32b .. +31, quantized (dtype 20 Q8_0 / 21 Q4_0 / 22 Q4_1 / 23 Q5_0 / 24 Q5_1 / 25 MXFP4) */
XS_FN void xs_block(uint8_t* out, int dtype, uint64_t seed, uint64_t r, uint64_t cols, uint64_t b, float mean, float std) {
    float v[32];
    for (int k = 0; k < 32; k++) v[k] = xs_value(seed, r * cols + 32 * b + k, mean, std);
    if (dtype == 20) xs_quant_q8_0(v, out);
    else if (dtype >= 22 && dtype <= 25) xs_quant_block(dtype, v, out);
    else xs_quant_q4_0(v, out);
}

/* ---- gguf K-quants (XH_Q4_K = 26, XH_Q6_K = 27): one super-block from 256 floats.  The reference
 * ships only their decoders (quants.py Q4_K / Q6_K dequantize_blocks); the quantizers are this
 * project's, defined in xalm_hip.h at xh_quantize_blocks: min / max per sub-block, the 6-bit / int8
 * sub-block scales against the super-block's largest.  Every f32 operation below stands alone (a
 * division or an addition behind a division: nothing a compiler can contract), so gcc, hipcc and
 * numpy agree byte for byte. */
XS_FN float xs_from_f16(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
    const uint32_t e = (h >> 10) & 31u, m = h & 0x3FFu;
    if (e == 0) return xs_bits_f32(sign | xs_f32_bits((float)m * (1.0f / 16777216.0f)));  /* m * 2^-24 */
    return xs_bits_f32(sign | ((e + 112u) << 23) | (m << 13));                          /* finite (e < 31) */
}
/* min(cap, floorf(a / d + 0.5f)), 0 when d == 0 (a >= 0) */
XS_FN int xs_kq_field(float a, float d, int cap) {
    if (d == 0.0f) return 0;
    const float t = a / d;
    const float r = floorf(t + 0.5f);
    return r > (float)cap ? cap : (int)r;
}
/* out: 144 bytes, f16 d, f16 dmin, s[12], qs[128] */
XS_FN void xs_quant_q4_k(const float* v, uint8_t* out) {
    float a[8], b[8], amax = 0.0f, bmax = 0.0f;
    for (int j = 0; j < 8; j++) {
        float mx = v[32 * j], lo = fminf(v[32 * j], 0.0f);
        for (int k = 1; k < 32; k++) { mx = fmaxf(mx, v[32 * j + k]); lo = fminf(lo, v[32 * j + k]); }
        a[j] = (mx - lo) / 15.0f;
        b[j] = 0.0f - lo;  /* +0 for lo == 0 */
        amax = fmaxf(amax, a[j]);
        bmax = fmaxf(bmax, b[j]);
    }
    const uint16_t dh = xs_to_f16(amax / 63.0f), mh = xs_to_f16(bmax / 63.0f);
    const float d = xs_from_f16(dh), dmin = xs_from_f16(mh);
    out[0] = (uint8_t)(dh & 0xFFu); out[1] = (uint8_t)(dh >> 8);
    out[2] = (uint8_t)(mh & 0xFFu); out[3] = (uint8_t)(mh >> 8);
    uint8_t sc[8], mn[8], q[256];
    for (int j = 0; j < 8; j++) {
        sc[j] = (uint8_t)xs_kq_field(a[j], d, 63);
        mn[j] = (uint8_t)xs_kq_field(b[j], dmin, 63);
        const float D = d * (float)sc[j], M = dmin * (float)mn[j];  /* exact: 11 + 6 bits */
        for (int k = 0; k < 32; k++) {
            float r = 0.0f;
            if (D != 0.0f) {
                const float t = (v[32 * j + k] + M) / D;
                r = floorf(t + 0.5f);
            }
            q[32 * j + k] = (uint8_t)(r < 0.0f ? 0.0f : (r > 15.0f ? 15.0f : r));
        }
    }
    uint8_t* s = out + 4;
    for (int j = 0; j < 4; j++) {
        s[j] = (uint8_t)(sc[j] | ((sc[j + 4] >> 4) << 6));
        s[j + 4] = (uint8_t)(mn[j] | ((mn[j + 4] >> 4) << 6));
        s[j + 8] = (uint8_t)((sc[j + 4] & 15u) | ((mn[j + 4] & 15u) << 4));
    }
    for (int g = 0; g < 4; g++)
        for (int l = 0; l < 32; l++) out[16 + 32 * g + l] = (uint8_t)(q[64 * g + l] | (q[64 * g + 32 + l] << 4));
}
/* out: 210 bytes, ql[128], qh[64], int8 sc[16], f16 d */
XS_FN void xs_quant_q6_k(const float* v, uint8_t* out) {
    float a[16], amax = 0.0f;
    for (int g = 0; g < 16; g++) {
        float m = 0.0f;
        for (int k = 0; k < 16; k++) m = fmaxf(m, fabsf(v[16 * g + k]));
        a[g] = m / 31.0f;
        amax = fmaxf(amax, a[g]);
    }
    const uint16_t dh = xs_to_f16(amax / 127.0f);
    const float d = xs_from_f16(dh);
    uint8_t q[256];
    for (int g = 0; g < 16; g++) {
        const int sc = xs_kq_field(a[g], d, 127);
        out[192 + g] = (uint8_t)sc;
        const float D = d * (float)sc;  /* exact: 11 + 7 bits */
        for (int k = 0; k < 16; k++) {
            float r = 0.0f;
            if (D != 0.0f) {
                const float t = v[16 * g + k] / D;
                r = floorf(t + 32.5f);
            }
            q[16 * g + k] = (uint8_t)(r < 0.0f ? 0.0f : (r > 63.0f ? 63.0f : r));
        }
    }
    for (int h = 0; h < 2; h++)
        for (int l = 0; l < 32; l++) {
            const uint8_t* e = q + 128 * h + l;  /* e[32 k]: element 128h + 32k + l */
            out[64 * h + l] = (uint8_t)((e[0] & 15u) | ((e[64] & 15u) << 4));
            out[64 * h + 32 + l] = (uint8_t)((e[32] & 15u) | ((e[96] & 15u) << 4));
            out[128 + 32 * h + l] = (uint8_t)((e[0] >> 4) | ((e[32] >> 4) << 2) | ((e[64] >> 4) << 4) | ((e[96] >> 4) << 6));
        }
    out[208] = (uint8_t)(dh & 0xFFu);
    out[209] = (uint8_t)(dh >> 8);
}
/* the decoders (the definition in xalm_hip.h): 256 floats from one super-block */
XS_FN void xs_dequant_q4_k(const uint8_t* in, float* o) {
    const float d = xs_from_f16((uint16_t)(in[0] | in[1] << 8)), dmin = xs_from_f16((uint16_t)(in[2] | in[3] << 8));
    const uint8_t* s = in + 4;
    for (int j = 0; j < 8; j++) {
        const int sc = j < 4 ? s[j] & 63 : (s[j + 4] & 15) | ((s[j - 4] >> 6) << 4);
        const int mn = j < 4 ? s[j + 4] & 63 : (s[j + 4] >> 4) | ((s[j] >> 6) << 4);
        const float D = d * (float)sc, M = dmin * (float)mn;
        for (int l = 0; l < 32; l++) {
            const uint8_t b = in[16 + 32 * (j >> 1) + l];
            o[32 * j + l] = fmaf(D, (float)((j & 1) ? b >> 4 : b & 15u), -M);
        }
    }
}
XS_FN void xs_dequant_q6_k(const uint8_t* in, float* o) {
    const float d = xs_from_f16((uint16_t)(in[208] | in[209] << 8));
    for (int e = 0; e < 256; e++) {
        const int h = e >> 7, k = (e >> 5) & 3, l = e & 31;
        const int lo = (in[64 * h + 32 * (k & 1) + l] >> (4 * (k >> 1))) & 15;
        const int hi = (in[128 + 32 * h + l] >> (2 * k)) & 3;
        o[e] = (d * (float)(int8_t)in[192 + (e >> 4)]) * (float)((lo | (hi << 4)) - 32);
    }
}
/* synthetic super-block b of row r of a [rows][cols] tensor (dtype 26 Q4_K / 27 Q6_K): the 256 values
 * xs_value gives elements r*cols + 256b .. +255, quantized; out: 144 / 210 bytes */
XS_FN void xs_superblock(uint8_t* out, int dtype, uint64_t seed, uint64_t r, uint64_t cols, uint64_t b, float mean, float std) {
    float v[256];
    for (int k = 0; k < 256; k++) v[k] = xs_value(seed, r * cols + 256 * b + k, mean, std);
    if (dtype == 26) xs_quant_q4_k(v, out);
    else xs_quant_q6_k(v, out);
}

/* dtype ids as in xalm_hip.h: 1 F32, 2 F16, 3 BF16, 6 F8_E4M3, 7 F8_E5M2 */
XS_FN void xs_store(void* dst, uint64_t idx, int dtype, float v) {
    switch (dtype) {
        case 1: ((float*)dst)[idx] = v; break;
        case 2: ((uint16_t*)dst)[idx] = xs_to_f16(v); break;
        case 3: ((uint16_t*)dst)[idx] = xs_to_bf16(v); break;
        case 6: ((uint8_t*)dst)[idx] = xs_to_f8(v, 4); break;
        case 7: ((uint8_t*)dst)[idx] = xs_to_f8(v, 5); break;
        default: break;
    }
}

#endif
