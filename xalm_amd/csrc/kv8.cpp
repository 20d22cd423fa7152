// kv8.cpp — the element of the fp8 (e4m3) KV ring on the host: plain C++, integer arithmetic on the
// f32 bits, no HIP.  xh_f8_e4m3_from_f32 is the definition of what every K/V writer of an fp8
// context stores (the qkv epilogues, the sink re-rotation, the synthetic fill); the device forms
// (kv8_pack, common.h) are held to it bit for bit by tests/test_kv8_gpu.py.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/xalm_hip.h"

namespace {

// Clamp to [-448, 448] with f32 min / max, then the nearest e4m3fn value, ties to the even
// mantissa; subnormals (multiples of 2^-9) down to 2^-9; below 2^-10, and the tie at 2^-10, a
// signed zero.  The sign is kept (-0 -> 0x80).  NaN is outside the contract.
uint8_t f8_e4m3_from_f32(float v) {
    v = std::fmin(std::fmax(v, -448.0f), 448.0f);
    uint32_t u;
    memcpy(&u, &v, 4);
    const uint8_t sign = (uint8_t)((u >> 24) & 0x80u);
    u &= 0x7fffffffu;
    if (u >= (121u << 23)) {
        // |v| >= 2^-6, e4m3's least normal: the mantissa to 3 bits, half to even (a carry runs
        // into the exponent, as it should); the exponent rebiased from 127 to 7
        const uint32_t r = (u + 0x7ffffu + ((u >> 20) & 1u)) >> 20;
        return sign | (uint8_t)(r - (120u << 3));
    }
    // below: q = |v| / 2^-9 to an integer, half to even; q = 8 is the least normal's code
    const int e = (int)(u >> 23);
    if (e < 116) return sign;  // |v| < 2^-11 (f32 subnormals included)
    const uint32_t m = (u & 0x7fffffu) | 0x800000u;  // |v| = m 2^(e - 150)
    const int shift = 141 - e;                       // 21 .. 25
    const uint32_t half = 1u << (shift - 1), rem = m & ((1u << shift) - 1u);
    uint32_t q = m >> shift;
    if (rem > half || (rem == half && (q & 1u))) q++;
    return sign | (uint8_t)q;
}

}  // namespace

extern "C" int xh_f8_e4m3_from_f32(const float* in, size_t n, uint8_t* out) {
    if (!in || !out) return XH_E_INVALID;
    for (size_t i = 0; i < n; i++) out[i] = f8_e4m3_from_f32(in[i]);
    return 0;
}
