// evrep_f16.h -- the two 16-bit map formats of the detector's entry points (include/evrep.h, rules W1 and W2): float16 and
// bfloat16 as their 16 bits, widened exactly to float32 and rounded once, to nearest even, from float32.  Integer arithmetic
// only, the same statements on the host and on the device, so a CPU build runs what the kernels run (evrep_cast16_host) and no
// conversion depends on a denormal or rounding mode of either machine.
//
//   widen   float16: sign, exponent rebiased by 112, mantissa shifted by 13; a subnormal m * 2^-24 is formed as float(m) * 2^-24
//           (both exact); inf and NaN keep their mantissa bits.  bfloat16: the 16 bits on top of 16 zero bits.
//   round   float16: a NaN stays a NaN (quiet, sign kept); |x| >= 65520 (the largest finite value plus half an ulp, a tie that
//           goes to the even side) is +-inf; |x| <= 2^-25 (a tie again) is +-0, so every float32 subnormal is; from 2^-14 on the
//           mantissa is rounded by adding 0xFFF + lsb in front of the shift, a carry runs into the exponent as it should; in
//           between the 24-bit significand is shifted to units of 2^-24 with the remainder compared to one half.
//           bfloat16: a NaN stays a NaN; else 0x7FFF + lsb is added in front of the shift: an overflow ends at +-inf by the
//           carry, and float32's subnormals round to bfloat16's, which have the same exponent.
// Both roundings give torch's float32_tensor.to(dtype) bit for bit wherever the value is no NaN.
#pragma once
#include <stdint.h>
#include <string.h>

#include "evrep.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EVREP_HD __host__ __device__
#else
#define EVREP_HD
#endif

namespace evrep {

EVREP_HD inline float f16_from_bits32(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
EVREP_HD inline uint32_t f16_to_bits32(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

EVREP_HD inline float widen_f16(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3FFu;
    if (e == 0u) {
        const float v = (float)(int32_t)m * 5.9604644775390625e-08f;      // m * 2^-24: exact, and a normal float32 (or 0)
        return f16_from_bits32(sign | f16_to_bits32(v));
    }
    if (e == 31u) return f16_from_bits32(sign | 0x7F800000u | (m << 13));
    return f16_from_bits32(sign | ((e + 112u) << 23) | (m << 13));
}

EVREP_HD inline float widen_bf16(uint16_t h) { return f16_from_bits32((uint32_t)h << 16); }

EVREP_HD inline uint16_t round_f16(float f) {
    const uint32_t x = f16_to_bits32(f), sign = (x >> 16) & 0x8000u;
    uint32_t a = x & 0x7FFFFFFFu;
    if (a > 0x7F800000u) return (uint16_t)(sign | 0x7E00u);              // NaN
    if (a >= 0x477FF000u) return (uint16_t)(sign | 0x7C00u);             // >= 65520: inf
    if (a >= 0x38800000u) {                                              // >= 2^-14: a normal float16
        a += 0xFFFu + ((a >> 13) & 1u);
        return (uint16_t)(sign | ((a - 0x38000000u) >> 13));
    }
    if (a <= 0x33000000u) return (uint16_t)sign;                         // <= 2^-25: zero
    const uint32_t e = a >> 23, m = (a & 0x7FFFFFu) | 0x800000u, shift = 126u - e;   // 14 .. 24
    uint32_t r = m >> shift;
    const uint32_t rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1u);
    if (rem > half || (rem == half && (r & 1u))) ++r;
    return (uint16_t)(sign | r);
}

EVREP_HD inline uint16_t round_bf16(float f) {
    const uint32_t x = f16_to_bits32(f);
    if ((x & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((x >> 16) | 0x40u);   // NaN
    return (uint16_t)((x + 0x7FFFu + ((x >> 16) & 1u)) >> 16);
}

// by dtype code (EVREP_DT_F16 or EVREP_DT_BF16; the callers have checked it)
EVREP_HD inline float widen16(uint16_t h, int dt) { return dt == EVREP_DT_F16 ? widen_f16(h) : widen_bf16(h); }
EVREP_HD inline uint16_t round16(float f, int dt) { return dt == EVREP_DT_F16 ? round_f16(f) : round_bf16(f); }

}  // namespace evrep
