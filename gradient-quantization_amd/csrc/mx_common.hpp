// The device functions libgq_mx.so (mx.hip) and libgq_mxr.so (mxr.hip) share: the formats, the block exponent, the code of an
// element and the value of a code, as include/gq_mx.h defines them.  Internal linkage: each library compiles its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "gq_mx.h"

namespace gqx {

constexpr uint32_t QNAN = 0x7fc00000u;
enum { DRAW_OFF = 0, DRAW_GIVEN = 1, DRAW_DEVICE = 2 };

template <int FMT>
struct Fmt;
template <>
struct Fmt<GQ_MX_FP4> {
    static constexpr int bits = 4, mb = 1, bias = 1, emax = 2;
    static constexpr uint32_t mthr = 0x400000u;
};
template <>
struct Fmt<GQ_MX_FP8> {
    static constexpr int bits = 8, mb = 3, bias = 7, emax = 8;
    static constexpr uint32_t mthr = 0x600000u;
};

__host__ __device__ constexpr int64_t up16(int64_t x) { return (x + 15) / 16 * 16; }

// the block exponent e of a block whose largest magnitude has the bits a (finite), integers only
template <class F>
__device__ __forceinline__ int block_exponent(uint32_t a) {
    const int E = (int)(a >> 23);
    const uint32_t M = a & 0x7fffffu;
    const int ea = E ? E - 127 : -126;
    const int over = (E != 0 && M > F::mthr) ? 1 : 0;
    return max(ea - F::emax + over, -127);
}

// the magnitude code of |w| in a block of exponent e: c_lo, or c_lo + 1 by the draw r (MODE != DRAW_OFF) or to nearest-even
template <class F, int MODE>
__device__ __forceinline__ uint32_t magnitude_code(uint32_t wbits, int e, float r) {
    const float y = ldexpf(__uint_as_float(wbits & 0x7fffffffu), -e);      // one rounding; exact unless subnormal
    const uint32_t yb = __float_as_uint(y);
    const int Ey = (int)(yb >> 23);
    const uint32_t S = (yb & 0x7fffffu) | (Ey ? 0x800000u : 0u);           // y = S * 2^(max(Ey, 1) - 150)
    const int d = (128 - F::bias) - max(Ey, 1);                            // > 0: y lies below the format's normal range
    const int shift = 23 - F::mb + max(d, 0);                              // t = y / q = S * 2^-shift
    const int sh = min(shift, 31);                                         // (S < 2^24: k = 0 and rem = S from 24 on)
    const uint32_t k = S >> sh;
    const uint32_t rem = S - (k << sh);
    const uint32_t c_lo = ((uint32_t)max(-d, 0) << F::mb) + k;
    bool up;
    if (MODE == DRAW_OFF) {
        const uint32_t half = 1u << (sh - 1);
        up = rem > half || (rem == half && (c_lo & 1u));
    } else {
        const float frac = ldexpf((float)rem, -shift);                     // exact: rem < 2^24, the result a multiple of 2^-149
        up = frac > r;
    }
    return c_lo + (up ? 1u : 0u);
}

// +-ldexp(mag(c), e) of a code (sign in bit bits - 1): one exact scaling, +-inf from 2^128 on
template <class F>
__device__ __forceinline__ float decode_value(uint32_t code, int e) {
    const uint32_t c = code & ((1u << (F::bits - 1)) - 1u);
    const uint32_t ce = c >> F::mb, cm = c & ((1u << F::mb) - 1u);
    const uint32_t sig = ce ? (cm | (1u << F::mb)) : cm;
    const float m = ldexpf((float)sig, (int)max(ce, 1u) - F::bias - F::mb + e);
    return __uint_as_float(__float_as_uint(m) | ((code >> (F::bits - 1)) << 31));
}

}  // namespace gqx
