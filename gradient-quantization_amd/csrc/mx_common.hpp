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
template <>
struct Fmt<GQ_MX_FP6_E2M3> {
    static constexpr int bits = 6, mb = 3, bias = 1, emax = 2;
    static constexpr uint32_t mthr = 0x700000u;
};
template <>
struct Fmt<GQ_MX_FP6_E3M2> {
    static constexpr int bits = 6, mb = 2, bias = 3, emax = 4;
    static constexpr uint32_t mthr = 0x600000u;
};

__host__ __device__ constexpr int64_t up16(int64_t x) { return (x + 15) / 16 * 16; }

// ---- the tensor-side element type (include/gq_mx.h, TENSOR-SIDE TYPE): sources, both launches' `out`, dense-copy sources -----------
// An enum, not a C++ type, so that another 16-bit format can follow (its widen / narrow pair and a Tensor<> line).
enum { TT_F32 = 0, TT_BF16 = 1 };
template <int TT>
struct Tensor;
template <>
struct Tensor<TT_F32> {
    using type = float;
};
template <>
struct Tensor<TT_BF16> {
    using type = uint16_t;
};

// widen: the f32 with bits h << 16 -- exact, NaNs and signed zeros included
__device__ __forceinline__ float widen(uint16_t h) { return __uint_as_float((uint32_t)h << 16); }

// narrow: round to nearest even onto bf16, in integers; every NaN becomes 0x7FC0.  The carry runs into the exponent and reaches
// +-inf at the top; f32 subnormals round onto bf16's grid as they are.
__device__ __forceinline__ uint16_t narrow(float x) {
    const uint32_t b = __float_as_uint(x);
    if ((b & 0x7fffffffu) > 0x7f800000u) return (uint16_t)0x7FC0u;
    return (uint16_t)((b + 0x7FFFu + ((b >> 16) & 1u)) >> 16);
}

__device__ __forceinline__ float to_f32(float x) { return x; }
__device__ __forceinline__ float to_f32(uint16_t h) { return widen(h); }
template <class T>
__device__ __forceinline__ T from_f32(float x);
template <>
__device__ __forceinline__ float from_f32<float>(float x) {
    return x;
}
template <>
__device__ __forceinline__ uint16_t from_f32<uint16_t>(float x) {
    return narrow(x);
}
__device__ __forceinline__ uint32_t narrow2(float lo, float hi) { return (uint32_t)narrow(lo) | ((uint32_t)narrow(hi) << 16); }

// A lane's 8 elements as f32, full form: all 8 exist and p is 16-byte aligned -- two float4 loads, or ONE 16-byte load of 8 bf16.
__device__ __forceinline__ void load8(const float *p, float (&w)[8]) {
    const float4 a0 = *reinterpret_cast<const float4 *>(p), a1 = *reinterpret_cast<const float4 *>(p + 4);
    w[0] = a0.x, w[1] = a0.y, w[2] = a0.z, w[3] = a0.w, w[4] = a1.x, w[5] = a1.y, w[6] = a1.z, w[7] = a1.w;
}
__device__ __forceinline__ void load8(const uint16_t *p, float (&w)[8]) {
    const uint4 a = *reinterpret_cast<const uint4 *>(p);
    w[0] = __uint_as_float(a.x << 16), w[1] = __uint_as_float(a.x & 0xffff0000u);
    w[2] = __uint_as_float(a.y << 16), w[3] = __uint_as_float(a.y & 0xffff0000u);
    w[4] = __uint_as_float(a.z << 16), w[5] = __uint_as_float(a.z & 0xffff0000u);
    w[6] = __uint_as_float(a.w << 16), w[7] = __uint_as_float(a.w & 0xffff0000u);
}
// ragged form (a tensor's end, or a view that is not 16-byte aligned): the kernels walk the elements that exist one by one --
// to_f32(p[k]) is the scalar load, p[k] = from_f32<T>(x) the scalar store

// 8 f32 into a lane's 8 elements of T, full form (as load8): two float4 stores, or ONE 16-byte store of 8 narrowed values
__device__ __forceinline__ void store8(float *p, const float (&f)[8]) {
    *reinterpret_cast<float4 *>(p) = make_float4(f[0], f[1], f[2], f[3]);
    *reinterpret_cast<float4 *>(p + 4) = make_float4(f[4], f[5], f[6], f[7]);
}
__device__ __forceinline__ void store8(uint16_t *p, const float (&f)[8]) {
    *reinterpret_cast<uint4 *>(p) = make_uint4(narrow2(f[0], f[1]), narrow2(f[2], f[3]), narrow2(f[4], f[5]), narrow2(f[6], f[7]));
}
// gql::copy_dense with sources of T: the identity-compressed tensors into the wire's f32 dense region, widened where T is 16-bit
template <int THREADS, class T>
__device__ __forceinline__ void copy_dense_as_f32(const int64_t *__restrict__ dense_table, int ndense, uint8_t *__restrict__ wire) {
    for (int t = blockIdx.x; t < ndense; t += gridDim.x) {
        const T *src = reinterpret_cast<const T *>(dense_table[3 * t]);
        float *dst = reinterpret_cast<float *>(wire + dense_table[3 * t + 1]);
        const int64_t n = dense_table[3 * t + 2];
        for (int64_t i = threadIdx.x; i < n; i += THREADS) dst[i] = to_f32(src[i]);
    }
}

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

// ---- the 6-bit wire: a block is 24 bytes at 24 * blk, element i in bits 6i .. 6i+5 of the little-endian bit string ----------------
// A lane's eight codes are 48 bits at byte 6 * (lane & 3) of its block; lo = bits 0 .. 31, hi = bits 32 .. 47.

// The quad's 24 bytes as three 8-byte stores (24 * blk is 8-byte aligned: the wire is 16-byte aligned, and so are a section and
// its scale bytes).  The block is the 192-bit string v0 | v1 << 48 | v2 << 96 | v3 << 144 of the lanes' 48-bit values; lane
// q = 0, 1, 2 stores its bits 64 q .. 64 q + 63 = (v_q >> 16 q) | (v_{q+1} << (48 - 16 q)): the next lane's lo and hi come by two
// DPP moves, and the two 64-bit shifts by the lane's own q need no select and no branch.  Lane 3 stores nothing of the block --
// it writes the 8 zero bytes that pad an odd number of blocks to 16, behind the last one.
// EVERY lane of the wave calls this (the DPP moves sit outside the bounds test); c[k] < 64.
__device__ __forceinline__ void store_codes6(uint8_t *codes, int64_t blk, int64_t nb, const uint32_t (&c)[8]) {
    const uint32_t lo = c[0] | (c[1] << 6) | (c[2] << 12) | (c[3] << 18) | (c[4] << 24) | (c[5] << 30);
    const uint32_t hi = (c[5] >> 2) | (c[6] << 4) | (c[7] << 10);
    const uint32_t nlo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)lo, 0xF9, 0xF, 0xF, true);      // quad_perm [1, 2, 3, 3]
    const uint32_t nhi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)hi, 0xF9, 0xF, 0xF, true);
    const uint32_t q = threadIdx.x & 3u;
    const uint64_t v = ((uint64_t)hi << 32) | lo, nv = ((uint64_t)nhi << 32) | nlo;
    const uint64_t d = (v >> (16 * q)) | (nv << (48 - 16 * q));      // (q = 3: not stored)
    if (blk < nb) {
        if (q < 3)
            *reinterpret_cast<uint2 *>(codes + 24 * blk + 8 * q) = make_uint2((uint32_t)d, (uint32_t)(d >> 32));
        else if (blk == nb - 1 && (nb & 1))
            *reinterpret_cast<uint2 *>(codes + 24 * nb) = make_uint2(0u, 0u);
    }
}

// A lane's 48 bits from cp = the payload's codes + 6 * (e0 / 8).  words (the payload 4-byte aligned): a pair of lanes owns 12
// bytes = three dwords at a multiple of 12; the even lane loads dwords 0 and 1, the odd lane dwords 1 and 2 -- both inside the
// pair, so inside the section, and no lane waits for another (gfx950 takes the pair of dwords as one 8-byte load at a 4-byte
// aligned address; the compiler emits that).  Otherwise its own six bytes (emitted as a dword and a 16-bit load of them).
__device__ __forceinline__ uint64_t load_codes6(const uint8_t *cp, bool odd, bool words) {
    if (words) {
        const uint32_t *p = reinterpret_cast<const uint32_t *>(cp - (odd ? 2 : 0));
        const uint32_t a = p[0], b = p[1];
        return odd ? ((uint64_t)b << 16) | (a >> 16) : ((uint64_t)(b & 0xffffu) << 32) | a;
    }
    uint64_t v = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) v |= (uint64_t)cp[k] << (8 * k);
    return v;
}

}  // namespace gqx
