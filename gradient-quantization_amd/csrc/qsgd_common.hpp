// What the QSGD kernels of libgq_hsq.so share (qsgd.hip, qsgd_batched.hip, qsgd_wide.hip): ONE coder, ONE de-quantiser, ONE packer and
// unpacker of code units and pairs, the element-pair and unit walks of a bucket, and the launchers' argument checks.  The wire:
// one code per element = sign << (bits - 1) | level, bits = 4 (two per byte, element 2i in the low nibble), 8 or 16 (little-endian).
#pragma once
#include "gq_common.hpp"

namespace gq {

typedef float __attribute__((address_space(1))) *gf_ptr;          // global address-space pointers: as plain pointers these
typedef float v2f __attribute__((ext_vector_type(2)));            // would be flat when they come out of a table (see hsq_encode_pf.hip)
typedef v2f __attribute__((address_space(1))) *gf2_ptr;
typedef f32x4 __attribute__((address_space(1))) *gv_ptr;
typedef const uint8_t __attribute__((address_space(1))) *gbyte_ptr;
typedef const float __attribute__((address_space(1))) gfloat;
typedef unsigned uv2 __attribute__((ext_vector_type(2)));
typedef unsigned uv4 __attribute__((ext_vector_type(4)));

// ---- the draws ------------------------------------------------------------------------------------------------------------------
// The draws of the bucketed kernels (GQ_RANDOM_DEVICE*: the library's own numbers, only their distribution is specified):
// element e of bucket b draws  u = top 24 bits of mix(key(seed, b) + e * phi) * 2^-24  with key = the library's three-round
// hash of (seed, b), taken ONCE per bucket and lane, and mix = one multiply-xorshift round.  The elements of a bucket walk a
// Weyl sequence through a bijective mixer; buckets and steps are separated by the full hash.  Round 5 ran the three-round hash
// (and a 64-bit index) per ELEMENT: ~20 of the ~46 vector instructions an element cost.
__device__ __forceinline__ uint32_t bucket_draw_key(uint64_t seed, int64_t b) { return uniform_bits(seed, (uint64_t)b); }
__device__ __forceinline__ float bucket_draw(uint32_t key, uint32_t e) {
    uint32_t h = key + e * 0x9E3779B1u;
    h ^= h >> 16;
    h *= 0x7FEB352Du;                                   // (the top 24 bits of the product are its best-mixed ones)
    return (float)(h >> 8) * 5.9604644775390625e-08f;   // k * 2^-24, the grid torch.rand uses for float32
}

// ---- the coder ------------------------------------------------------------------------------------------------------------------
// qsgd_compressor.py:50-51: x = |v / norm| * s, the IEEE division.  (The quick form of the bucketed kernels is shared_quotient.)
__device__ __forceinline__ float qsgd_quotient(float v, float norm, float s) { return fabsf(v / norm) * s; }
// the operand window of the FAST form for a bucket norm and the smallest |v| of the lane's elements: shared_quotient needs
// 2^-80 <= norm / s <= 2^20 (s <= 2^16: hence the test of the norm at 2^-64) and every |v| >= 2^-102 (gq_common.hpp).  A lane that holds an exact zero next to non-zero
// elements takes the division: rare outside all-zero buckets, whose norm is outside the window anyway.
__device__ __forceinline__ bool quotient_window(float norm, float min_abs) {
    return norm >= 0x1p-64f && norm <= 0x1p20f && min_abs >= 0x1p-102f;
}
// qsgd_compressor.py:52-61 for a quotient x that is not NaN: clamp, truncate, stochastic round up.  `u` is only called when `draw`.
// LOWER = false: the caller knows x >= 0.
template <bool LOWER = true, class Draw>
__device__ __forceinline__ unsigned qsgd_level(float x, float smax, bool draw, Draw &&u) {
    const float c = LOWER ? fminf(fmaxf(x, 0.0f), smax) : fminf(x, smax);
    unsigned l = (unsigned)(int)c;
    if (draw) {
        const float prob = x - (float)l;
        l += (prob > u()) ? 1u : 0u;
    }
    return l;
}
// One element's wire code from v and its scaled quotient x (qsgd_quotient, or FAST: shared_quotient): the level with the sign above it.
// FAST: x = RN(|v| / norm) * s from the bucket's ONE reciprocal by Markstein's correction (shared_quotient: the correctly rounded
// quotient, bit for bit what v_div_* gives, in three operations instead of ~11) -- taken of |v| and norm / s with the reciprocal
// y * s: s is a power of two, so RN(|v| / (norm / s)) IS RN(|v| / norm) * s and the multiplication by s goes too.  The caller has
// checked the operand window (quotient_window) for every element of the lane; then no NaN can occur and the quotient is >= 0:
// the NaN test and the lower clamp go as well.  The sign bit is clamp(bits(v), 0, 1) (v is finite there: > 0 iff its bits, as a
// signed integer, are).
// RND: 1 / 0 = the caller has tested the mode once for all of a lane's elements, -1 = `draws` says so here.
template <bool FAST, int RND = -1, class Draw>
__device__ __forceinline__ unsigned qsgd_code(float v, float x, float smax, bool draws, Draw &&u, int bits) {
    unsigned l = 0, sgn;
    if constexpr (FAST) {
        // (as inline asm: the compiler turns min(max(bits, 0), 1) back into v_cmp + v_cndmask + v_or through VCC, with the
        // wait states gfx950 wants between a VALU write of VCC and its VALU read)
        asm("v_med3_i32 %0, %1, 0, 1" : "=v"(sgn) : "v"(__float_as_uint(v)));
    } else {
        sgn = v > 0.0f ? 1u : 0u;
    }
    if (!FAST && x != x) {
        // NaN (a zero bucket's 0 / 0, a NaN norm): the reference's cast makes it INT_MIN, a NEGATIVE level, and decodes
        // (-2^31) (2 sign - 1) norm / s (qsgd_compressor.py:53,69-70) -- for a zero bucket (-2^31)(-1)(0) = +0.  The wire's level
        // is 0 and the level's sign goes into the sign bit: a zero bucket decodes to +0 too (round 5 wrote sign 0: -0, which
        // only a bit-for-bit comparison of a PLAIN decode sees -- the aggregate starts from +0).
        sgn ^= 1u;
    } else {
        l = qsgd_level<!FAST>(x, smax, RND == 1 || (RND == -1 && draws), u);
    }
    return l | (sgn << (bits - 1));
}

// ---- the de-quantiser -------------------------------------------------------------------------------------------------------------
// qsgd_compressor.py:69-70, (l * (2 sign - 1)) * norm / s, every step rounded on its own, as  ((+-l) * norm) * inv_s  with the sign
// put on the float's sign bit and inv_s = 1 / s.  The same bits for every input: l * (-1) = -l and 0 * (-1) = -0 exactly, so the
// first product IS the level with its sign bit set (a level 0 with a clear sign bit decodes to -0); and s = 2^n_bit, so for the
// rounded product p both p / s and p * inv_s are ONE correct rounding of the same exact real p * 2^-n_bit -- inv_s itself is exact,
// and that holds where the result is subnormal too (the real is rounded once onto the 2^-149 grid either way), for inf and for NaN.
__device__ __forceinline__ float qsgd_signed_level(unsigned level, unsigned negative) {
    return __uint_as_float(__float_as_uint((float)level) | (negative << 31));
}
__device__ __forceinline__ float qsgd_scale(float signed_level, float norm, float inv_s) {
    const float t = signed_level * norm;
    return t * inv_s;
}
// a code c < 2^bits (sign bit 1: positive)
__device__ __forceinline__ float qsgd_dequant(unsigned c, int bits, float norm, float inv_s) {
    return qsgd_scale(qsgd_signed_level(c & ((1u << (bits - 1)) - 1u), (c >> (bits - 1)) ^ 1u), norm, inv_s);
}

// ---- units of 8 codes (BITS / 4 dwords, codes in ascending element order from the low end) and pairs ------------------------------
template <int BITS>
__device__ __forceinline__ void store_unit(uint8_t *dst, const unsigned (&code)[8]) {
    if constexpr (BITS == 4) {
        unsigned word = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) word |= code[k] << (4 * k);
        *reinterpret_cast<unsigned *>(dst) = word;
    } else if constexpr (BITS == 8) {
        *reinterpret_cast<uint2 *>(dst) = make_uint2(code[0] | (code[1] << 8) | (code[2] << 16) | (code[3] << 24),
                                                     code[4] | (code[5] << 8) | (code[6] << 16) | (code[7] << 24));
    } else {
        *reinterpret_cast<uint4 *>(dst) = make_uint4(code[0] | (code[1] << 16), code[2] | (code[3] << 16),
                                                     code[4] | (code[5] << 16), code[6] | (code[7] << 16));
    }
}
template <int BITS>
__device__ __forceinline__ void load_unit(gbyte_ptr p, unsigned (&w)[BITS / 4]) {
    if constexpr (BITS == 4) {
        w[0] = *(const unsigned __attribute__((address_space(1))) *)p;
    } else if constexpr (BITS == 8) {
        const uv2 v = *(const uv2 __attribute__((address_space(1))) *)p;
        w[0] = v[0];
        w[1] = v[1];
    } else {
        const uv4 v = *(const uv4 __attribute__((address_space(1))) *)p;
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = v[i];
    }
}
// (+-level) of code k of a unit, straight from the unit's dwords `w` and their complements `nw` (two bit-field extracts per element)
template <int BITS>
__device__ __forceinline__ float unit_signed_level(const unsigned (&w)[BITS / 4], const unsigned (&nw)[BITS / 4], int k) {
    constexpr int PER = 32 / BITS;   // codes per dword
    const int word = k / PER, sh = BITS * (k % PER);
    return qsgd_signed_level((w[word] >> sh) & ((1u << (BITS - 1)) - 1u), (nw[word] >> (sh + BITS - 1)) & 1u);
}
// the codes of elements e, e + 1 (e even) of a section sit pair_at(e, bits) bytes into it: one byte, two, or a dword
__device__ __forceinline__ int pair_at(int e, int bits) { return (e * bits) >> 3; }
__device__ __forceinline__ void store_pair(uint8_t *pair, int bits, unsigned c0, unsigned c1) {
    if (bits == 4) {
        *pair = (uint8_t)(c0 | (c1 << 4));
    } else if (bits == 8) {
        *reinterpret_cast<uchar2 *>(pair) = make_uchar2((uint8_t)c0, (uint8_t)c1);
    } else {
        *reinterpret_cast<unsigned *>(pair) = c0 | (c1 << 16);
    }
}
__device__ __forceinline__ void load_pair(const uint8_t *pair, int bits, unsigned &c0, unsigned &c1) {
    if (bits == 4) {
        const unsigned byte = *pair;
        c0 = byte & 15u;
        c1 = byte >> 4;
    } else if (bits == 8) {
        const uchar2 cc = *reinterpret_cast<const uchar2 *>(pair);
        c0 = cc.x;
        c1 = cc.y;
    } else {
        const unsigned cc = *reinterpret_cast<const unsigned *>(pair);
        c0 = cc & 0xFFFFu;
        c1 = cc >> 16;
    }
}

// ---- a bucket walked by a team of `lanes` lanes (a power of two inside one wave), this one being `lane` --------------------------
// compress, an element pair per lane and trip, the bucket read twice.  EF: error feedback fused around the codec
// (ps_quantizer.py:35-39): the bucket is read as v = grad + ef_scale * error (product rounded, then the add), v is written back over
// grad, and error = v - decode(code) replaces the old error -- all in this one pass.  err: the bucket's error, or null.
template <bool EF>
__device__ __forceinline__ void qsgd_compress_pair_walk(int lanes, int lane, gf_ptr v, gf_ptr err, int d, float ef_scale, int64_t b,
                                                        int bits, int n_bit, int random_mode, uint64_t seed, float *norm_dst, uint8_t *dst) {
    const float s = (float)(1 << n_bit), smax = s - 1.0f, inv_s = 1.0f / s;
    auto load = [&](int e) {
        v2f p = *(gf2_ptr)(v + e);
        if (EF && err) {
            const v2f q = *(gf2_ptr)(err + e);
            const float p0 = ef_scale * q[0], p1 = ef_scale * q[1];
            p[0] = p[0] + p0;
            p[1] = p[1] + p1;
        }
        return p;
    };
    float mx = 0.0f;
    for (int e = 2 * lane; e < d; e += 2 * lanes) {
        const v2f p = load(e);
        mx = absmax3_nan(mx, p[0], p[1]);   // NaN-propagating, like torch.max (qsgd_compressor.py:49)
    }
#pragma unroll
    for (int o = lanes / 2; o > 0; o >>= 1) mx = max_nan(mx, __shfl_xor(mx, o, 64));
    if (lane == 0) *norm_dst = mx;
    const uint64_t sd = random_mode == GQ_RANDOM_DEVICE_KEYED ? keyed_seed(seed, mx, mx) : seed;   // keyed by the bucket's norm
    const uint32_t key = bucket_draw_key(sd, b);   // the draws' stream of this bucket (element index inside the bucket)
    const bool draws = random_mode >= GQ_RANDOM_DEVICE;   // DEVICE, or DEVICE_KEYED with the bucket's keyed seed
    for (int e = 2 * lane; e < d; e += 2 * lanes) {
        const v2f p = load(e);
        const unsigned c0 = qsgd_code<false>(p[0], qsgd_quotient(p[0], mx, s), smax, draws, [&] { return bucket_draw(key, (uint32_t)e); }, bits);
        const unsigned c1 = qsgd_code<false>(p[1], qsgd_quotient(p[1], mx, s), smax, draws, [&] { return bucket_draw(key, (uint32_t)e + 1u); }, bits);
        store_pair(dst + pair_at(e, bits), bits, c0, c1);
        if (EF && err) {   // this element's own code decoded, then ps_quantizer.py:39
            *(gf2_ptr)(v + e) = p;
            *(gf2_ptr)(err + e) = v2f{p[0] - qsgd_dequant(c0, bits, mx, inv_s), p[1] - qsgd_dequant(c1, bits, mx, inv_s)};
        }
    }
}

// decode + mean of R payloads, payloads in ascending order: `codes` = byte offset of the bucket's codes inside a payload (Off: 32 bits
// where the caller knows that they do), norm_of(payload) = the bucket's norm there, o = the bucket's output.  An element pair per lane and trip ...
template <class NormOf, class Off>
__device__ __forceinline__ void qsgd_decode_pair_walk(int lanes, int lane, int d, int bits, const uint8_t *gathered, int64_t user_stride,
                                                      int R, NormOf &&norm_of, Off codes, float inv_s, const MeanDiv &md, float *o) {
    for (int e = 2 * lane; e < d; e += 2 * lanes) {
        float a0 = 0.0f, a1 = 0.0f;
        for (int r = 0; r < R; ++r) {
            const uint8_t *p = gathered + (int64_t)r * user_stride;
            const float norm = norm_of(p);
            unsigned c0, c1;
            load_pair(p + (codes + (Off)pair_at(e, bits)), bits, c0, c1);   // (one offset for every payload)
            const float t0 = qsgd_dequant(c0, bits, norm, inv_s), t1 = qsgd_dequant(c1, bits, norm, inv_s);
            a0 = (r == 0) ? t0 : a0 + t0;
            a1 = (r == 0) ? t1 : a1 + t1;
        }
        if (md.apply) {
            a0 = mean_div(a0, md);
            a1 = mean_div(a1, md);
        }
        *reinterpret_cast<float2 *>(o + e) = make_float2(a0, a1);
    }
}
// ... and a whole unit of 8 elements (d % 8 == 0; 32 contiguous bytes stored), units `first`, first + lanes, ... counted from where
// `codes` and `o` point (the bucket's start, or a lane's own first unit with d counted from there); norm_at = byte offset of the
// bucket's norm (an aligned word) inside a payload
template <int BITS, class Off>
__device__ __forceinline__ void qsgd_decode_unit_walk(int lanes, int first, int d, const uint8_t *gathered, int64_t user_stride, int R,
                                                      Off norm_at, Off codes, float inv_s, const MeanDiv &md, float *o) {
    for (int c = first; 8 * c < d; c += lanes) {
        f32x4 acc[2];
        for (int r = 0; r < R; ++r) {
            const uint8_t *p = gathered + (int64_t)r * user_stride;
            const float norm = *reinterpret_cast<const float *>(p + norm_at);
            unsigned w[BITS / 4], nw[BITS / 4];
            load_unit<BITS>((gbyte_ptr)(p + codes + BITS * c), w);
#pragma unroll
            for (int i = 0; i < BITS / 4; ++i) nw[i] = ~w[i];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float t = qsgd_scale(unit_signed_level<BITS>(w, nw, k), norm, inv_s);
                acc[k >> 2][k & 3] = r == 0 ? t : acc[k >> 2][k & 3] + t;
            }
        }
        if (md.apply) {
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[k >> 2][k & 3] = mean_div(acc[k >> 2][k & 3], md);
        }
        *reinterpret_cast<f32x4 *>(o + 8 * c) = acc[0];
        *reinterpret_cast<f32x4 *>(o + 8 * c + 4) = acc[1];
    }
}

// ---- host: what the multi-tensor launchers refuse (bucketed and wide alike; `what` names the entry point) ------------------------
// compress: -> GQ_OK and the code width, or the refusal
static inline int qsgd_compress_check(const char *what, bool pointers, int nseg, int64_t nitems, int n_bit, int random_mode, int *bits) {
    if (nseg < 1 || nitems < 1 || n_bit < 1) return fail(GQ_ERR_INVALID_ARG, "%s: bad sizes", what);
    if (!pointers) return fail(GQ_ERR_INVALID_ARG, "%s: null pointer", what);
    if (random_mode != GQ_RANDOM_OFF && random_mode != GQ_RANDOM_DEVICE && random_mode != GQ_RANDOM_DEVICE_KEYED &&
        random_mode != GQ_RANDOM_DEVICE_COUNTER)
        return fail(GQ_ERR_UNSUPPORTED, "%s: random_mode must be OFF, DEVICE, DEVICE_KEYED or DEVICE_COUNTER", what);
    *bits = gq_qsgd_code_bits(n_bit, random_mode);
    if (!*bits) return fail(GQ_ERR_UNSUPPORTED, "%s: n_bit %d has no packed format", what, n_bit);
    return GQ_OK;
}
static inline int qsgd_decode_check(const char *what, bool pointers, int nseg, int64_t nitems, int n_bit, int bits, int R) {
    if (nseg < 1 || nitems < 1 || n_bit < 1 || R < 1 || (bits != 4 && bits != 8 && bits != 16))
        return fail(GQ_ERR_INVALID_ARG, "%s: bad sizes", what);
    if (!pointers) return fail(GQ_ERR_INVALID_ARG, "%s: null pointer", what);
    return GQ_OK;
}

}  // namespace gq
