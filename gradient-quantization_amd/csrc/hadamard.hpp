// The 256-point randomized Hadamard rotation libgq_mxr.so (mxr.hip), libgq_drive.so (drive.hip) and libgq_eden.so (eden.hip) share, in registers
// (include/gq_mxr.h: the transform, to the bit).  Internal linkage: each library compiles its own copy.
// A lane owns eight consecutive elements, so 32 lanes own a rotation block of 256: the Walsh-Hadamard transform is three
// butterfly stages inside the lane (strides 1, 2, 4) and five across lanes (strides 8 ... 128 = lane xor 1, 2, 4, 8, 16), which
// never leave a 32-lane half -- DPP quad permutes for xor 1 and 2, ds_swizzle (its 32-lane bit mode) for the rest.  No LDS is
// allocated, no barrier, no scratch.  In a cross-lane stage the lane with the stage's bit clear computes mine + other and its
// partner other - mine; both are  other + (+-mine), one addition.  Every lane of a wave must execute the exchanges: a caller
// selects afterwards and keeps them out of divergent control flow.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gqx {

constexpr int HAD_PER_LANE = 8;                       // elements of a lane
constexpr int HAD_BLOCK = 32 * HAD_PER_LANE;          // elements of a rotation block: a 32-lane half owns one
using HadLane = float[HAD_PER_LANE];

struct Signs {
    uint64_t w[4];
};

// this lane's byte of the sign words: bit k belongs to its element k (element j of the block: bit j & 63 of word j >> 6)
__device__ __forceinline__ uint32_t sign_byte(const Signs &s) {
    const uint32_t l = threadIdx.x & 31u;
    const uint32_t q = l >> 3;
    const uint64_t word = q == 0 ? s.w[0] : q == 1 ? s.w[1] : q == 2 ? s.w[2] : s.w[3];      // (selects: no indexed kernel argument)
    return (uint32_t)(word >> (8 * (l & 7u))) & 0xffu;
}

// A lane's sign byte, ready made (stepped_sign_byte below): what Hadamard is built from when the words are not a launch argument.
struct SignByte {
    uint32_t v;
};

// the splitmix64 finaliser: the two multiplications and the three xor-shifts
__device__ __forceinline__ uint64_t splitmix_fin(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// SIGNS, STEPPED (include/gq_drive.h, include/gq_eden.h): word k of the launch at (seed, step) is output 4 * step + k of the
// splitmix64 stream started at seed.  A lane needs the word of its quarter only: one finaliser (two 64-bit multiplications) and
// the lane's byte.
__device__ __forceinline__ SignByte stepped_sign_byte(uint64_t seed, uint64_t step) {
    constexpr uint64_t G = 0x9E3779B97F4A7C15ull;
    const uint32_t l = threadIdx.x & 31u;
    const uint32_t q = l >> 3;
    const uint64_t first = seed + (4 * step + 1) * G;      // (uniform; all of it mod 2^64)
    const uint64_t z = splitmix_fin(first + (q == 0 ? 0 : q == 1 ? G : q == 2 ? 2 * G : 3 * G));
    return SignByte{(uint32_t)(z >> (8 * (l & 7u))) & 0xffu};
}

// `rotation` is a device { seed, step } pair: one plain wave-uniform read.  Once per launch: a caller keeps this out of its item loop.
__device__ __forceinline__ SignByte stepped_sign_byte(const uint64_t *__restrict__ rotation) {
    return stepped_sign_byte(rotation[0], rotation[1]);
}

// what a stepped launch takes in the place of Signs: the pair's address, which never changes
struct Stepped {
    const uint64_t *pair;
};

// SIGNS, PER STREAM (include/gq_drive.h, include/gq_eden.h): the seed of stream sigma >= 0.  Stream 0 keeps the seed, so its words
// are the stepped ones bit for bit; any other stream's seed is one 64-bit multiply-add and one finaliser away, all of it on values
// that are uniform over the workgroup.
__device__ __forceinline__ uint64_t stream_seed(uint64_t seed, uint32_t sigma) {
    const uint64_t mixed = splitmix_fin(seed + (uint64_t)sigma * 0xD6E8FEB86659FD93ull);
    return sigma == 0 ? seed : mixed;
}

// the lane's sign byte of stream sigma at (seed, step): the stepped byte of (seed_sigma, step)
__device__ __forceinline__ SignByte stream_sign_byte(uint64_t seed, uint64_t step, uint32_t sigma) {
    return stepped_sign_byte(stream_seed(seed, sigma), step);
}

// what a compress under one stream takes: the pair's address and the stream, by value (a function of the wire slot)
struct Streamed {
    const uint64_t *pair;
    uint32_t sigma;
};

// the value of lane ^ M, M = 1, 2, 4, 8 or 16 (all inside a 32-lane half)
template <int M>
__device__ __forceinline__ float lane_xor(float v) {
    const int x = __float_as_int(v);
    if (M == 1) return __int_as_float(__builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, true));      // quad_perm [1, 0, 3, 2]
    if (M == 2) return __int_as_float(__builtin_amdgcn_update_dpp(0, x, 0x4E, 0xF, 0xF, true));      // quad_perm [2, 3, 0, 1]
    return __int_as_float(__builtin_amdgcn_ds_swizzle(x, (M << 10) | 0x1F));                         // bit mode: and 0x1f, or 0, xor M
}

// one cross-lane stage, stride 8 M: the lane with bit M clear takes mine + other, its partner other - mine
template <int M>
__device__ __forceinline__ void cross_stage(float (&x)[HAD_PER_LANE]) {
    const uint32_t neg = (threadIdx.x & M) ? 0x80000000u : 0u;
#pragma unroll
    for (int k = 0; k < HAD_PER_LANE; ++k) {
        const float other = lane_xor<M>(x[k]);
        x[k] = other + __uint_as_float(__float_as_uint(x[k]) ^ neg);
    }
}

// the eight stages t = 0 ... 7 in this order, then * 2^-4 (include/gq_mxr.h)
__device__ __forceinline__ void stages_and_scale(float (&x)[HAD_PER_LANE]) {
#pragma unroll
    for (int h = 1; h < HAD_PER_LANE; h <<= 1) {
#pragma unroll
        for (int j = 0; j < HAD_PER_LANE; ++j) {
            if (!(j & h)) {
                const float a = x[j], b = x[j + h];
                x[j] = a + b;
                x[j + h] = a - b;
            }
        }
    }
    cross_stage<1>(x);
    cross_stage<2>(x);
    cross_stage<4>(x);
    cross_stage<8>(x);
    cross_stage<16>(x);
#pragma unroll
    for (int k = 0; k < HAD_PER_LANE; ++k) x[k] = x[k] * 0.0625f;
}

__device__ __forceinline__ float flip(float v, uint32_t sbyte, int k) { return __uint_as_float(__float_as_uint(v) ^ (((sbyte >> k) & 1u) << 31)); }

// The rotation by H * diag(signs) / 16 over blocks of 256, as the policy csrc/mx_kernels.hpp asks for (csrc/rotq_kernels.hpp calls forward
// and inverse with rot = true: its blocks are zero-padded, every one is rotated); it carries the lane's sign byte.
struct Hadamard {
    using Args = Signs;
    static constexpr int BLOCK = HAD_BLOCK;       // a 32-lane half owns one: `rot` is uniform over the half
    static constexpr bool EVERY_LANE = true;      // the cross-lane stages: every lane executes them and selects afterwards
    uint32_t sbyte;
    __device__ __forceinline__ explicit Hadamard(const Signs &s) : sbyte(sign_byte(s)) {}
    __device__ __forceinline__ explicit Hadamard(const SignByte &b) : sbyte(b.v) {}
    __device__ __forceinline__ explicit Hadamard(const Stepped &r) : Hadamard(stepped_sign_byte(r.pair)) {}      // (csrc/rotq_kernels.hpp)
    __device__ __forceinline__ explicit Hadamard(const Streamed &r) : Hadamard(stream_sign_byte(r.pair[0], r.pair[1], r.sigma)) {}
    // w -> x' (rot; otherwise x' = w)
    __device__ __forceinline__ const HadLane &forward(const HadLane &w, HadLane &x, bool rot) const {
#pragma unroll
        for (int k = 0; k < HAD_PER_LANE; ++k) x[k] = flip(w[k], sbyte, k);
        stages_and_scale(x);
#pragma unroll
        for (int k = 0; k < HAD_PER_LANE; ++k) x[k] = rot ? x[k] : w[k];
        return x;
    }
    // y -> its inverse transform, in place
    __device__ __forceinline__ void inverse(HadLane &y, bool rot) const {
        float t[HAD_PER_LANE];
#pragma unroll
        for (int k = 0; k < HAD_PER_LANE; ++k) t[k] = y[k];
        stages_and_scale(t);
#pragma unroll
        for (int k = 0; k < HAD_PER_LANE; ++k) y[k] = rot ? flip(t[k], sbyte, k) : y[k];
    }
    // host: the sign words of a descriptor that ends with them (gq_mxr_batch, gq_drive_batch)
    template <class B>
    static Args args(const B *b) {
        return Signs{{b->signs[0], b->signs[1], b->signs[2], b->signs[3]}};
    }
};

}  // namespace gqx
