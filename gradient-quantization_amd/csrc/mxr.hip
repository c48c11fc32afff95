// The microscaling compressor behind a randomized Hadamard rotation, multi-tensor (segment table) form -- libgq_mxr.so
// (include/gq_mxr.h: the contract, to the bit; tests/mxr_contract.py restates it in numpy).
//
// The kernels and the host path are csrc/mx_kernels.hpp's, shared with mx.hip; this file is the rotation -- the policy the kernels
// are instantiated with, and what it calls -- the descriptor and the exported names.
// The kernels' shape: one workgroup per item of GQ_MX_ITEM_ELEMS elements, two steps of 2048, a lane owns eight
// consecutive elements and a quad an MX block.  32 lanes therefore own a rotation block of 256: the 256-point Walsh-Hadamard
// transform is three butterfly stages inside the lane (strides 1, 2, 4) and five across lanes (strides 8 ... 128 = lane xor
// 1, 2, 4, 8, 16), which never leave a 32-lane half -- DPP quad permutes for xor 1 and 2, ds_swizzle (its 32-lane bit mode)
// for the rest.  No LDS is allocated, no barrier, no scratch, no extra pass over memory.  In a cross-lane stage the lane with
// the stage's bit clear computes mine + other and its partner other - mine; both are  other + (+-mine), one addition.
// Whether a half is rotated (block start + 256 <= n) is uniform over that half; every lane executes the exchanges and selects
// afterwards, so no exchange sits under divergent control flow.
// compress  load (+ error feedback) -> sign flip -> 8 stages -> * 2^-4 -> the exponent / code / store path; if `out` or
//           error feedback is asked for: decode -> 8 stages -> * 2^-4 -> sign flip -> out / w / err = w - D.
// decode    the accumulation over the R payloads and the division, then ONE inverse transform, then the store.
// A lane's eight sign bits are one byte of the descriptor's sign words (passed by value), extracted once per kernel.
#include "gq_mxr.h"
#include "mx_common.hpp"
#include "mx_kernels.hpp"

#define GQXR_API extern "C" __attribute__((visibility("default")))

namespace gqx {

static_assert(GQ_MXR_BLOCK == 32 * PER_LANE && STEP % GQ_MXR_BLOCK == 0, "a 32-lane half owns a rotation block");
static_assert(sizeof(gq_mxr_batch) == 80, "gq_mxr_batch: the layout the ctypes binding declares (gq_amd/native.py)");

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
__device__ __forceinline__ void cross_stage(float (&x)[PER_LANE]) {
    const uint32_t neg = (threadIdx.x & M) ? 0x80000000u : 0u;
#pragma unroll
    for (int k = 0; k < PER_LANE; ++k) {
        const float other = lane_xor<M>(x[k]);
        x[k] = other + __uint_as_float(__float_as_uint(x[k]) ^ neg);
    }
}

// the eight stages t = 0 ... 7 in this order, then * 2^-4 (include/gq_mxr.h)
__device__ __forceinline__ void stages_and_scale(float (&x)[PER_LANE]) {
#pragma unroll
    for (int h = 1; h < PER_LANE; h <<= 1) {
#pragma unroll
        for (int j = 0; j < PER_LANE; ++j) {
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
    for (int k = 0; k < PER_LANE; ++k) x[k] = x[k] * 0.0625f;
}

__device__ __forceinline__ float flip(float v, uint32_t sbyte, int k) { return __uint_as_float(__float_as_uint(v) ^ (((sbyte >> k) & 1u) << 31)); }

// The rotation policy of csrc/mx_kernels.hpp: blocks of 256 by H * diag(signs) / 16; it carries the lane's sign byte.
struct Hadamard {
    using Args = Signs;
    static constexpr int BLOCK = GQ_MXR_BLOCK;    // a 32-lane half owns one: `rot` is uniform over the half
    static constexpr bool EVERY_LANE = true;      // the cross-lane stages: every lane executes them and selects afterwards
    uint32_t sbyte;
    __device__ __forceinline__ explicit Hadamard(const Signs &s) : sbyte(sign_byte(s)) {}
    // w -> x' (rot; otherwise x' = w)
    __device__ __forceinline__ const Lane8 &forward(const Lane8 &w, Lane8 &x, bool rot) const {
#pragma unroll
        for (int k = 0; k < PER_LANE; ++k) x[k] = flip(w[k], sbyte, k);
        stages_and_scale(x);
#pragma unroll
        for (int k = 0; k < PER_LANE; ++k) x[k] = rot ? x[k] : w[k];
        return x;
    }
    // y -> its inverse transform, in place
    __device__ __forceinline__ void inverse(Lane8 &y, bool rot) const {
        float t[PER_LANE];
#pragma unroll
        for (int k = 0; k < PER_LANE; ++k) t[k] = y[k];
        stages_and_scale(t);
#pragma unroll
        for (int k = 0; k < PER_LANE; ++k) y[k] = rot ? flip(t[k], sbyte, k) : y[k];
    }
    static Args args(const gq_mxr_batch *b) { return Signs{{b->signs[0], b->signs[1], b->signs[2], b->signs[3]}}; }
};

}  // namespace gqx

GQXR_API int gq_mxr_abi_version(void) { return GQ_MXR_ABI_VERSION; }

GQXR_API const char *gq_mxr_last_error(void) { return gqx::err_buf; }

GQXR_API int gq_mxr_compress_batched(const gq_mxr_batch *b, uint8_t *wire, int random_mode, const float *r, uint64_t seed, float ef_scale,
                                     float *out, void *stream) {
    return gqx::compress_batched<gqx::Hadamard, gqx::TT_F32>("gq_mxr_compress_batched", b, wire, random_mode, r, seed, ef_scale, out, stream);
}

GQXR_API int gq_mxr_decode_sum_batched(const gq_mxr_batch *b, const uint8_t *gathered, int64_t user_stride_bytes, int R, float *out, int plain,
                                       void *stream) {
    return gqx::decode_sum_batched<gqx::Hadamard, gqx::TT_F32>("gq_mxr_decode_sum_batched", b, gathered, user_stride_bytes, R, out, plain, stream);
}

// the same launches over bf16 sources, `out` and dense-copy sources (include/gq_mxr.h, TENSOR-SIDE TYPE); the wire is the f32 twin's
GQXR_API int gq_mxr_compress_batched_bf16(const gq_mxr_batch *b, uint8_t *wire, int random_mode, const float *r, uint64_t seed, float ef_scale,
                                          uint16_t *out, void *stream) {
    return gqx::compress_batched<gqx::Hadamard, gqx::TT_BF16>("gq_mxr_compress_batched_bf16", b, wire, random_mode, r, seed, ef_scale, out, stream);
}

GQXR_API int gq_mxr_decode_sum_batched_bf16(const gq_mxr_batch *b, const uint8_t *gathered, int64_t user_stride_bytes, int R, uint16_t *out,
                                            int plain, void *stream) {
    return gqx::decode_sum_batched<gqx::Hadamard, gqx::TT_BF16>("gq_mxr_decode_sum_batched_bf16", b, gathered, user_stride_bytes, R, out, plain, stream);
}
