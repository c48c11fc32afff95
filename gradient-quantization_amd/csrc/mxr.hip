// The microscaling compressor behind a randomized Hadamard rotation, multi-tensor (segment table) form -- libgq_mxr.so
// (include/gq_mxr.h: the contract, to the bit; tests/mxr_contract.py restates it in numpy).
//
// The kernels keep mx.hip's shape: one workgroup per item of GQ_MX_ITEM_ELEMS elements, two steps of 2048, a lane owns eight
// consecutive elements and a quad an MX block.  32 lanes therefore own a rotation block of 256: the 256-point Walsh-Hadamard
// transform is three butterfly stages inside the lane (strides 1, 2, 4) and five across lanes (strides 8 ... 128 = lane xor
// 1, 2, 4, 8, 16), which never leave a 32-lane half -- DPP quad permutes for xor 1 and 2, ds_swizzle (its 32-lane bit mode)
// for the rest.  No LDS is allocated, no barrier, no scratch, no extra pass over memory.  In a cross-lane stage the lane with
// the stage's bit clear computes mine + other and its partner other - mine; both are  other + (+-mine), one addition.
// Whether a half is rotated (block start + 256 <= n) is uniform over that half; every lane executes the exchanges and selects
// afterwards, so no exchange sits under divergent control flow.
// compress  load (+ error feedback) -> sign flip -> 8 stages -> * 2^-4 -> mx.hip's exponent / code / store path; if `out` or
//           error feedback is asked for: decode -> 8 stages -> * 2^-4 -> sign flip -> out / w / err = w - D.
// decode    mx.hip's accumulation over the R payloads and the division, then ONE inverse transform, then the store.
// A lane's eight sign bits are one byte of the descriptor's sign words (passed by value), extracted once per kernel.
#include <math.h>

#include "gq_common.hpp"
#include "gq_lib_prelude.hpp"
#include "gq_mxr.h"
#include "mx_common.hpp"

#define GQXR_API extern "C" __attribute__((visibility("default")))

namespace gqx {

constexpr int THREADS = 256;
constexpr int PER_LANE = 8;                           // elements of a lane: a quad owns an MX block, 32 lanes a rotation block
constexpr int STEP = THREADS * PER_LANE;              // elements of a workgroup-wide step
constexpr int STEPS = GQ_MX_ITEM_ELEMS / STEP;
static_assert(GQ_MX_BLOCK == 4 * PER_LANE, "a quad owns a block");
static_assert(GQ_MXR_BLOCK == 32 * PER_LANE && STEP % GQ_MXR_BLOCK == 0, "a 32-lane half owns a rotation block");
static_assert(GQ_MX_ITEM_ELEMS % STEP == 0 && GQ_MX_ITEM_ELEMS % (16 * GQ_MX_BLOCK) == 0, "an item is whole steps and whole 16-byte runs of scale bytes");
static_assert(sizeof(gq_mxr_batch) == 80, "gq_mxr_batch: the layout the ctypes binding declares (gq_amd/native.py)");

using gql::aligned16;
using gql::copy_dense;
using gql::err_buf;
using gql::fail;

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

// w -> x' (rot: this lane's half is a rotated block; otherwise x' = w)
__device__ __forceinline__ void forward(const float (&w)[PER_LANE], float (&x)[PER_LANE], uint32_t sbyte, bool rot) {
#pragma unroll
    for (int k = 0; k < PER_LANE; ++k) x[k] = flip(w[k], sbyte, k);
    stages_and_scale(x);
#pragma unroll
    for (int k = 0; k < PER_LANE; ++k) x[k] = rot ? x[k] : w[k];
}

// y -> its inverse transform, in place
__device__ __forceinline__ void inverse(float (&y)[PER_LANE], uint32_t sbyte, bool rot) {
    float t[PER_LANE];
#pragma unroll
    for (int k = 0; k < PER_LANE; ++k) t[k] = y[k];
    stages_and_scale(t);
#pragma unroll
    for (int k = 0; k < PER_LANE; ++k) y[k] = rot ? flip(t[k], sbyte, k) : y[k];
}

template <int FMT, int MODE, bool EF, int TT>
__global__ __launch_bounds__(THREADS) void mxr_compress_kernel(const int64_t *__restrict__ seg_table, const int32_t *__restrict__ item_seg,
                                                               uint8_t *__restrict__ wire, typename Tensor<TT>::type *__restrict__ out, float ef_scale,
                                                               int random_mode, const float *__restrict__ rbuf, uint64_t seed,
                                                               const int64_t *__restrict__ dense_table, int ndense, Signs signs) {
    using F = Fmt<FMT>;
    using T = typename Tensor<TT>::type;
    if (MODE == DRAW_DEVICE) gq::resolve_seed(random_mode, seed);
    if (TT == TT_F32)
        copy_dense<THREADS>(dense_table, ndense, wire);
    else
        copy_dense_as_f32<THREADS, T>(dense_table, ndense, wire);
    const int64_t item = blockIdx.x;
    const int seg = item_seg[item];
    const int64_t *rec = seg_table + 8 * (int64_t)seg;
    const int64_t n = rec[1];
    const int64_t nb = (n + GQ_MX_BLOCK - 1) / GQ_MX_BLOCK, nb_pad = up16(nb);
    T *v = reinterpret_cast<T *>(rec[0]);
    float *err = EF ? reinterpret_cast<float *>(rec[7]) : nullptr;
    uint8_t *scales = wire + rec[3];
    uint8_t *codes = scales + nb_pad;
    T *o = out ? out + rec[5] : nullptr;
    const int64_t first_draw = rec[6];
    const int lane = threadIdx.x & 63;
    const uint32_t sbyte = sign_byte(signs);
    const int64_t base = (item - rec[2]) * GQ_MX_ITEM_ELEMS;
    for (int s = 0; s < STEPS; ++s) {
        if (base + (int64_t)s * STEP >= nb_pad * GQ_MX_BLOCK) break;      // (uniform over the workgroup)
        const int64_t e0 = base + (int64_t)s * STEP + (int64_t)threadIdx.x * PER_LANE;      // this lane's first element
        const bool rot = (e0 & ~(int64_t)(GQ_MXR_BLOCK - 1)) + GQ_MXR_BLOCK <= n;           // (uniform over the 32-lane half)
        float w[PER_LANE];
#pragma unroll
        for (int k = 0; k < PER_LANE; ++k) w[k] = 0.0f;
        const bool ef = EF && err;
        const bool full = e0 + PER_LANE - 1 < n && aligned16(v + e0) && (!ef || aligned16(err + e0));
        if (full) {
            load8(v + e0, w);
            if (ef) {
                float rr[PER_LANE];
                load8(err + e0, rr);
#pragma unroll
                for (int k = 0; k < PER_LANE; ++k) {
                    const float p = ef_scale * rr[k];      // (-ffp-contract=off: the product rounded, then the sum)
                    w[k] = w[k] + p;
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < PER_LANE; ++k) {
                if (e0 + k < n) {
                    w[k] = to_f32(v[e0 + k]);
                    if (ef) {
                        const float p = ef_scale * err[e0 + k];
                        w[k] = w[k] + p;
                    }
                }
            }
        }
        float x[PER_LANE];      // x': the rotated block, or the tail as it is
        forward(w, x, sbyte, rot);
        // from here to the stores: mx.hip's path over x'
        uint32_t a = 0;
#pragma unroll
        for (int k = 0; k < PER_LANE; ++k) a = max(a, __float_as_uint(x[k]) & 0x7fffffffu);
        a = max(a, (uint32_t)__shfl_xor((int)a, 1, 64));
        a = max(a, (uint32_t)__shfl_xor((int)a, 2, 64));
        const bool bad = a >= 0x7f800000u;      // an infinity or a NaN in the block
        const int e = block_exponent<F>(bad ? 0u : a);
        const uint32_t sb = bad ? 0xFFu : (uint32_t)(e + 127);

        uint32_t c[PER_LANE];
#pragma unroll
        for (int k = 0; k < PER_LANE; ++k) {
            float r = 0.0f;
            if (MODE == DRAW_GIVEN) r = e0 + k < n ? rbuf[first_draw + e0 + k] : 0.0f;
            if (MODE == DRAW_DEVICE) r = gq::uniform01(seed, (uint64_t)(first_draw + e0 + k));
            const uint32_t xb = __float_as_uint(x[k]);
            const uint32_t m = magnitude_code<F, MODE>(xb, e, r);
            c[k] = bad ? 0u : (m | ((xb >> 31) << (F::bits - 1)));
        }
        if (o || ef) {      // (uniform over the workgroup: the inverse transform's exchanges run in every lane)
            float d[PER_LANE];
#pragma unroll
            for (int k = 0; k < PER_LANE; ++k) d[k] = bad ? __uint_as_float(QNAN) : decode_value<F>(c[k], e);
            inverse(d, sbyte, rot);
            if (e0 < n) {
                const bool vec = e0 + PER_LANE - 1 < n;
                if (o) {
                    if (vec && aligned16(o + e0)) {
                        store8(o + e0, d);
                    } else {
                        for (int k = 0; k < PER_LANE && e0 + k < n; ++k) o[e0 + k] = from_f32<T>(d[k]);
                    }
                }
                if (ef) {      // the residual from the UNROUNDED w; only the copy stored back into the source is narrowed (T = bf16)
                    if (full) {
                        store8(v + e0, w);
                        *reinterpret_cast<float4 *>(err + e0) = make_float4(w[0] - d[0], w[1] - d[1], w[2] - d[2], w[3] - d[3]);
                        *reinterpret_cast<float4 *>(err + e0 + 4) = make_float4(w[4] - d[4], w[5] - d[5], w[6] - d[6], w[7] - d[7]);
                    } else {
                        for (int k = 0; k < PER_LANE && e0 + k < n; ++k) {
                            v[e0 + k] = from_f32<T>(w[k]);
                            err[e0 + k] = w[k] - d[k];
                        }
                    }
                }
            }
        }
        // the lane's codes: element 2i in the low nibble (FP4) / element i in byte i (FP8), little-endian words; FP6: the quad's
        // six dwords (store_codes6, + the pad behind an odd number of blocks)
        const int64_t blk = e0 / GQ_MX_BLOCK;
        if (F::bits == 6) {
            store_codes6(codes, blk, nb, c);
        } else if (blk < nb) {
            if (FMT == GQ_MX_FP4) {
                uint32_t word = 0;
#pragma unroll
                for (int k = 0; k < PER_LANE; ++k) word |= c[k] << (4 * k);
                reinterpret_cast<uint32_t *>(codes)[e0 / PER_LANE] = word;
            } else {
                const uint32_t lo = c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24);
                const uint32_t hi = c[4] | (c[5] << 8) | (c[6] << 16) | (c[7] << 24);
                reinterpret_cast<uint2 *>(codes)[e0 / PER_LANE] = make_uint2(lo, hi);
            }
        }
        // four quads' scale bytes -> one little-endian word (lanes 16j .. 16j+15 hold the blocks 4j .. 4j+3 of the step)
        uint32_t sw = sb << (8 * ((lane >> 2) & 3));
        sw |= (uint32_t)__shfl_xor((int)sw, 4, 64);
        sw |= (uint32_t)__shfl_xor((int)sw, 8, 64);
        if ((lane & 15) == 0 && blk < nb_pad) reinterpret_cast<uint32_t *>(scales)[blk >> 2] = sw;
    }
}

template <int FMT, int TT>
__global__ __launch_bounds__(THREADS) void mxr_decode_kernel(const int64_t *__restrict__ seg_table, const int32_t *__restrict__ item_seg,
                                                             const uint8_t *__restrict__ gathered, int64_t stride, int R,
                                                             typename Tensor<TT>::type *__restrict__ out, int plain, Signs signs) {
    using F = Fmt<FMT>;
    constexpr int CODE_BYTES = PER_LANE * F::bits / 8;      // a lane's code bytes: 4 (FP4), 6 (FP6) or 8 (FP8)
    const int64_t item = blockIdx.x;
    const int seg = item_seg[item];
    const int64_t *rec = seg_table + 8 * (int64_t)seg;
    const int64_t n = rec[1], off = rec[3];
    const int64_t nb_pad = up16((n + GQ_MX_BLOCK - 1) / GQ_MX_BLOCK);
    using T = typename Tensor<TT>::type;
    T *o = out + rec[5];
    const int64_t base = (item - rec[2]) * GQ_MX_ITEM_ELEMS;
    const bool direct = plain && R == 1;
    const float fR = (float)R;
    const uint32_t sbyte = sign_byte(signs);
    // (wire offsets are multiples of 16: the payloads' own alignment decides)
    const bool words = ((reinterpret_cast<uintptr_t>(gathered) | (uintptr_t)(R > 1 ? stride : 0)) & 7u) == 0;
    // (FP6: a pair of lanes owns 12 bytes at a multiple of 12 -- dword loads wherever the payloads are 4-byte aligned)
    const bool words6 = ((reinterpret_cast<uintptr_t>(gathered) | (uintptr_t)(R > 1 ? stride : 0)) & 3u) == 0;
    for (int s = 0; s < STEPS; ++s) {
        if (base + (int64_t)s * STEP >= n) break;      // (uniform over the workgroup; a lane behind the tensor's end reads nothing)
        const int64_t e0 = base + (int64_t)s * STEP + (int64_t)threadIdx.x * PER_LANE;
        const bool rot = (e0 & ~(int64_t)(GQ_MXR_BLOCK - 1)) + GQ_MXR_BLOCK <= n;
        const bool live = e0 < n;
        float acc[PER_LANE];
#pragma unroll
        for (int k = 0; k < PER_LANE; ++k) acc[k] = 0.0f;
        const uint8_t *p = gathered + off;
        for (int r = 0; r < R && live; ++r, p += stride) {
            const uint32_t sb = p[e0 / GQ_MX_BLOCK];
            const uint8_t *cp = p + nb_pad + (e0 / PER_LANE) * CODE_BYTES;
            uint32_t lo = 0, hi = 0;
            uint64_t six = 0;
            if (F::bits == 6) {
                six = load_codes6(cp, (e0 / PER_LANE) & 1, words6);
            } else if (words) {
                if (FMT == GQ_MX_FP4) {
                    lo = *reinterpret_cast<const uint32_t *>(cp);
                } else {
                    const uint2 q = *reinterpret_cast<const uint2 *>(cp);
                    lo = q.x, hi = q.y;
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) lo |= (uint32_t)cp[k] << (8 * k);
                if (FMT == GQ_MX_FP8) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) hi |= (uint32_t)cp[4 + k] << (8 * k);
                }
            }
            const int e = (int)sb - 127;
#pragma unroll
            for (int k = 0; k < PER_LANE; ++k) {
                const uint32_t code = F::bits == 6     ? (uint32_t)(six >> (6 * k)) & 63u
                                      : FMT == GQ_MX_FP4 ? (lo >> (4 * k)) & 15u
                                                         : ((k < 4 ? lo : hi) >> (8 * (k & 3))) & 255u;
                const float d = sb == 0xFFu ? __uint_as_float(QNAN) : decode_value<F>(code, e);
                acc[k] = direct ? d : acc[k] + d;
            }
        }
        float f[PER_LANE];
#pragma unroll
        for (int k = 0; k < PER_LANE; ++k) f[k] = direct ? acc[k] : acc[k] / fR;
        inverse(f, sbyte, rot);      // the mean first, then ONE inverse rotation
        if (live) {
            if (e0 + PER_LANE - 1 < n && aligned16(o + e0)) {
                store8(o + e0, f);      // (T = bf16: the f32 result narrowed once, here)
            } else {
                for (int k = 0; k < PER_LANE && e0 + k < n; ++k) o[e0 + k] = from_f32<T>(f[k]);
            }
        }
    }
}

static int check_batch(const gq_mxr_batch *b, const char *what, bool compress) {
    if (!b || b->struct_bytes != sizeof(gq_mxr_batch)) return fail(GQ_ERR_INVALID_ARG, "%s: descriptor missing or of another size", what);
    if (b->format != GQ_MX_FP4 && b->format != GQ_MX_FP8 && b->format != GQ_MX_FP6_E2M3 && b->format != GQ_MX_FP6_E3M2)
        return fail(GQ_ERR_INVALID_ARG, "%s: format %d (GQ_MX_FP4, GQ_MX_FP8, GQ_MX_FP6_E2M3 or GQ_MX_FP6_E3M2)", what, b->format);
    if (b->nseg < 1 || b->nitems < 1 || b->nitems > 0x7fffffff || b->ndense < 0)
        return fail(GQ_ERR_INVALID_ARG, "%s: bad sizes (nseg %d, nitems %lld, ndense %d)", what, b->nseg, (long long)b->nitems, b->ndense);
    if (!b->seg_table || !b->item_seg) return fail(GQ_ERR_INVALID_ARG, "%s: null table", what);
    if (compress && b->ndense > 0 && !b->dense_table) return fail(GQ_ERR_INVALID_ARG, "%s: null dense table", what);
    return GQ_OK;
}

static Signs signs_of(const gq_mxr_batch *b) { return Signs{{b->signs[0], b->signs[1], b->signs[2], b->signs[3]}}; }

template <int FMT, int MODE, int TT>
static void launch_compress(const gq_mxr_batch *b, uint8_t *wire, int random_mode, const float *r, uint64_t seed, float ef_scale,
                            typename Tensor<TT>::type *out, hipStream_t st) {
    const dim3 grid((unsigned)b->nitems), block(THREADS);
    if (!isnan(ef_scale))
        hipLaunchKernelGGL(HIP_KERNEL_NAME(mxr_compress_kernel<FMT, MODE, true, TT>), grid, block, 0, st, b->seg_table, b->item_seg, wire, out,
                           ef_scale, random_mode, r, seed, b->dense_table, b->ndense, signs_of(b));
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(mxr_compress_kernel<FMT, MODE, false, TT>), grid, block, 0, st, b->seg_table, b->item_seg, wire, out,
                           0.0f, random_mode, r, seed, b->dense_table, b->ndense, signs_of(b));
}

template <int FMT, int TT>
static void launch_compress(const gq_mxr_batch *b, uint8_t *wire, int random_mode, const float *r, uint64_t seed, float ef_scale,
                            typename Tensor<TT>::type *out, hipStream_t st) {
    if (random_mode == GQ_RANDOM_OFF)
        launch_compress<FMT, DRAW_OFF, TT>(b, wire, random_mode, r, seed, ef_scale, out, st);
    else if (random_mode == GQ_RANDOM_GIVEN)
        launch_compress<FMT, DRAW_GIVEN, TT>(b, wire, random_mode, r, seed, ef_scale, out, st);
    else
        launch_compress<FMT, DRAW_DEVICE, TT>(b, wire, random_mode, r, seed, ef_scale, out, st);
}

// The two entry points of a tensor-side type: `what` is the exported name (the refusals quote it).  out needs the alignment of T.
template <int TT>
static int compress_batched(const char *what, const gq_mxr_batch *b, uint8_t *wire, int random_mode, const float *r, uint64_t seed, float ef_scale,
                            typename Tensor<TT>::type *out, void *stream) {
    constexpr unsigned ALIGN = sizeof(typename Tensor<TT>::type);
    const int rc = check_batch(b, what, true);
    if (rc != GQ_OK) return rc;
    if (random_mode != GQ_RANDOM_OFF && random_mode != GQ_RANDOM_GIVEN && random_mode != GQ_RANDOM_DEVICE &&
        random_mode != GQ_RANDOM_DEVICE_COUNTER)
        return fail(GQ_ERR_INVALID_ARG, "%s: random_mode %d (off, given, device or device counter)", what, random_mode);
    if (random_mode == GQ_RANDOM_GIVEN && !r) return fail(GQ_ERR_INVALID_ARG, "%s: GQ_RANDOM_GIVEN without draws", what);
    if (random_mode == GQ_RANDOM_DEVICE_COUNTER && (seed == 0 || (seed & 7) != 0))
        return fail(GQ_ERR_INVALID_ARG, "%s: GQ_RANDOM_DEVICE_COUNTER needs the address of a { seed, step } pair", what);
    if (!wire || (reinterpret_cast<uintptr_t>(wire) & 15) != 0)
        return fail(GQ_ERR_INVALID_ARG, "%s: the wire must be a 16-byte aligned device buffer", what);
    if ((reinterpret_cast<uintptr_t>(out) & (ALIGN - 1)) != 0 || (reinterpret_cast<uintptr_t>(r) & 3) != 0)
        return fail(GQ_ERR_INVALID_ARG, "%s: out must be %u-byte aligned and r 4-byte aligned", what, ALIGN);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (b->format == GQ_MX_FP4)
        launch_compress<GQ_MX_FP4, TT>(b, wire, random_mode, r, seed, ef_scale, out, st);
    else if (b->format == GQ_MX_FP8)
        launch_compress<GQ_MX_FP8, TT>(b, wire, random_mode, r, seed, ef_scale, out, st);
    else if (b->format == GQ_MX_FP6_E2M3)
        launch_compress<GQ_MX_FP6_E2M3, TT>(b, wire, random_mode, r, seed, ef_scale, out, st);
    else
        launch_compress<GQ_MX_FP6_E3M2, TT>(b, wire, random_mode, r, seed, ef_scale, out, st);
    GQL_CHECK_LAUNCH(what);
    return GQ_OK;
}

template <int TT>
static int decode_sum_batched(const char *what, const gq_mxr_batch *b, const uint8_t *gathered, int64_t user_stride_bytes, int R,
                              typename Tensor<TT>::type *out, int plain, void *stream) {
    constexpr unsigned ALIGN = sizeof(typename Tensor<TT>::type);
    const int rc = check_batch(b, what, false);
    if (rc != GQ_OK) return rc;
    if (!gathered || !out) return fail(GQ_ERR_INVALID_ARG, "%s: null pointer", what);
    if (R < 1 || (R > 1 && user_stride_bytes < 0))
        return fail(GQ_ERR_INVALID_ARG, "%s: R = %d, user stride %lld", what, R, (long long)user_stride_bytes);
    if ((reinterpret_cast<uintptr_t>(out) & (ALIGN - 1)) != 0) return fail(GQ_ERR_INVALID_ARG, "%s: out must be %u-byte aligned", what, ALIGN);
    const dim3 grid((unsigned)b->nitems), block(THREADS);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (b->format == GQ_MX_FP4)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(mxr_decode_kernel<GQ_MX_FP4, TT>), grid, block, 0, st, b->seg_table, b->item_seg, gathered,
                           user_stride_bytes, R, out, plain ? 1 : 0, signs_of(b));
    else if (b->format == GQ_MX_FP8)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(mxr_decode_kernel<GQ_MX_FP8, TT>), grid, block, 0, st, b->seg_table, b->item_seg, gathered,
                           user_stride_bytes, R, out, plain ? 1 : 0, signs_of(b));
    else if (b->format == GQ_MX_FP6_E2M3)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(mxr_decode_kernel<GQ_MX_FP6_E2M3, TT>), grid, block, 0, st, b->seg_table, b->item_seg, gathered,
                           user_stride_bytes, R, out, plain ? 1 : 0, signs_of(b));
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(mxr_decode_kernel<GQ_MX_FP6_E3M2, TT>), grid, block, 0, st, b->seg_table, b->item_seg, gathered,
                           user_stride_bytes, R, out, plain ? 1 : 0, signs_of(b));
    GQL_CHECK_LAUNCH(what);
    return GQ_OK;
}

}  // namespace gqx

GQXR_API int gq_mxr_abi_version(void) { return GQ_MXR_ABI_VERSION; }
                                
GQXR_API const char *gq_mxr_last_error(void) { return gqx::err_buf; }

GQXR_API int gq_mxr_compress_batched(const gq_mxr_batch *b, uint8_t *wire, int random_mode, const float *r, uint64_t seed, float ef_scale,
                                     float *out, void *stream) {
    return gqx::compress_batched<gqx::TT_F32>("gq_mxr_compress_batched", b, wire, random_mode, r, seed, ef_scale, out, stream);
}

GQXR_API int gq_mxr_decode_sum_batched(const gq_mxr_batch *b, const uint8_t *gathered, int64_t user_stride_bytes, int R, float *out, int plain,
                                       void *stream) {
    return gqx::decode_sum_batched<gqx::TT_F32>("gq_mxr_decode_sum_batched", b, gathered, user_stride_bytes, R, out, plain, stream);
}

// the same launches over bf16 sources, `out` and dense-copy sources (include/gq_mxr.h, TENSOR-SIDE TYPE); the wire is the f32 twin's
GQXR_API int gq_mxr_compress_batched_bf16(const gq_mxr_batch *b, uint8_t *wire, int random_mode, const float *r, uint64_t seed, float ef_scale,
                                          uint16_t *out, void *stream) {
    return gqx::compress_batched<gqx::TT_BF16>("gq_mxr_compress_batched_bf16", b, wire, random_mode, r, seed, ef_scale, out, stream);
}

GQXR_API int gq_mxr_decode_sum_batched_bf16(const gq_mxr_batch *b, const uint8_t *gathered, int64_t user_stride_bytes, int R, uint16_t *out,
                                            int plain, void *stream) {
    return gqx::decode_sum_batched<gqx::TT_BF16>("gq_mxr_decode_sum_batched_bf16", b, gathered, user_stride_bytes, R, out, plain, stream);
}
