// The ONE compress kernel, the ONE decode kernel and the ONE host path of libgq_mx.so (mx.hip) and libgq_mxr.so (mxr.hip), over a
// rotation policy ROT (include/gq_mx.h and include/gq_mxr.h: the contracts, to the bit).  Internal linkage: each library compiles
// its own instantiations.  A policy is
//     struct ROT {
//         using Args = ...;                       // what the kernels take by value as their last argument (Plain: an empty struct)
//         static constexpr bool EVERY_LANE;       // forward / inverse exchange across lanes: no lane may skip them
//         __device__ explicit ROT(const Args &);  // built once per kernel, before the step loop
//         static constexpr int BLOCK;             // elements of a rotation block, a power of two (0: nothing is rotated); a block
//                                                 // that does not lie whole inside its tensor stays as it is (rot = false)
//         __device__ const Lane8 &forward(const Lane8 &w, Lane8 &buf, bool rot) const;      // w -> x', what is coded: buf, or w itself
//         __device__ void inverse(Lane8 &y, bool rot) const;                                // decoded values back, in place
//         static Args args(const <its descriptor> *b);                               // host: the descriptor's part of it
//     };
// The __global__ kernels themselves are the templates, with __restrict__ on their own parameters: the same body behind a
// one-line __global__ wrapper compiles to other code.  EVERY_LANE is the one difference in control flow, and it
// is a compile-time one: with it the kernels leave their loops and skip the decode on workgroup-uniform tests only and mask the
// loads and stores per lane; without it a lane behind its tensor's end leaves at once.
//
// compress  one workgroup per item of GQ_MX_ITEM_ELEMS = 4096 elements (128 blocks), in two steps of 2048.  A lane owns eight
//           consecutive elements (two float4 loads; scalar loads at a tensor's ragged end or on a misaligned view), so the four
//           lanes of a quad own a block: the block's largest magnitude is two shuffles inside the quad -- no LDS round trip, no
//           atomics -- and the exponent follows from its bits in integers.  An element is scaled by one ldexp (exact unless the
//           result is subnormal) and split into code and fraction with shifts of its bits; the fraction, rebuilt as an exact f32,
//           is compared with the draw.  A lane stores its 4 (FP4) or 8 (FP8) code bytes as one word / word pair; the scale bytes
//           of four quads are gathered into one word by two more shuffles.  Every byte of the section is written, the pad
//           included.  Also: the dense decode (out), error feedback (w back into the source, err = w - decoded), and the
//           identity-compressed tensors copied into the wire.  The stream is 4 B read per element, like sign.hip; no scratch.
// decode    the same items and lanes; a lane reads its block's scale byte and its code bytes of each of the R payloads in
//           order (words where the payloads are 8-byte aligned, bytes otherwise), adds the exact values and divides by R.
// f32 subnormals are kept (hipcc's default kernel mode, float_denorm_mode_32 = 3): ldexp rounds onto the 2^-149 grid and the
// comparison sees subnormal fractions and draws as they are.
// Every launch's arguments depend on the layout alone: both replay from a HIP graph.
#pragma once
#include <math.h>

#include <type_traits>

#include "gq_common.hpp"
#include "gq_lib_prelude.hpp"
#include "mx_common.hpp"

namespace gqx {

constexpr int THREADS = 256;
constexpr int PER_LANE = 8;                           // elements of a lane: a quad owns a block of 32
constexpr int STEP = THREADS * PER_LANE;              // elements of a workgroup-wide step
constexpr int STEPS = GQ_MX_ITEM_ELEMS / STEP;
using Lane8 = float[PER_LANE];                        // a lane's elements as f32
static_assert(GQ_MX_BLOCK == 4 * PER_LANE, "a quad owns a block");
static_assert(GQ_MX_ITEM_ELEMS % STEP == 0 && GQ_MX_ITEM_ELEMS % (16 * GQ_MX_BLOCK) == 0, "an item is whole steps and whole 16-byte runs of scale bytes");

using gql::aligned16;
using gql::copy_dense;
using gql::err_buf;
using gql::fail;

template <class ROT, int FMT, int MODE, bool EF, int TT>
__global__ __launch_bounds__(THREADS) void mx_compress_kernel(const int64_t *__restrict__ seg_table, const int32_t *__restrict__ item_seg,
                                                              uint8_t *__restrict__ wire, typename Tensor<TT>::type *__restrict__ out, float ef_scale,
                                                              int random_mode, const float *__restrict__ rbuf, uint64_t seed,
                                                              const int64_t *__restrict__ dense_table, int ndense, typename ROT::Args rot_args) {
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
    const ROT rotation(rot_args);
    const int64_t base = (item - rec[2]) * GQ_MX_ITEM_ELEMS;
    for (int s = 0; s < STEPS; ++s) {
        if (base + (int64_t)s * STEP >= nb_pad * GQ_MX_BLOCK) break;      // (uniform over the workgroup)
        const int64_t e0 = base + (int64_t)s * STEP + (int64_t)threadIdx.x * PER_LANE;      // this lane's first element
        // the lane's rotation block lies whole inside the tensor (uniform over the block's lanes); otherwise it is the tail as it is.
        // (Written out here and in the decode kernel: behind a policy member, even a force-inlined one, other code comes out.)
        const bool rot = ROT::BLOCK > 0 && (e0 & ~(int64_t)(ROT::BLOCK - 1)) + ROT::BLOCK <= n;
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
        float xbuf[PER_LANE];
        const Lane8 &x = rotation.forward(w, xbuf, rot);      // x': what is coded (Plain: w itself, not a copy of it)
        // the block's largest magnitude, as bits: inside the lane, then across the quad that owns the block
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
        // EVERY_LANE: o || ef is uniform over the workgroup, so the inverse's exchanges run in every lane
        if ((ROT::EVERY_LANE || e0 < n) && (o || ef)) {
            float d[PER_LANE];
#pragma unroll
            for (int k = 0; k < PER_LANE; ++k) d[k] = bad ? __uint_as_float(QNAN) : decode_value<F>(c[k], e);
            rotation.inverse(d, rot);
            if (!ROT::EVERY_LANE || e0 < n) {      // (the stores: per lane)
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

template <class ROT, int FMT, int TT>
__global__ __launch_bounds__(THREADS) void mx_decode_kernel(const int64_t *__restrict__ seg_table, const int32_t *__restrict__ item_seg,
                                                            const uint8_t *__restrict__ gathered, int64_t stride, int R,
                                                            typename Tensor<TT>::type *__restrict__ out, int plain, typename ROT::Args rot_args) {
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
    const ROT rotation(rot_args);
    // (wire offsets are multiples of 16: the payloads' own alignment decides)
    const bool words = ((reinterpret_cast<uintptr_t>(gathered) | (uintptr_t)(R > 1 ? stride : 0)) & 7u) == 0;
    // (FP6: a pair of lanes owns 12 bytes at a multiple of 12 -- dword loads wherever the payloads are 4-byte aligned)
    const bool words6 = ((reinterpret_cast<uintptr_t>(gathered) | (uintptr_t)(R > 1 ? stride : 0)) & 3u) == 0;
    for (int s = 0; s < STEPS; ++s) {
        // EVERY_LANE: leave on the workgroup's first element (uniform); a lane behind the tensor's end stays and reads nothing
        if (ROT::EVERY_LANE && base + (int64_t)s * STEP >= n) break;
        const int64_t e0 = base + (int64_t)s * STEP + (int64_t)threadIdx.x * PER_LANE;
        if (!ROT::EVERY_LANE && e0 >= n) break;
        const bool rot = ROT::BLOCK > 0 && (e0 & ~(int64_t)(ROT::BLOCK - 1)) + ROT::BLOCK <= n;
        const bool live = e0 < n;      // (always so without EVERY_LANE)
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
        rotation.inverse(f, rot);      // the mean first, then ONE inverse transform
        if (live) {
            if (e0 + PER_LANE - 1 < n && aligned16(o + e0)) {
                store8(o + e0, f);      // (T = bf16: the f32 result narrowed once, here)
            } else {
                for (int k = 0; k < PER_LANE && e0 + k < n; ++k) o[e0 + k] = from_f32<T>(f[k]);
            }
        }
    }
}

// ---- the host path, over the policy and the descriptor B (gq_mx_batch, or gq_mxr_batch: the same fields, then its own) -------------
template <class B>
static int check_batch(const B *b, const char *what, bool compress) {
    if (!b || b->struct_bytes != sizeof(B)) return fail(GQ_ERR_INVALID_ARG, "%s: descriptor missing or of another size", what);
    if (b->format != GQ_MX_FP4 && b->format != GQ_MX_FP8 && b->format != GQ_MX_FP6_E2M3 && b->format != GQ_MX_FP6_E3M2)
        return fail(GQ_ERR_INVALID_ARG, "%s: format %d (GQ_MX_FP4, GQ_MX_FP8, GQ_MX_FP6_E2M3 or GQ_MX_FP6_E3M2)", what, b->format);
    if (b->nseg < 1 || b->nitems < 1 || b->nitems > 0x7fffffff || b->ndense < 0)
        return fail(GQ_ERR_INVALID_ARG, "%s: bad sizes (nseg %d, nitems %lld, ndense %d)", what, b->nseg, (long long)b->nitems, b->ndense);
    if (!b->seg_table || !b->item_seg) return fail(GQ_ERR_INVALID_ARG, "%s: null table", what);
    if (compress && b->ndense > 0 && !b->dense_table) return fail(GQ_ERR_INVALID_ARG, "%s: null dense table", what);
    return GQ_OK;
}

// f(std::integral_constant<int, the format>): the one ladder over the formats (format: checked by check_batch)
template <class Fn>
static void with_format(int format, Fn f) {
    if (format == GQ_MX_FP4)
        f(std::integral_constant<int, GQ_MX_FP4>());
    else if (format == GQ_MX_FP8)
        f(std::integral_constant<int, GQ_MX_FP8>());
    else if (format == GQ_MX_FP6_E2M3)
        f(std::integral_constant<int, GQ_MX_FP6_E2M3>());
    else
        f(std::integral_constant<int, GQ_MX_FP6_E3M2>());
}

// f(std::integral_constant<int, DRAW_*>): the kernels' draw of a (checked) random_mode
template <class Fn>
static void with_draw(int random_mode, Fn f) {
    if (random_mode == GQ_RANDOM_OFF)
        f(std::integral_constant<int, DRAW_OFF>());
    else if (random_mode == GQ_RANDOM_GIVEN)
        f(std::integral_constant<int, DRAW_GIVEN>());
    else
        f(std::integral_constant<int, DRAW_DEVICE>());
}

// The two entry points of a tensor-side type: `what` is the exported name (the refusals quote it).  out needs the alignment of T.
template <class ROT, int TT, class B>
static int compress_batched(const char *what, const B *b, uint8_t *wire, int random_mode, const float *r, uint64_t seed, float ef_scale,
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
    const dim3 grid((unsigned)b->nitems), block(THREADS);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const bool ef = !isnan(ef_scale);
    with_format(b->format, [&](auto fmt) {
        with_draw(random_mode, [&](auto draw) {
            constexpr int FMT = decltype(fmt)::value, MODE = decltype(draw)::value;
            if (ef)
                hipLaunchKernelGGL(HIP_KERNEL_NAME(mx_compress_kernel<ROT, FMT, MODE, true, TT>), grid, block, 0, st, b->seg_table, b->item_seg,
                                   wire, out, ef_scale, random_mode, r, seed, b->dense_table, b->ndense, ROT::args(b));
            else
                hipLaunchKernelGGL(HIP_KERNEL_NAME(mx_compress_kernel<ROT, FMT, MODE, false, TT>), grid, block, 0, st, b->seg_table, b->item_seg,
                                   wire, out, 0.0f, random_mode, r, seed, b->dense_table, b->ndense, ROT::args(b));
        });
    });
    GQL_CHECK_LAUNCH(what);
    return GQ_OK;
}

template <class ROT, int TT, class B>
static int decode_sum_batched(const char *what, const B *b, const uint8_t *gathered, int64_t user_stride_bytes, int R,
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
    with_format(b->format, [&](auto fmt) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(mx_decode_kernel<ROT, decltype(fmt)::value, TT>), grid, block, 0, st, b->seg_table, b->item_seg,
                           gathered, user_stride_bytes, R, out, plain ? 1 : 0, ROT::args(b));
    });
    GQL_CHECK_LAUNCH(what);
    return GQ_OK;
}

}  // namespace gqx
