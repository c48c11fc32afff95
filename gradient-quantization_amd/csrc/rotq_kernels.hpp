// The ONE compress kernel, the TWO decode-mean kernels and the ONE host path of libgq_drive.so (drive.hip) and libgq_eden.so
// (eden.hip), over a coder policy (include/gq_drive.h and include/gq_eden.h: the contracts, to the bit; tests/drive_contract.py and
// tests/eden_contract.py restate them in numpy).  Internal linkage: each library compiles its own instantiations.
// DRIVE is the one-bit member of EDEN's family: both rotate a zero-padded block of 256, code its coordinates against one f32
// scale, and differ in the code alone.  A coder is an empty struct of static functions (gqd::Sign1 in drive.hip, gqe::LloydMax<B> in eden.hip):
//     struct Coder {
//         static constexpr int CODE_BYTES;        // a block's code bytes
//         template <int SCALE>                    // x' -> the lane's eight codes (word) and the block's scale S; c: what
//         __device__ static float encode(const HadLane &x, uint32_t &word, float (&c)[PER_LANE]);      // decoded() keeps of it
//         __device__ static float decoded(float S, uint32_t word, const float (&c)[PER_LANE], const HadLane &x, int k);
//                                                 // the value of the lane's code k, for the compress launch's own inverse path
//         __device__ static void store(uint8_t *block, uint32_t l, bool live, uint32_t word);      // the block's code bytes; EVERY
//                                                 // lane calls it (its exchanges sit outside the bounds test)
//         __device__ static uint32_t load(const uint8_t *p, int64_t lane, bool words);             // a lane's codes of payload p
//         __device__ static float value(uint32_t word, uint32_t sbits, int k);                     // code k under the scale's bits
//     };
// and a library states its descriptor, its own check and which coder a descriptor asks for in a small trait (see the host path).
// The __global__ kernels themselves are the templates, with __restrict__ on their own parameters.
//
// The kernels have the shape of csrc/mx_kernels.hpp's: one workgroup per item of GQ_MX_ITEM_ELEMS = 4096 elements, two steps of
// 2048, a lane owns eight consecutive elements (two float4 loads; scalar loads at a tensor's ragged end or on a misaligned view)
// and a 32-lane half a block of 256.  The rotation is csrc/hadamard.hpp's, shared with mxr.hip.  Everything between the loads and
// the stores stays in registers: no LDS is allocated, no barrier, no scratch.
// compress  load (+ error feedback) -> sign flip -> 8 stages -> * 2^-4 = x' -> the coder's encode: a lane's eight codes are whole
//           bytes, and the block's sums are the contract's balanced tree (block_sum: three levels inside the lane, five across
//           the half -- an addition commutes, so the lane on either side of a pair gets the same bits), then ONE division.  The
//           coder stores the block's code bytes; lane 0 of the half stores the scale.  If `out` or error feedback is asked for:
//           the decoded values -> 8 stages -> * 2^-4 -> sign flip -> out / w / err = w - D.
// decode    the same items and lanes; a lane reads its code bytes and its block's scale of each of the R payloads in order
//           (aligned loads where the payloads are 4-byte aligned, bytes otherwise), adds the values and divides by R, then ONE
//           inverse transform, then the store.
// The last block of a tensor is zero-padded and rotated like any other, so whether a lane takes part is a test on its BLOCK
// (blk < nb), uniform over the half, and the steps are left on workgroup-uniform tests only: no exchange sits under divergent
// control flow.  Loads and stores are masked per lane (e0 + k < n).
// Every launch's arguments depend on the layout alone, and there are no draws: both replay from a HIP graph as they are.
// stepped   the *_stepped entry points: the same bodies, with the lane's sign byte made once per launch from a device
//           { seed, step } pair (gqx::stepped_sign_byte) instead of from four words passed by value.  The pair's ADDRESS is the
//           launch argument: a replay rotates afresh once the step word has moved.
// streams   the *_streams entry points (SIGNS, PER STREAM).  compress is the stepped kernel with one more step in its prelude:
//           pair -> the stream's seed (one 64-bit multiply-add and one finaliser, on uniform values) -> the lane's sign byte.
//           decode-mean is a body of its own: payload r was rotated by stream first + r, so it goes through its OWN inverse
//           transform and the mean is taken in the gradient's domain -- R transforms per block.  The payload loop is the outer
//           one and the item's two steps the inner one, so a stream's sign byte is derived once per workgroup and payload (never
//           once per block) whatever R is, with nothing kept in an R-sized array; across payloads a lane keeps its 2 x 8
//           accumulators and nothing else.
#pragma once
#include <math.h>

#include "gq_lib_prelude.hpp"
#include "hadamard.hpp"
#include "mx_common.hpp"

namespace gqr {

using gql::aligned16;
using gql::check_rotation;
using gql::copy_dense;
using gql::err_buf;
using gql::fail;
using gqx::Hadamard;
using gqx::HadLane;
using gqx::lane_xor;
using gqx::load8;      // a lane's eight f32, full form: csrc/mx_common.hpp's
using gqx::store8;
using gqx::QNAN;       // the scale of a block that is not finite
using gqx::Signs;

constexpr int THREADS = 256;
constexpr int PER_LANE = gqx::HAD_PER_LANE;          // elements of a lane: a 32-lane half owns a block of 256
constexpr int BLOCK = gqx::HAD_BLOCK;                 // elements that share a scale (GQ_DRIVE_BLOCK, GQ_EDEN_BLOCK): a rotation block
constexpr int STEP = THREADS * PER_LANE;              // elements of a workgroup-wide step: 8 blocks
constexpr int STEPS = GQ_MX_ITEM_ELEMS / STEP;
enum { UNBIASED = 0, MSE = 1 };                       // the scale modes (GQ_DRIVE_UNBIASED / _MSE, GQ_EDEN_UNBIASED / _MSE)
static_assert(STEP % BLOCK == 0 && GQ_MX_ITEM_ELEMS % STEP == 0, "a 32-lane half owns a block, an item is whole steps");
static_assert((STEP / BLOCK) % 4 == 0, "a step holds whole 16-byte runs of scales: the scales' pad lies in the step of the last block");

// lane_xor over a word of bits
template <int M>
__device__ __forceinline__ uint32_t lane_xor_bits(uint32_t v) {
    return __float_as_uint(lane_xor<M>(__uint_as_float(v)));      // (moves only: no arithmetic touches the bits)
}

// the contract's balanced tree over the block's 256 values, eight of them in this lane: levels 0 .. 2 here, 3 .. 7 across the half
__device__ __forceinline__ float block_sum(const float (&a)[PER_LANE]) {
    const float a01 = a[0] + a[1], a23 = a[2] + a[3], a45 = a[4] + a[5], a67 = a[6] + a[7];
    const float lo = a01 + a23, hi = a45 + a67;
    float s = lo + hi;
    s = s + lane_xor<1>(s);
    s = s + lane_xor<2>(s);
    s = s + lane_xor<4>(s);
    s = s + lane_xor<8>(s);
    s = s + lane_xor<16>(s);
    return s;
}

// ---- the kernels -------------------------------------------------------------------------------------------------------------------
// Rot: how the launch is told its rotation -- gqx::Signs (the four words, by value), gqx::Stepped (the address of a device
// { seed, step } pair) or gqx::Streamed (the pair and a stream): the only difference between the launch kinds is how `rotation`
// below is built
template <class Coder, int SCALE, bool EF, class Rot>
__global__ __launch_bounds__(THREADS) void compress_kernel(const int64_t *__restrict__ seg_table, const int32_t *__restrict__ item_seg,
                                                           uint8_t *__restrict__ wire, float *__restrict__ out, float ef_scale,
                                                           const int64_t *__restrict__ dense_table, int ndense, Rot signs) {
    copy_dense<THREADS>(dense_table, ndense, wire);
    const int64_t item = blockIdx.x;
    const int seg = item_seg[item];
    const int64_t *rec = seg_table + 8 * (int64_t)seg;
    const int64_t n = rec[1];
    const int64_t nb = (n + BLOCK - 1) / BLOCK, nb_pad = (nb + 3) / 4 * 4;
    float *v = reinterpret_cast<float *>(rec[0]);
    float *err = EF ? reinterpret_cast<float *>(rec[7]) : nullptr;
    uint8_t *codes = wire + rec[3];
    float *scales = reinterpret_cast<float *>(codes + nb * Coder::CODE_BYTES);
    float *o = out ? out + rec[5] : nullptr;
    const uint32_t l = threadIdx.x & 31u;      // the lane's place in the half that owns its block
    const Hadamard rotation(signs);
    const int64_t base = (item - rec[2]) * GQ_MX_ITEM_ELEMS;
    for (int s = 0; s < STEPS; ++s) {
        if (base + (int64_t)s * STEP >= nb * BLOCK) break;      // (uniform over the workgroup)
        const int64_t e0 = base + (int64_t)s * STEP + (int64_t)threadIdx.x * PER_LANE;      // this lane's first element
        const int64_t blk = e0 / BLOCK;                                                     // (uniform over the half)
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
                    w[k] = v[e0 + k];
                    if (ef) {
                        const float p = ef_scale * err[e0 + k];
                        w[k] = w[k] + p;
                    }
                }
            }
        }
        float xbuf[PER_LANE];
        const HadLane &x = rotation.forward(w, xbuf, true);      // x': every block is rotated, the zero-padded last one too
        uint32_t word;             // the lane's eight codes
        float cm[PER_LANE];        // (what the coder's decoded() keeps of its encode; Sign1 leaves it untouched and never reads it)
        const float S = Coder::template encode<SCALE>(x, word, cm);
        // o || ef is uniform over the workgroup, so the inverse's exchanges run in every lane
        if (o || ef) {
            float d[PER_LANE];
#pragma unroll
            for (int k = 0; k < PER_LANE; ++k) d[k] = Coder::decoded(S, word, cm, x, k);
            rotation.inverse(d, true);
            if (e0 < n) {      // (the stores: per lane)
                const bool vec = e0 + PER_LANE - 1 < n;
                if (o) {
                    if (vec && aligned16(o + e0)) {
                        store8(o + e0, d);
                    } else {
                        for (int k = 0; k < PER_LANE && e0 + k < n; ++k) o[e0 + k] = d[k];
                    }
                }
                if (ef) {
                    if (full) {
                        store8(v + e0, w);
                        *reinterpret_cast<float4 *>(err + e0) = make_float4(w[0] - d[0], w[1] - d[1], w[2] - d[2], w[3] - d[3]);
                        *reinterpret_cast<float4 *>(err + e0 + 4) = make_float4(w[4] - d[4], w[5] - d[5], w[6] - d[6], w[7] - d[7]);
                    } else {
                        for (int k = 0; k < PER_LANE && e0 + k < n; ++k) {
                            v[e0 + k] = w[k];
                            err[e0 + k] = w[k] - d[k];
                        }
                    }
                }
            }
        }
        Coder::store(codes + blk * Coder::CODE_BYTES, l, blk < nb, word);
        // the scale, and +0 in the scales' pad (which lies in the step of the last block)
        if (l == 0 && blk < nb_pad) scales[blk] = blk < nb ? S : 0.0f;
    }
}

template <class Coder, class Rot>
__global__ __launch_bounds__(THREADS) void decode_kernel(const int64_t *__restrict__ seg_table, const int32_t *__restrict__ item_seg,
                                                         const uint8_t *__restrict__ gathered, int64_t stride, int R,
                                                         float *__restrict__ out, int plain, Rot signs) {
    const int64_t item = blockIdx.x;
    const int seg = item_seg[item];
    const int64_t *rec = seg_table + 8 * (int64_t)seg;
    const int64_t n = rec[1], off = rec[3];
    const int64_t nb = (n + BLOCK - 1) / BLOCK;
    float *o = out + rec[5];
    const int64_t base = (item - rec[2]) * GQ_MX_ITEM_ELEMS;
    const bool direct = plain != 0;      // (the host side: R == 1)
    const float fR = (float)R;
    const Hadamard rotation(signs);
    // (wire offsets are multiples of 16 and the codes of a section a multiple of 4 bytes: the payloads' own alignment decides)
    const bool words = ((reinterpret_cast<uintptr_t>(gathered) | (uintptr_t)(R > 1 ? stride : 0)) & 3u) == 0;
    for (int s = 0; s < STEPS; ++s) {
        if (base + (int64_t)s * STEP >= n) break;      // (uniform over the workgroup)
        const int64_t e0 = base + (int64_t)s * STEP + (int64_t)threadIdx.x * PER_LANE;
        const int64_t blk = e0 / BLOCK;
        const bool live = blk < nb;      // (uniform over the half; the elements behind n - 1 of a last block are decoded too)
        float acc[PER_LANE];
#pragma unroll
        for (int k = 0; k < PER_LANE; ++k) acc[k] = 0.0f;
        const uint8_t *p = gathered + off;
        for (int r = 0; r < R && live; ++r, p += stride) {
            const uint32_t word = Coder::load(p, e0 / PER_LANE, words);
            // the scale's two forms stay written out here: behind a function the compiler joins them into one unaligned load
            const uint8_t *sp = p + nb * Coder::CODE_BYTES + 4 * blk;
            uint32_t sbits = 0;
            if (words) {
                sbits = *reinterpret_cast<const uint32_t *>(sp);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) sbits |= (uint32_t)sp[k] << (8 * k);
            }
#pragma unroll
            for (int k = 0; k < PER_LANE; ++k) {
                const float y = Coder::value(word, sbits, k);
                acc[k] = direct ? y : acc[k] + y;
            }
        }
        float f[PER_LANE];
#pragma unroll
        for (int k = 0; k < PER_LANE; ++k) f[k] = direct ? acc[k] : acc[k] / fR;
        rotation.inverse(f, true);      // the mean first, then ONE inverse transform
        if (e0 < n) {
            if (e0 + PER_LANE - 1 < n && aligned16(o + e0)) {
                store8(o + e0, f);
            } else {
                for (int k = 0; k < PER_LANE && e0 + k < n; ++k) o[e0 + k] = f[k];
            }
        }
    }
}

// SIGNS, PER STREAM: payload r under stream first + r.  Every lane of the workgroup runs every exchange: a block that is not there
// (blk >= nb) decodes zeros that are never stored; a step that is not there is skipped on a workgroup-uniform test.
template <class Coder>
__global__ __launch_bounds__(THREADS) void decode_streams_kernel(const int64_t *__restrict__ seg_table, const int32_t *__restrict__ item_seg,
                                                                 const uint8_t *__restrict__ gathered, int64_t stride, int R,
                                                                 float *__restrict__ out, int plain, const uint64_t *__restrict__ pair,
                                                                 uint32_t first) {
    const int64_t item = blockIdx.x;
    const int seg = item_seg[item];
    const int64_t *rec = seg_table + 8 * (int64_t)seg;
    const int64_t n = rec[1], off = rec[3];
    const int64_t nb = (n + BLOCK - 1) / BLOCK;
    float *o = out + rec[5];
    const int64_t base = (item - rec[2]) * GQ_MX_ITEM_ELEMS;
    const bool direct = plain != 0;      // (the host side: R == 1)
    const float fR = (float)R;
    const uint64_t seed = pair[0], step = pair[1];      // (one uniform read per launch)
    const bool words = ((reinterpret_cast<uintptr_t>(gathered) | (uintptr_t)(R > 1 ? stride : 0)) & 3u) == 0;
    const int64_t lane0 = base + (int64_t)threadIdx.x * PER_LANE;      // this lane's first element of step 0
    float acc[STEPS][PER_LANE];
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
#pragma unroll
        for (int k = 0; k < PER_LANE; ++k) acc[s][k] = 0.0f;
    }
    const uint8_t *p = gathered + off;
    for (int r = 0; r < R; ++r, p += stride) {
        const Hadamard rotation(gqx::stream_sign_byte(seed, step, first + (uint32_t)r));
#pragma unroll
        for (int s = 0; s < STEPS; ++s) {
            if (base + (int64_t)s * STEP < n) {      // (uniform over the workgroup)
                const int64_t e0 = lane0 + (int64_t)s * STEP;
                const int64_t blk = e0 / BLOCK;
                uint32_t word = 0, sbits = 0;
                if (blk < nb) {      // (uniform over the half: loads only, no exchange in here)
                    word = Coder::load(p, e0 / PER_LANE, words);
                    const uint8_t *sp = p + nb * Coder::CODE_BYTES + 4 * blk;
                    if (words) {
                        sbits = *reinterpret_cast<const uint32_t *>(sp);
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; ++k) sbits |= (uint32_t)sp[k] << (8 * k);
                    }
                }
                float y[PER_LANE];
#pragma unroll
                for (int k = 0; k < PER_LANE; ++k) y[k] = Coder::value(word, sbits, k);
                rotation.inverse(y, true);      // this payload's own inverse transform
#pragma unroll
                for (int k = 0; k < PER_LANE; ++k) acc[s][k] = direct ? y[k] : acc[s][k] + y[k];
            }
        }
    }
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
        const int64_t e0 = lane0 + (int64_t)s * STEP;
        if (e0 < n) {
            float f[PER_LANE];
#pragma unroll
            for (int k = 0; k < PER_LANE; ++k) f[k] = direct ? acc[s][k] : acc[s][k] / fR;
            if (e0 + PER_LANE - 1 < n && aligned16(o + e0)) {
                store8(o + e0, f);
            } else {
                for (int k = 0; k < PER_LANE && e0 + k < n; ++k) o[e0 + k] = f[k];
            }
        }
    }
}

// ---- the host path -----------------------------------------------------------------------------------------------------------------
// A library's trait Lib states what is its own:
//     struct Lib {
//         using Batch = ...;                                         // its descriptor: struct_bytes, nseg, nitems, seg_table, item_seg,
//                                                                    // dense_table, ndense, scale_mode, ..., signs[4]
//         static constexpr const char *SCALE_MODES;                  // the names of its two scale modes, for the message
//         static int check_own(const Batch *b, const char *what);    // the fields no other descriptor has
//         template <class F> static void with_coder(const Batch *b, F f);      // f(the coder b asks for)
//     };
template <class Lib>
static int check_batch(const typename Lib::Batch *b, const char *what, bool compress) {
    if (!b || b->struct_bytes != sizeof(typename Lib::Batch)) return fail(GQ_ERR_INVALID_ARG, "%s: descriptor missing or of another size", what);
    const int own = Lib::check_own(b, what);
    if (own != GQ_OK) return own;
    if (b->scale_mode != UNBIASED && b->scale_mode != MSE)
        return fail(GQ_ERR_INVALID_ARG, "%s: scale_mode %d (%s)", what, b->scale_mode, Lib::SCALE_MODES);
    if (b->nseg < 1 || b->nitems < 1 || b->nitems > 0x7fffffff || b->ndense < 0)
        return fail(GQ_ERR_INVALID_ARG, "%s: bad sizes (nseg %d, nitems %lld, ndense %d)", what, b->nseg, (long long)b->nitems, b->ndense);
    if (!b->seg_table || !b->item_seg) return fail(GQ_ERR_INVALID_ARG, "%s: null table", what);
    if (compress && b->ndense > 0 && !b->dense_table) return fail(GQ_ERR_INVALID_ARG, "%s: null dense table", what);
    return GQ_OK;
}

// SIGNS, PER STREAM: streams first ... first + R - 1 are non-negative int32
static int check_streams(int32_t first, int R, const char *what) {
    if (first < 0) return fail(GQ_ERR_INVALID_ARG, "%s: stream %d is negative", what, (int)first);
    if ((int64_t)first + (int64_t)R > 0x7fffffffll) return fail(GQ_ERR_INVALID_ARG, "%s: first stream %d + R = %d overflows int32", what, (int)first, R);
    return GQ_OK;
}

// rot: Hadamard::args(b), the fixed words of the descriptor, or gqx::Stepped / gqx::Streamed: the kernels then do not read them
template <class Coder, int SCALE, class Batch, class Rot>
static void launch_compress(const Batch *b, uint8_t *wire, float ef_scale, float *out, Rot rot, hipStream_t st) {
    const dim3 grid((unsigned)b->nitems), block(THREADS);
    if (!isnan(ef_scale))
        hipLaunchKernelGGL(HIP_KERNEL_NAME(compress_kernel<Coder, SCALE, true, Rot>), grid, block, 0, st, b->seg_table, b->item_seg, wire, out,
                           ef_scale, b->dense_table, b->ndense, rot);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(compress_kernel<Coder, SCALE, false, Rot>), grid, block, 0, st, b->seg_table, b->item_seg, wire, out,
                           0.0f, b->dense_table, b->ndense, rot);
}

template <class Lib, class Rot>
static void launch_compress(const typename Lib::Batch *b, uint8_t *wire, float ef_scale, float *out, Rot rot, hipStream_t st) {
    Lib::with_coder(b, [&](auto coder) {
        using Coder = decltype(coder);
        if (b->scale_mode == UNBIASED)
            launch_compress<Coder, UNBIASED>(b, wire, ef_scale, out, rot, st);
        else
            launch_compress<Coder, MSE>(b, wire, ef_scale, out, rot, st);
    });
}

// the two entry points of a launch kind; stepped: `rotation` is checked and the descriptor's sign words are not read;
// sigma (stepped only): the stream of a *_streams call, null otherwise
template <class Lib>
static int compress(const char *what, const typename Lib::Batch *b, uint8_t *wire, float ef_scale, float *out, bool stepped,
                    const uint64_t *rotation, void *stream, const int32_t *sigma = nullptr) {
    int rc = check_batch<Lib>(b, what, true);
    if (rc == GQ_OK && stepped) rc = check_rotation(rotation, what);
    if (rc == GQ_OK && sigma) rc = check_streams(*sigma, 0, what);
    if (rc != GQ_OK) return rc;
    if (!wire || (reinterpret_cast<uintptr_t>(wire) & 15) != 0)
        return fail(GQ_ERR_INVALID_ARG, "%s: the wire must be a 16-byte aligned device buffer", what);
    if ((reinterpret_cast<uintptr_t>(out) & 3) != 0) return fail(GQ_ERR_INVALID_ARG, "%s: out must be 4-byte aligned", what);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (sigma)
        launch_compress<Lib>(b, wire, ef_scale, out, gqx::Streamed{rotation, (uint32_t)*sigma}, st);
    else if (stepped)
        launch_compress<Lib>(b, wire, ef_scale, out, gqx::Stepped{rotation}, st);
    else
        launch_compress<Lib>(b, wire, ef_scale, out, Hadamard::args(b), st);
    GQL_CHECK_LAUNCH(what);
    return GQ_OK;
}

template <class Lib>
static int decode_sum(const char *what, const typename Lib::Batch *b, const uint8_t *gathered, int64_t user_stride_bytes, int R, float *out,
                      int plain, bool stepped, const uint64_t *rotation, void *stream, const int32_t *first = nullptr) {
    int rc = check_batch<Lib>(b, what, false);
    if (rc == GQ_OK && stepped) rc = check_rotation(rotation, what);
    if (rc != GQ_OK) return rc;
    if (!gathered || !out) return fail(GQ_ERR_INVALID_ARG, "%s: null pointer", what);
    if (R < 1 || (R > 1 && user_stride_bytes < 0))
        return fail(GQ_ERR_INVALID_ARG, "%s: R = %d, user stride %lld", what, R, (long long)user_stride_bytes);
    if (plain && R != 1) return fail(GQ_ERR_INVALID_ARG, "%s: plain is the decode of ONE payload, R = %d", what, R);
    if ((reinterpret_cast<uintptr_t>(out) & 3) != 0) return fail(GQ_ERR_INVALID_ARG, "%s: out must be 4-byte aligned", what);
    if (first && (rc = check_streams(*first, R, what)) != GQ_OK) return rc;
    const dim3 grid((unsigned)b->nitems), block(THREADS);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    Lib::with_coder(b, [&](auto coder) {
        using Coder = decltype(coder);
        if (first)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(decode_streams_kernel<Coder>), grid, block, 0, st, b->seg_table, b->item_seg, gathered,
                               user_stride_bytes, R, out, plain ? 1 : 0, rotation, (uint32_t)*first);
        else if (stepped)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(decode_kernel<Coder, gqx::Stepped>), grid, block, 0, st, b->seg_table, b->item_seg, gathered,
                               user_stride_bytes, R, out, plain ? 1 : 0, gqx::Stepped{rotation});
        else
            hipLaunchKernelGGL(HIP_KERNEL_NAME(decode_kernel<Coder, Signs>), grid, block, 0, st, b->seg_table, b->item_seg, gathered,
                               user_stride_bytes, R, out, plain ? 1 : 0, Hadamard::args(b));
    });
    GQL_CHECK_LAUNCH(what);
    return GQ_OK;
}

}  // namespace gqr
