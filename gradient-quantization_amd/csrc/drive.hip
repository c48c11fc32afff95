// The rotated 1-bit compressor (DRIVE), multi-tensor (segment table) form -- libgq_drive.so
// (include/gq_drive.h: the contract, to the bit; tests/drive_contract.py restates it in numpy).
//
// The kernels have the shape of csrc/mx_kernels.hpp's: one workgroup per item of GQ_MX_ITEM_ELEMS = 4096 elements, two steps of
// 2048, a lane owns eight consecutive elements (two float4 loads; scalar loads at a tensor's ragged end or on a misaligned view)
// and a 32-lane half a block of 256.  The rotation is csrc/hadamard.hpp's, shared with mxr.hip.  Everything between the loads and
// the stores stays in registers: no LDS is allocated, no barrier, no scratch.
// compress  load (+ error feedback) -> sign flip -> 8 stages -> * 2^-4 = x'.  A lane's eight codes (the sign bits of x') are one
//           byte.  |x'| and x' * x' are summed as the contract's balanced tree: three levels inside the lane, five across the
//           half (lane xor 1, 2, 4, 8, 16: after them every lane of the half holds the block's sum -- an addition commutes, so the
//           lane on either side of a pair gets the same bits), then ONE division.  The bytes of a quad are gathered into a dword
//           by two DPP moves and the dwords of four quads into 16 bytes by three swizzles: a block's 32 code bytes leave as two
//           16-byte stores; lane 0 of the half stores the scale.  If `out` or error feedback is asked for: y = +-S -> 8 stages ->
//           * 2^-4 -> sign flip -> out / w / err = w - D.
// decode    the same items and lanes; a lane reads its code byte and its block's scale of each of the R payloads in order
//           (an aligned dword where the payloads are 4-byte aligned, bytes otherwise), adds +-S and divides by R, then ONE
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
#include <math.h>

#include "gq_drive.h"
#include "gq_lib_prelude.hpp"
#include "hadamard.hpp"

#define GQD_API extern "C" __attribute__((visibility("default")))

namespace gqd {

using gql::aligned16;
using gql::copy_dense;
using gql::err_buf;
using gql::check_rotation;
using gql::fail;
using gqx::Hadamard;
using gqx::lane_xor;
using gqx::Signs;

constexpr int THREADS = 256;
constexpr int PER_LANE = gqx::HAD_PER_LANE;          // elements of a lane: a 32-lane half owns a block of 256
constexpr int STEP = THREADS * PER_LANE;              // elements of a workgroup-wide step: 8 blocks
constexpr int STEPS = GQ_MX_ITEM_ELEMS / STEP;
constexpr int CODE_BYTES = GQ_DRIVE_BLOCK / 8;        // a block's code bytes
constexpr uint32_t QNAN = 0x7fc00000u;                // the scale of a block that is not finite
static_assert(GQ_DRIVE_BLOCK == gqx::HAD_BLOCK && STEP % GQ_DRIVE_BLOCK == 0 && GQ_MX_ITEM_ELEMS % STEP == 0, "a 32-lane half owns a block, an item is whole steps");
static_assert((STEP / GQ_DRIVE_BLOCK) % 4 == 0, "a step holds whole 16-byte runs of scales: the scales' pad lies in the step of the last block");
static_assert(sizeof(gq_drive_batch) == 80, "gq_drive_batch: the layout the ctypes binding declares (gq_amd/native.py)");

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

__device__ __forceinline__ void load8(const float *p, float (&w)[PER_LANE]) {
    const float4 a0 = *reinterpret_cast<const float4 *>(p), a1 = *reinterpret_cast<const float4 *>(p + 4);
    w[0] = a0.x, w[1] = a0.y, w[2] = a0.z, w[3] = a0.w, w[4] = a1.x, w[5] = a1.y, w[6] = a1.z, w[7] = a1.w;
}

__device__ __forceinline__ void store8(float *p, const float (&f)[PER_LANE]) {
    *reinterpret_cast<float4 *>(p) = make_float4(f[0], f[1], f[2], f[3]);
    *reinterpret_cast<float4 *>(p + 4) = make_float4(f[4], f[5], f[6], f[7]);
}

// Rot: how the launch is told its rotation -- gqx::Signs (the four words, by value) or gqx::Stepped (the address of a device
// { seed, step } pair): the only difference between a fixed and a stepped launch is how `rotation` below is built
template <int SCALE, bool EF, class Rot>
__global__ __launch_bounds__(THREADS) void drive_compress_kernel(const int64_t *__restrict__ seg_table, const int32_t *__restrict__ item_seg,
                                                                 uint8_t *__restrict__ wire, float *__restrict__ out, float ef_scale,
                                                                 const int64_t *__restrict__ dense_table, int ndense, Rot signs) {
    copy_dense<THREADS>(dense_table, ndense, wire);
    const int64_t item = blockIdx.x;
    const int seg = item_seg[item];
    const int64_t *rec = seg_table + 8 * (int64_t)seg;
    const int64_t n = rec[1];
    const int64_t nb = (n + GQ_DRIVE_BLOCK - 1) / GQ_DRIVE_BLOCK, nb_pad = (nb + 3) / 4 * 4;
    float *v = reinterpret_cast<float *>(rec[0]);
    float *err = EF ? reinterpret_cast<float *>(rec[7]) : nullptr;
    uint8_t *codes = wire + rec[3];
    float *scales = reinterpret_cast<float *>(codes + nb * CODE_BYTES);
    float *o = out ? out + rec[5] : nullptr;
    const uint32_t l = threadIdx.x & 31u;      // the lane's place in the half that owns its block
    const Hadamard rotation(signs);
    const int64_t base = (item - rec[2]) * GQ_MX_ITEM_ELEMS;
    for (int s = 0; s < STEPS; ++s) {
        if (base + (int64_t)s * STEP >= nb * GQ_DRIVE_BLOCK) break;      // (uniform over the workgroup)
        const int64_t e0 = base + (int64_t)s * STEP + (int64_t)threadIdx.x * PER_LANE;      // this lane's first element
        const int64_t blk = e0 / GQ_DRIVE_BLOCK;                                            // (uniform over the half)
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
        const gqx::HadLane &x = rotation.forward(w, xbuf, true);      // x': every block is rotated, the zero-padded last one too
        uint32_t byte = 0;
        float a[PER_LANE], q[PER_LANE];
#pragma unroll
        for (int k = 0; k < PER_LANE; ++k) {
            const uint32_t xb = __float_as_uint(x[k]);
            byte |= (xb >> 31) << k;
            a[k] = __uint_as_float(xb & 0x7fffffffu);
            q[k] = x[k] * x[k];      // (one multiplication; never fused into the tree's additions)
        }
        const float L1 = block_sum(a);
        float S;
        if (SCALE == GQ_DRIVE_UNBIASED) {
            const float Q = block_sum(q);
            S = Q / L1;
        } else {
            S = L1 / 256.0f;
        }
        S = L1 == 0.0f ? 0.0f : S;
        S = (__float_as_uint(L1) & 0x7fffffffu) >= 0x7f800000u ? __uint_as_float(QNAN) : S;      // an infinity or a NaN among the x'
        // o || ef is uniform over the workgroup, so the inverse's exchanges run in every lane
        if (o || ef) {
            float d[PER_LANE];
            const uint32_t sbits = __float_as_uint(S);
#pragma unroll
            for (int k = 0; k < PER_LANE; ++k) d[k] = __uint_as_float(sbits ^ (((byte >> k) & 1u) << 31));
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
        // the block's 32 code bytes, lane l's at byte l: a quad's four into a little-endian dword, four quads' dwords into 16 bytes
        uint32_t dw = byte << (8 * (l & 3u));
        dw |= lane_xor_bits<1>(dw);
        dw |= lane_xor_bits<2>(dw);
        const uint32_t d1 = lane_xor_bits<4>(dw), d2 = lane_xor_bits<8>(dw), d3 = lane_xor_bits<8>(d1);      // of the lanes + 4, + 8, + 12
        if (blk < nb && (l & 15u) == 0)
            *reinterpret_cast<uint4 *>(codes + blk * CODE_BYTES + l) = make_uint4(dw, d1, d2, d3);
        // the scale, and +0 in the scales' pad (which lies in the step of the last block)
        if (l == 0 && blk < nb_pad) scales[blk] = blk < nb ? S : 0.0f;
    }
}

template <class Rot>
__global__ __launch_bounds__(THREADS) void drive_decode_kernel(const int64_t *__restrict__ seg_table, const int32_t *__restrict__ item_seg,
                                                               const uint8_t *__restrict__ gathered, int64_t stride, int R,
                                                               float *__restrict__ out, int plain, Rot signs) {
    const int64_t item = blockIdx.x;
    const int seg = item_seg[item];
    const int64_t *rec = seg_table + 8 * (int64_t)seg;
    const int64_t n = rec[1], off = rec[3];
    const int64_t nb = (n + GQ_DRIVE_BLOCK - 1) / GQ_DRIVE_BLOCK;
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
        const int64_t blk = e0 / GQ_DRIVE_BLOCK;
        const bool live = blk < nb;      // (uniform over the half; the elements behind n - 1 of a last block are decoded too)
        float acc[PER_LANE];
#pragma unroll
        for (int k = 0; k < PER_LANE; ++k) acc[k] = 0.0f;
        const uint8_t *p = gathered + off;
        for (int r = 0; r < R && live; ++r, p += stride) {
            const uint32_t byte = p[e0 / PER_LANE];
            const uint8_t *sp = p + nb * CODE_BYTES + 4 * blk;
            uint32_t sbits = 0;
            if (words) {
                sbits = *reinterpret_cast<const uint32_t *>(sp);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) sbits |= (uint32_t)sp[k] << (8 * k);
            }
#pragma unroll
            for (int k = 0; k < PER_LANE; ++k) {
                const float y = __uint_as_float(sbits ^ (((byte >> k) & 1u) << 31));
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
__global__ __launch_bounds__(THREADS) void drive_decode_streams_kernel(const int64_t *__restrict__ seg_table, const int32_t *__restrict__ item_seg,
                                                                       const uint8_t *__restrict__ gathered, int64_t stride, int R,
                                                                       float *__restrict__ out, int plain, const uint64_t *__restrict__ pair,
                                                                       uint32_t first) {
    const int64_t item = blockIdx.x;
    const int seg = item_seg[item];
    const int64_t *rec = seg_table + 8 * (int64_t)seg;
    const int64_t n = rec[1], off = rec[3];
    const int64_t nb = (n + GQ_DRIVE_BLOCK - 1) / GQ_DRIVE_BLOCK;
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
                const int64_t blk = e0 / GQ_DRIVE_BLOCK;
                uint32_t byte = 0, sbits = 0;
                if (blk < nb) {      // (uniform over the half: loads only, no exchange in here)
                    byte = p[e0 / PER_LANE];
                    const uint8_t *sp = p + nb * CODE_BYTES + 4 * blk;
                    if (words) {
                        sbits = *reinterpret_cast<const uint32_t *>(sp);
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; ++k) sbits |= (uint32_t)sp[k] << (8 * k);
                    }
                }
                float y[PER_LANE];
#pragma unroll
                for (int k = 0; k < PER_LANE; ++k) y[k] = __uint_as_float(sbits ^ (((byte >> k) & 1u) << 31));
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

static int check_batch(const gq_drive_batch *b, const char *what, bool compress) {
    if (!b || b->struct_bytes != sizeof(gq_drive_batch)) return fail(GQ_ERR_INVALID_ARG, "%s: descriptor missing or of another size", what);
    if (b->scale_mode != GQ_DRIVE_UNBIASED && b->scale_mode != GQ_DRIVE_MSE)
        return fail(GQ_ERR_INVALID_ARG, "%s: scale_mode %d (GQ_DRIVE_UNBIASED or GQ_DRIVE_MSE)", what, b->scale_mode);
    if (b->nseg < 1 || b->nitems < 1 || b->nitems > 0x7fffffff || b->ndense < 0)
        return fail(GQ_ERR_INVALID_ARG, "%s: bad sizes (nseg %d, nitems %lld, ndense %d)", what, b->nseg, (long long)b->nitems, b->ndense);
    if (!b->seg_table || !b->item_seg) return fail(GQ_ERR_INVALID_ARG, "%s: null table", what);
    if (compress && b->ndense > 0 && !b->dense_table) return fail(GQ_ERR_INVALID_ARG, "%s: null dense table", what);
    return GQ_OK;
}

// rot: Hadamard::args(b), the fixed words of the descriptor, or gqx::Stepped: the kernels then do not read them
template <int SCALE, class Rot>
static void launch_compress(const gq_drive_batch *b, uint8_t *wire, float ef_scale, float *out, Rot rot, hipStream_t st) {
    const dim3 grid((unsigned)b->nitems), block(THREADS);
    if (!isnan(ef_scale))
        hipLaunchKernelGGL(HIP_KERNEL_NAME(drive_compress_kernel<SCALE, true, Rot>), grid, block, 0, st, b->seg_table, b->item_seg, wire, out,
                           ef_scale, b->dense_table, b->ndense, rot);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(drive_compress_kernel<SCALE, false, Rot>), grid, block, 0, st, b->seg_table, b->item_seg, wire, out,
                           0.0f, b->dense_table, b->ndense, rot);
}

template <class Rot>
static void launch_compress(const gq_drive_batch *b, uint8_t *wire, float ef_scale, float *out, Rot rot, hipStream_t st) {
    if (b->scale_mode == GQ_DRIVE_UNBIASED)
        launch_compress<GQ_DRIVE_UNBIASED>(b, wire, ef_scale, out, rot, st);
    else
        launch_compress<GQ_DRIVE_MSE>(b, wire, ef_scale, out, rot, st);
}

// SIGNS, PER STREAM: streams first ... first + R - 1 are non-negative int32
static int check_streams(int32_t first, int R, const char *what) {
    if (first < 0) return fail(GQ_ERR_INVALID_ARG, "%s: stream %d is negative", what, (int)first);
    if ((int64_t)first + (int64_t)R > 0x7fffffffll) return fail(GQ_ERR_INVALID_ARG, "%s: first stream %d + R = %d overflows int32", what, (int)first, R);
    return GQ_OK;
}

// the two entry points of a launch kind; stepped: `rotation` is checked and the descriptor's sign words are not read;
// sigma (stepped only): the stream of a *_streams call, null otherwise
static int compress(const char *what, const gq_drive_batch *b, uint8_t *wire, float ef_scale, float *out, bool stepped, const uint64_t *rotation,
                    void *stream, const int32_t *sigma = nullptr) {
    int rc = check_batch(b, what, true);
    if (rc == GQ_OK && stepped) rc = check_rotation(rotation, what);
    if (rc == GQ_OK && sigma) rc = check_streams(*sigma, 0, what);
    if (rc != GQ_OK) return rc;
    if (!wire || (reinterpret_cast<uintptr_t>(wire) & 15) != 0)
        return fail(GQ_ERR_INVALID_ARG, "%s: the wire must be a 16-byte aligned device buffer", what);
    if ((reinterpret_cast<uintptr_t>(out) & 3) != 0) return fail(GQ_ERR_INVALID_ARG, "%s: out must be 4-byte aligned", what);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (sigma)
        launch_compress(b, wire, ef_scale, out, gqx::Streamed{rotation, (uint32_t)*sigma}, st);
    else if (stepped)
        launch_compress(b, wire, ef_scale, out, gqx::Stepped{rotation}, st);
    else
        launch_compress(b, wire, ef_scale, out, Hadamard::args(b), st);
    GQL_CHECK_LAUNCH(what);
    return GQ_OK;
}

static int decode_sum(const char *what, const gq_drive_batch *b, const uint8_t *gathered, int64_t user_stride_bytes, int R, float *out, int plain,
                      bool stepped, const uint64_t *rotation, void *stream, const int32_t *first = nullptr) {
    int rc = check_batch(b, what, false);
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
    if (first)
        hipLaunchKernelGGL(drive_decode_streams_kernel, grid, block, 0, st, b->seg_table, b->item_seg, gathered, user_stride_bytes, R, out,
                           plain ? 1 : 0, rotation, (uint32_t)*first);
    else if (stepped)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(drive_decode_kernel<gqx::Stepped>), grid, block, 0, st, b->seg_table, b->item_seg, gathered,
                           user_stride_bytes, R, out, plain ? 1 : 0, gqx::Stepped{rotation});
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(drive_decode_kernel<Signs>), grid, block, 0, st, b->seg_table, b->item_seg, gathered,
                           user_stride_bytes, R, out, plain ? 1 : 0, Hadamard::args(b));
    GQL_CHECK_LAUNCH(what);
    return GQ_OK;
}

}  // namespace gqd

GQD_API int gq_drive_abi_version(void) { return GQ_DRIVE_ABI_VERSION; }

GQD_API const char *gq_drive_last_error(void) { return gqd::err_buf; }

GQD_API int gq_drive_compress_batched(const gq_drive_batch *b, uint8_t *wire, float ef_scale, float *out, void *stream) {
    return gqd::compress("gq_drive_compress_batched", b, wire, ef_scale, out, false, nullptr, stream);
}

GQD_API int gq_drive_compress_batched_stepped(const gq_drive_batch *b, const uint64_t *rotation, uint8_t *wire, float ef_scale, float *out,
                                              void *stream) {
    return gqd::compress("gq_drive_compress_batched_stepped", b, wire, ef_scale, out, true, rotation, stream);
}

GQD_API int gq_drive_decode_sum_batched(const gq_drive_batch *b, const uint8_t *gathered, int64_t user_stride_bytes, int R, float *out, int plain,
                                        void *stream) {
    return gqd::decode_sum("gq_drive_decode_sum_batched", b, gathered, user_stride_bytes, R, out, plain, false, nullptr, stream);
}

GQD_API int gq_drive_decode_sum_batched_stepped(const gq_drive_batch *b, const uint64_t *rotation, const uint8_t *gathered,
                                                int64_t user_stride_bytes, int R, float *out, int plain, void *stream) {
    return gqd::decode_sum("gq_drive_decode_sum_batched_stepped", b, gathered, user_stride_bytes, R, out, plain, true, rotation, stream);
}

GQD_API int gq_drive_compress_batched_streams(const gq_drive_batch *b, const uint64_t *rotation, int32_t stream, uint8_t *wire, float ef_scale,
                                              float *out, void *stream_handle) {
    return gqd::compress("gq_drive_compress_batched_streams", b, wire, ef_scale, out, true, rotation, stream_handle, &stream);
}

GQD_API int gq_drive_decode_sum_batched_streams(const gq_drive_batch *b, const uint64_t *rotation, int32_t first_stream, const uint8_t *gathered,
                                                int64_t user_stride_bytes, int R, float *out, int plain, void *stream_handle) {
    return gqd::decode_sum("gq_drive_decode_sum_batched_streams", b, gathered, user_stride_bytes, R, out, plain, true, rotation, stream_handle,
                           &first_stream);
}
