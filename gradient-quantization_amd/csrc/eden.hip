// The rotated 2-, 3- and 4-bit compressor (EDEN), multi-tensor (segment table) form -- libgq_eden.so
// (include/gq_eden.h: the contract, to the bit; tests/eden_contract.py restates it in numpy).
//
// The kernels follow csrc/drive.hip point by point: one workgroup per item of GQ_MX_ITEM_ELEMS = 4096 elements, two steps of 2048,
// a lane owns eight consecutive elements (two float4 loads; scalar loads at a tensor's ragged end or on a misaligned view) and a
// 32-lane half a block of 256.  The rotation is csrc/hadamard.hpp's, shared with mxr.hip and drive.hip.  Everything between the
// loads and the stores stays in registers: no LDS is allocated, no barrier, no scratch.
// compress  load (+ error feedback) -> sign flip -> 8 stages -> * 2^-4 = x'.  Q = the tree sum of x' * x' (three levels inside the
//           lane, five across the half: lane xor 1, 2, 4, 8, 16 -- an addition commutes, so every lane of the half ends with the
//           block's sum), sigma = sqrtf(Q * 2^-8), the thresholds t_i * sigma, then per element the magnitude index m by strict
//           compares in ascending order (the centroid c_m is picked along the way: selects, no table in memory).  A lane's eight
//           codes are b whole bytes.  P = the tree sum of |x'| * c_m and (mse) C2 = that of c_m * c_m, then ONE division.
//           b = 4: a lane's 4 code bytes leave as its own dword (a half's 128 bytes in one store).  b = 2, 3: three DPP moves
//           bring a quad's four words to its first lane, which stores the quad's 8 or 12 bytes.  Lane 0 of the half stores the
//           scale.  If `out` or error feedback is asked for: y = +-(S * c_m) -> 8 stages -> * 2^-4 -> sign flip -> out / w / err.
// decode    the same items and lanes; a lane reads its b code bytes and its block's scale of each of the R payloads in order
//           (aligned loads where the payloads are 4-byte aligned, bytes otherwise; b = 3 always reads bytes), adds +-(S * c_m) and
//           divides by R, then ONE inverse transform, then the store.
// The last block of a tensor is zero-padded and rotated like any other, so whether a lane takes part is a test on its BLOCK
// (blk < nb), uniform over the half, and the steps are left on workgroup-uniform tests only: no exchange sits under divergent
// control flow.  Loads and stores are masked per lane (e0 + k < n).
// Every launch's arguments depend on the layout alone, and there are no draws: both replay from a HIP graph as they are.
// stepped   the *_stepped entry points: the same bodies, with the lane's sign byte made once per launch from a device
//           { seed, step } pair (gqx::stepped_sign_byte) instead of from four words passed by value.  The pair's ADDRESS is the
//           launch argument: a replay rotates afresh once the step word has moved.
// streams   the *_streams entry points (SIGNS, PER STREAM), as in csrc/drive.hip.  compress is the stepped kernel with one more step
//           in its prelude: pair -> the stream's seed -> the lane's sign byte.  decode-mean is a body of its own: payload r goes
//           through its OWN inverse transform under stream first + r and the mean is taken in the gradient's domain.  The payload
//           loop is the outer one and the item's two steps the inner one, so a stream's sign byte is derived once per workgroup and
//           payload whatever R is; across payloads a lane keeps its 2 x 8 accumulators and nothing else.
#include <math.h>

#include "gq_eden.h"
#include "gq_lib_prelude.hpp"
#include "hadamard.hpp"

#define GQE_API extern "C" __attribute__((visibility("default")))

namespace gqe {

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
constexpr uint32_t QNAN = 0x7fc00000u;                // the scale of a block that is not finite
static_assert(GQ_EDEN_BLOCK == gqx::HAD_BLOCK && STEP % GQ_EDEN_BLOCK == 0 && GQ_MX_ITEM_ELEMS % STEP == 0, "a 32-lane half owns a block, an item is whole steps");
static_assert((STEP / GQ_EDEN_BLOCK) % 4 == 0, "a step holds whole 16-byte runs of scales: the scales' pad lies in the step of the last block");
static_assert(sizeof(gq_eden_batch) == 88, "gq_eden_batch: the layout the ctypes binding declares (gq_amd/native.py)");

// include/gq_eden.h's TABLES: L = 2^(B-1) magnitudes, L - 1 thresholds, by their bit patterns.  Every index is a constant once the
// loops are unrolled: the values are immediates, there is no table in memory.
template <int B>
struct Table {
    static constexpr int L = 1 << (B - 1);
    static constexpr uint32_t MASK = (1u << B) - 1u;
    static __device__ __forceinline__ float c(int i) {
        constexpr uint32_t C2[2] = {0x3ee7d2c9u, 0x3fc1555du};
        constexpr uint32_t C3[4] = {0x3e7af9f8u, 0x3f418990u, 0x3fac0538u, 0x4009b97au};
        constexpr uint32_t C4[8] = {0x3e0379fdu, 0x3ec6ae44u, 0x3f28215eu, 0x3f713d39u, 0x3fa0cc2fu, 0x3fcf1c25u, 0x40046ac7u, 0x402ee2bfu};
        return __uint_as_float(B == 2 ? C2[i & 1] : B == 3 ? C3[i & 3] : C4[i & 7]);
    }
    static __device__ __forceinline__ float t(int i) {
        constexpr uint32_t T2[1] = {0x3f7b4a0fu};
        constexpr uint32_t T3[3] = {0x3f002407u, 0x3f866500u, 0x3fdfbc17u};
        constexpr uint32_t T4[7] = {0x3e8435a1u, 0x3f05bc40u, 0x3f4caf4bu, 0x3f8cb566u, 0x3fb7f42au, 0x3febf8dau, 0x4019a6c3u};
        return __uint_as_float(B == 2 ? T2[0] : B == 3 ? T3[i < 3 ? i : 2] : T4[i < 7 ? i : 6]);
    }
    // c_m of a magnitude index read off the wire: selects on its bits
    static __device__ __forceinline__ float mag(uint32_t m) {
        if (B == 2) return (m & 1u) ? c(1) : c(0);
        if (B == 3) return (m & 2u) ? ((m & 1u) ? c(3) : c(2)) : ((m & 1u) ? c(1) : c(0));
        const float lo = (m & 2u) ? ((m & 1u) ? c(3) : c(2)) : ((m & 1u) ? c(1) : c(0));
        const float hi = (m & 2u) ? ((m & 1u) ? c(7) : c(6)) : ((m & 1u) ? c(5) : c(4));
        return (m & 4u) ? hi : lo;
    }
};

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
template <int B, int SCALE, bool EF, class Rot>
__global__ __launch_bounds__(THREADS) void eden_compress_kernel(const int64_t *__restrict__ seg_table, const int32_t *__restrict__ item_seg,
                                                                uint8_t *__restrict__ wire, float *__restrict__ out, float ef_scale,
                                                                const int64_t *__restrict__ dense_table, int ndense, Rot signs) {
    using T = Table<B>;
    constexpr int CODE_BYTES = GQ_EDEN_BLOCK * B / 8;      // a block's code bytes: B of them per lane
    copy_dense<THREADS>(dense_table, ndense, wire);
    const int64_t item = blockIdx.x;
    const int seg = item_seg[item];
    const int64_t *rec = seg_table + 8 * (int64_t)seg;
    const int64_t n = rec[1];
    const int64_t nb = (n + GQ_EDEN_BLOCK - 1) / GQ_EDEN_BLOCK, nb_pad = (nb + 3) / 4 * 4;
    float *v = reinterpret_cast<float *>(rec[0]);
    float *err = EF ? reinterpret_cast<float *>(rec[7]) : nullptr;
    uint8_t *codes = wire + rec[3];
    float *scales = reinterpret_cast<float *>(codes + nb * CODE_BYTES);
    float *o = out ? out + rec[5] : nullptr;
    const uint32_t l = threadIdx.x & 31u;      // the lane's place in the half that owns its block
    const Hadamard rotation(signs);
    const int64_t base = (item - rec[2]) * GQ_MX_ITEM_ELEMS;
    for (int s = 0; s < STEPS; ++s) {
        if (base + (int64_t)s * STEP >= nb * GQ_EDEN_BLOCK) break;      // (uniform over the workgroup)
        const int64_t e0 = base + (int64_t)s * STEP + (int64_t)threadIdx.x * PER_LANE;      // this lane's first element
        const int64_t blk = e0 / GQ_EDEN_BLOCK;                                             // (uniform over the half)
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
        float a[PER_LANE], q[PER_LANE];
#pragma unroll
        for (int k = 0; k < PER_LANE; ++k) {
            a[k] = __uint_as_float(__float_as_uint(x[k]) & 0x7fffffffu);
            q[k] = x[k] * x[k];      // (one multiplication; never fused into the tree's additions)
        }
        const float Q = block_sum(q);
        const float sigma = sqrtf(Q * 0.00390625f);      // one multiplication by 2^-8, one correctly rounded square root
        float th[T::L > 1 ? T::L - 1 : 1];
#pragma unroll
        for (int i = 0; i < T::L - 1; ++i) th[i] = T::t(i) * sigma;
        uint32_t word = 0;      // the lane's eight codes: B bytes
        float c[PER_LANE], pc[PER_LANE], cc[PER_LANE];
#pragma unroll
        for (int k = 0; k < PER_LANE; ++k) {
            uint32_t m = 0;
            float ck = T::c(0);
#pragma unroll
            for (int i = 0; i < T::L - 1; ++i) {      // the thresholds ascend: the last one passed is the count of those passed
                const bool gt = a[k] > th[i];
                m = gt ? (uint32_t)(i + 1) : m;
                ck = gt ? T::c(i + 1) : ck;
            }
            c[k] = ck;
            word |= (m | ((__float_as_uint(x[k]) >> 31) << (B - 1))) << (B * k);
            pc[k] = a[k] * ck;
            cc[k] = ck * ck;
        }
        const float P = block_sum(pc);
        float S;
        if (SCALE == GQ_EDEN_UNBIASED) {
            S = Q / P;
        } else {
            const float C2 = block_sum(cc);
            S = P / C2;
        }
        S = P == 0.0f ? 0.0f : S;
        S = (__float_as_uint(P) & 0x7fffffffu) >= 0x7f800000u ? __uint_as_float(QNAN) : S;      // an infinity or a NaN among the x'
        // o || ef is uniform over the workgroup, so the inverse's exchanges run in every lane
        if (o || ef) {
            float d[PER_LANE];
#pragma unroll
            for (int k = 0; k < PER_LANE; ++k) {
                const float y = S * c[k];
                d[k] = __uint_as_float(__float_as_uint(y) ^ (__float_as_uint(x[k]) & 0x80000000u));
            }
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
        // the block's 32 B code bytes, lane l's at byte B l
        uint8_t *cp = codes + blk * CODE_BYTES + B * l;
        if (B == 4) {
            if (blk < nb) *reinterpret_cast<uint32_t *>(cp) = word;      // a half's 128 bytes in one store
        } else {
            // the words of the quad's lanes + 1, + 2, + 3 in its first lane, which stores the quad's 4 B bytes (at a multiple of 4 B)
            const uint32_t w1 = lane_xor_bits<1>(word), w2 = lane_xor_bits<2>(word), w3 = lane_xor_bits<2>(w1);
            if (blk < nb && (l & 3u) == 0) {
                if (B == 2) {
                    *reinterpret_cast<uint2 *>(cp) = make_uint2(word | (w1 << 16), w2 | (w3 << 16));
                } else {
                    uint32_t *c32 = reinterpret_cast<uint32_t *>(cp);
                    c32[0] = word | (w1 << 24);
                    c32[1] = (w1 >> 8) | (w2 << 16);
                    c32[2] = (w2 >> 16) | (w3 << 8);
                }
            }
        }
        // the scale, and +0 in the scales' pad (which lies in the step of the last block)
        if (l == 0 && blk < nb_pad) scales[blk] = blk < nb ? S : 0.0f;
    }
}

template <int B, class Rot>
__global__ __launch_bounds__(THREADS) void eden_decode_kernel(const int64_t *__restrict__ seg_table, const int32_t *__restrict__ item_seg,
                                                              const uint8_t *__restrict__ gathered, int64_t stride, int R,
                                                              float *__restrict__ out, int plain, Rot signs) {
    using T = Table<B>;
    constexpr int CODE_BYTES = GQ_EDEN_BLOCK * B / 8;
    const int64_t item = blockIdx.x;
    const int seg = item_seg[item];
    const int64_t *rec = seg_table + 8 * (int64_t)seg;
    const int64_t n = rec[1], off = rec[3];
    const int64_t nb = (n + GQ_EDEN_BLOCK - 1) / GQ_EDEN_BLOCK;
    float *o = out + rec[5];
    const int64_t base = (item - rec[2]) * GQ_MX_ITEM_ELEMS;
    const bool direct = plain != 0;      // (the host side: R == 1)
    const float fR = (float)R;
    const Hadamard rotation(signs);
    // (wire offsets are multiples of 16 and the codes of a section a multiple of 16 bytes: the payloads' own alignment decides)
    const bool words = ((reinterpret_cast<uintptr_t>(gathered) | (uintptr_t)(R > 1 ? stride : 0)) & 3u) == 0;
    for (int s = 0; s < STEPS; ++s) {
        if (base + (int64_t)s * STEP >= n) break;      // (uniform over the workgroup)
        const int64_t e0 = base + (int64_t)s * STEP + (int64_t)threadIdx.x * PER_LANE;
        const int64_t blk = e0 / GQ_EDEN_BLOCK;
        const bool live = blk < nb;      // (uniform over the half; the elements behind n - 1 of a last block are decoded too)
        float acc[PER_LANE];
#pragma unroll
        for (int k = 0; k < PER_LANE; ++k) acc[k] = 0.0f;
        const uint8_t *p = gathered + off;
        for (int r = 0; r < R && live; ++r, p += stride) {
            const uint8_t *cp = p + (e0 / PER_LANE) * B;      // this lane's B code bytes
            const uint8_t *sp = p + nb * CODE_BYTES + 4 * blk;
            uint32_t word = 0, sbits = 0;
            if (words) {
                sbits = *reinterpret_cast<const uint32_t *>(sp);
                if (B == 4) word = *reinterpret_cast<const uint32_t *>(cp);
                if (B == 2) word = *reinterpret_cast<const uint16_t *>(cp);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) sbits |= (uint32_t)sp[k] << (8 * k);
            }
            if (B == 3 || !words) {
#pragma unroll
                for (int k = 0; k < B; ++k) word |= (uint32_t)cp[k] << (8 * k);
            }
            const float S = __uint_as_float(sbits);
#pragma unroll
            for (int k = 0; k < PER_LANE; ++k) {
                const uint32_t code = (word >> (B * k)) & T::MASK;
                const float ym = S * T::mag(code);      // (one multiplication)
                const float y = __uint_as_float(__float_as_uint(ym) ^ ((code >> (B - 1)) << 31));
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
template <int B>
__global__ __launch_bounds__(THREADS) void eden_decode_streams_kernel(const int64_t *__restrict__ seg_table, const int32_t *__restrict__ item_seg,
                                                                      const uint8_t *__restrict__ gathered, int64_t stride, int R,
                                                                      float *__restrict__ out, int plain, const uint64_t *__restrict__ pair,
                                                                      uint32_t first) {
    using T = Table<B>;
    constexpr int CODE_BYTES = GQ_EDEN_BLOCK * B / 8;
    const int64_t item = blockIdx.x;
    const int seg = item_seg[item];
    const int64_t *rec = seg_table + 8 * (int64_t)seg;
    const int64_t n = rec[1], off = rec[3];
    const int64_t nb = (n + GQ_EDEN_BLOCK - 1) / GQ_EDEN_BLOCK;
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
                const int64_t blk = e0 / GQ_EDEN_BLOCK;
                uint32_t word = 0, sbits = 0;
                if (blk < nb) {      // (uniform over the half: loads only, no exchange in here)
                    const uint8_t *cp = p + (e0 / PER_LANE) * B;      // this lane's B code bytes
                    const uint8_t *sp = p + nb * CODE_BYTES + 4 * blk;
                    if (words) {
                        sbits = *reinterpret_cast<const uint32_t *>(sp);
                        if (B == 4) word = *reinterpret_cast<const uint32_t *>(cp);
                        if (B == 2) word = *reinterpret_cast<const uint16_t *>(cp);
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; ++k) sbits |= (uint32_t)sp[k] << (8 * k);
                    }
                    if (B == 3 || !words) {
#pragma unroll
                        for (int k = 0; k < B; ++k) word |= (uint32_t)cp[k] << (8 * k);
                    }
                }
                const float S = __uint_as_float(sbits);
                float y[PER_LANE];
#pragma unroll
                for (int k = 0; k < PER_LANE; ++k) {
                    const uint32_t code = (word >> (B * k)) & T::MASK;
                    const float ym = S * T::mag(code);      // (one multiplication)
                    y[k] = __uint_as_float(__float_as_uint(ym) ^ ((code >> (B - 1)) << 31));
                }
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

static int check_batch(const gq_eden_batch *b, const char *what, bool compress) {
    if (!b || b->struct_bytes != sizeof(gq_eden_batch)) return fail(GQ_ERR_INVALID_ARG, "%s: descriptor missing or of another size", what);
    if (b->bits < GQ_EDEN_MIN_BITS || b->bits > GQ_EDEN_MAX_BITS)
        return fail(GQ_ERR_INVALID_ARG, "%s: bits %d (2, 3 or 4; one bit is libgq_drive.so)", what, b->bits);
    if (b->scale_mode != GQ_EDEN_UNBIASED && b->scale_mode != GQ_EDEN_MSE)
        return fail(GQ_ERR_INVALID_ARG, "%s: scale_mode %d (GQ_EDEN_UNBIASED or GQ_EDEN_MSE)", what, b->scale_mode);
    if (b->nseg < 1 || b->nitems < 1 || b->nitems > 0x7fffffff || b->ndense < 0)
        return fail(GQ_ERR_INVALID_ARG, "%s: bad sizes (nseg %d, nitems %lld, ndense %d)", what, b->nseg, (long long)b->nitems, b->ndense);
    if (!b->seg_table || !b->item_seg) return fail(GQ_ERR_INVALID_ARG, "%s: null table", what);
    if (compress && b->ndense > 0 && !b->dense_table) return fail(GQ_ERR_INVALID_ARG, "%s: null dense table", what);
    return GQ_OK;
}

// rot: Hadamard::args(b), the fixed words of the descriptor, or gqx::Stepped: the kernels then do not read them
template <int B, int SCALE, class Rot>
static void launch_compress(const gq_eden_batch *b, uint8_t *wire, float ef_scale, float *out, Rot rot, hipStream_t st) {
    const dim3 grid((unsigned)b->nitems), block(THREADS);
    if (!isnan(ef_scale))
        hipLaunchKernelGGL(HIP_KERNEL_NAME(eden_compress_kernel<B, SCALE, true, Rot>), grid, block, 0, st, b->seg_table, b->item_seg, wire, out,
                           ef_scale, b->dense_table, b->ndense, rot);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(eden_compress_kernel<B, SCALE, false, Rot>), grid, block, 0, st, b->seg_table, b->item_seg, wire, out,
                           0.0f, b->dense_table, b->ndense, rot);
}

template <int B, class Rot>
static void launch_compress(const gq_eden_batch *b, uint8_t *wire, float ef_scale, float *out, Rot rot, hipStream_t st) {
    if (b->scale_mode == GQ_EDEN_UNBIASED)
        launch_compress<B, GQ_EDEN_UNBIASED>(b, wire, ef_scale, out, rot, st);
    else
        launch_compress<B, GQ_EDEN_MSE>(b, wire, ef_scale, out, rot, st);
}

template <class Rot>
static void launch_compress(const gq_eden_batch *b, uint8_t *wire, float ef_scale, float *out, Rot rot, hipStream_t st) {
    if (b->bits == 2)
        launch_compress<2>(b, wire, ef_scale, out, rot, st);
    else if (b->bits == 3)
        launch_compress<3>(b, wire, ef_scale, out, rot, st);
    else
        launch_compress<4>(b, wire, ef_scale, out, rot, st);
}

template <int B, class Rot>
static void launch_decode(const gq_eden_batch *b, const uint8_t *gathered, int64_t stride, int R, float *out, int plain, Rot rot, hipStream_t st) {
    const dim3 grid((unsigned)b->nitems), block(THREADS);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(eden_decode_kernel<B, Rot>), grid, block, 0, st, b->seg_table, b->item_seg, gathered, stride, R, out, plain,
                       rot);
}

template <class Rot>
static void launch_decode(const gq_eden_batch *b, const uint8_t *gathered, int64_t stride, int R, float *out, int plain, Rot rot, hipStream_t st) {
    if (b->bits == 2)
        launch_decode<2>(b, gathered, stride, R, out, plain, rot, st);
    else if (b->bits == 3)
        launch_decode<3>(b, gathered, stride, R, out, plain, rot, st);
    else
        launch_decode<4>(b, gathered, stride, R, out, plain, rot, st);
}

static void launch_decode_streams(const gq_eden_batch *b, const uint8_t *gathered, int64_t stride, int R, float *out, int plain,
                                  const uint64_t *pair, uint32_t first, hipStream_t st) {
    const dim3 grid((unsigned)b->nitems), block(THREADS);
    if (b->bits == 2)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(eden_decode_streams_kernel<2>), grid, block, 0, st, b->seg_table, b->item_seg, gathered, stride, R, out,
                           plain, pair, first);
    else if (b->bits == 3)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(eden_decode_streams_kernel<3>), grid, block, 0, st, b->seg_table, b->item_seg, gathered, stride, R, out,
                           plain, pair, first);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(eden_decode_streams_kernel<4>), grid, block, 0, st, b->seg_table, b->item_seg, gathered, stride, R, out,
                           plain, pair, first);
}

// SIGNS, PER STREAM: streams first ... first + R - 1 are non-negative int32
static int check_streams(int32_t first, int R, const char *what) {
    if (first < 0) return fail(GQ_ERR_INVALID_ARG, "%s: stream %d is negative", what, (int)first);
    if ((int64_t)first + (int64_t)R > 0x7fffffffll) return fail(GQ_ERR_INVALID_ARG, "%s: first stream %d + R = %d overflows int32", what, (int)first, R);
    return GQ_OK;
}

// the two entry points of a launch kind; stepped: `rotation` is checked and the descriptor's sign words are not read;
// sigma (stepped only): the stream of a *_streams call, null otherwise
static int compress(const char *what, const gq_eden_batch *b, uint8_t *wire, float ef_scale, float *out, bool stepped, const uint64_t *rotation,
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

static int decode_sum(const char *what, const gq_eden_batch *b, const uint8_t *gathered, int64_t user_stride_bytes, int R, float *out, int plain,
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
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (first)
        launch_decode_streams(b, gathered, user_stride_bytes, R, out, plain ? 1 : 0, rotation, (uint32_t)*first, st);
    else if (stepped)
        launch_decode(b, gathered, user_stride_bytes, R, out, plain ? 1 : 0, gqx::Stepped{rotation}, st);
    else
        launch_decode(b, gathered, user_stride_bytes, R, out, plain ? 1 : 0, Hadamard::args(b), st);
    GQL_CHECK_LAUNCH(what);
    return GQ_OK;
}

}  // namespace gqe

GQE_API int gq_eden_abi_version(void) { return GQ_EDEN_ABI_VERSION; }

GQE_API const char *gq_eden_last_error(void) { return gqe::err_buf; }

GQE_API int gq_eden_compress_batched(const gq_eden_batch *b, uint8_t *wire, float ef_scale, float *out, void *stream) {
    return gqe::compress("gq_eden_compress_batched", b, wire, ef_scale, out, false, nullptr, stream);
}

GQE_API int gq_eden_compress_batched_stepped(const gq_eden_batch *b, const uint64_t *rotation, uint8_t *wire, float ef_scale, float *out,
                                             void *stream) {
    return gqe::compress("gq_eden_compress_batched_stepped", b, wire, ef_scale, out, true, rotation, stream);
}

GQE_API int gq_eden_decode_sum_batched(const gq_eden_batch *b, const uint8_t *gathered, int64_t user_stride_bytes, int R, float *out, int plain,
                                       void *stream) {
    return gqe::decode_sum("gq_eden_decode_sum_batched", b, gathered, user_stride_bytes, R, out, plain, false, nullptr, stream);
}

GQE_API int gq_eden_decode_sum_batched_stepped(const gq_eden_batch *b, const uint64_t *rotation, const uint8_t *gathered,
                                               int64_t user_stride_bytes, int R, float *out, int plain, void *stream) {
    return gqe::decode_sum("gq_eden_decode_sum_batched_stepped", b, gathered, user_stride_bytes, R, out, plain, true, rotation, stream);
}

GQE_API int gq_eden_compress_batched_streams(const gq_eden_batch *b, const uint64_t *rotation, int32_t stream, uint8_t *wire, float ef_scale,
                                             float *out, void *stream_handle) {
    return gqe::compress("gq_eden_compress_batched_streams", b, wire, ef_scale, out, true, rotation, stream_handle, &stream);
}

GQE_API int gq_eden_decode_sum_batched_streams(const gq_eden_batch *b, const uint64_t *rotation, int32_t first_stream, const uint8_t *gathered,
                                               int64_t user_stride_bytes, int R, float *out, int plain, void *stream_handle) {
    return gqe::decode_sum("gq_eden_decode_sum_batched_streams", b, gathered, user_stride_bytes, R, out, plain, true, rotation, stream_handle,
                           &first_stream);
}
