// The rotated 2-, 3- and 4-bit compressor (EDEN), multi-tensor (segment table) form -- libgq_eden.so
// (include/gq_eden.h: the contract, to the bit; tests/eden_contract.py restates it in numpy).
//
// The kernels and the host path are csrc/rotq_kernels.hpp's, shared with drive.hip and instantiated here with its Lloyd-Max coders
// (LloydMax<2>, <3>, <4>, below); the rotation is csrc/hadamard.hpp's, shared with mxr.hip; this file is the descriptor, its `bits`
// and the exported names.
#include <math.h>

#include "gq_eden.h"
#include "gq_lib_prelude.hpp"
#include "hadamard.hpp"
#include "rotq_kernels.hpp"

#define GQE_API extern "C" __attribute__((visibility("default")))

namespace gqe {

static_assert(GQ_EDEN_BLOCK == gqr::BLOCK && GQ_EDEN_UNBIASED == gqr::UNBIASED && GQ_EDEN_MSE == gqr::MSE,
              "csrc/rotq_kernels.hpp codes the blocks, and under the scale modes, of include/gq_eden.h");
static_assert(GQ_EDEN_MIN_BITS == 2 && GQ_EDEN_MAX_BITS == 4, "with_coder below: one coder per width");
static_assert(sizeof(gq_eden_batch) == 88, "gq_eden_batch: the layout the ctypes binding declares (gq_amd/native.py)");

using gqr::BLOCK;
using gqr::block_sum;
using gqr::lane_xor_bits;
using gqr::MSE;
using gqr::PER_LANE;
using gqr::QNAN;
using gqr::UNBIASED;
using gqx::HadLane;

// EDEN, B = 2, 3, 4: a code is the index of the nearest Lloyd-Max centroid of N(0, 1) with the sign on top, a lane's eight B whole
// bytes.  Q = the tree sum of x' * x', sigma = sqrtf(Q * 2^-8), the thresholds t_i * sigma, then per element the magnitude index m
// by strict compares in ascending order (the centroid c_m is picked along the way: selects, no table in memory).  P = the tree sum
// of |x'| * c_m and (mse) C2 = that of c_m * c_m; S = Q / P (unbiased) or P / C2 (mse).  B = 4: a lane's 4 code bytes leave as its
// own dword (a half's 128 bytes in one store).  B = 2, 3: three DPP moves bring a quad's four words to its first lane, which stores
// the quad's 8 or 12 bytes.  A decoded value is +-(S * c_m): one multiplication, then the sign.  The decodes read aligned words
// where the payloads are 4-byte aligned; B = 3 always reads bytes.
// include/gq_eden.h's TABLES: L = 2^(B-1) magnitudes, L - 1 thresholds, by their bit patterns.  Every index is a constant once the
// loops are unrolled: the values are immediates.
template <int B>
struct LloydMax {
    static constexpr int CODE_BYTES = BLOCK * B / 8;      // B of them per lane
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
    template <int SCALE>
    __device__ __forceinline__ static float encode(const HadLane &x, uint32_t &word, float (&cm)[PER_LANE]) {
        float a[PER_LANE], q[PER_LANE];
#pragma unroll
        for (int k = 0; k < PER_LANE; ++k) {
            a[k] = __uint_as_float(__float_as_uint(x[k]) & 0x7fffffffu);
            q[k] = x[k] * x[k];      // (one multiplication; never fused into the tree's additions)
        }
        const float Q = block_sum(q);
        const float sigma = sqrtf(Q * 0.00390625f);      // one multiplication by 2^-8, one correctly rounded square root
        float th[L > 1 ? L - 1 : 1];
#pragma unroll
        for (int i = 0; i < L - 1; ++i) th[i] = t(i) * sigma;
        uint32_t w = 0;      // the lane's eight codes: B bytes
        float pc[PER_LANE], cc[PER_LANE];
#pragma unroll
        for (int k = 0; k < PER_LANE; ++k) {
            uint32_t m = 0;
            float ck = c(0);
#pragma unroll
            for (int i = 0; i < L - 1; ++i) {      // the thresholds ascend: the last one passed is the count of those passed
                const bool gt = a[k] > th[i];
                m = gt ? (uint32_t)(i + 1) : m;
                ck = gt ? c(i + 1) : ck;
            }
            cm[k] = ck;
            w |= (m | ((__float_as_uint(x[k]) >> 31) << (B - 1))) << (B * k);
            pc[k] = a[k] * ck;
            cc[k] = ck * ck;
        }
        word = w;
        const float P = block_sum(pc);
        float S;
        if (SCALE == UNBIASED) {
            S = Q / P;
        } else {
            const float C2 = block_sum(cc);
            S = P / C2;
        }
        S = P == 0.0f ? 0.0f : S;
        return (__float_as_uint(P) & 0x7fffffffu) >= 0x7f800000u ? __uint_as_float(QNAN) : S;      // an infinity or a NaN among the x'
    }
    __device__ __forceinline__ static float decoded(float S, uint32_t, const float (&cm)[PER_LANE], const HadLane &x, int k) {
        const float y = S * cm[k];
        return __uint_as_float(__float_as_uint(y) ^ (__float_as_uint(x[k]) & 0x80000000u));
    }
    // lane l's B bytes at byte B l of the block
    __device__ __forceinline__ static void store(uint8_t *block, uint32_t l, bool live, uint32_t word) {
        uint8_t *cp = block + B * l;
        if (B == 4) {
            if (live) *reinterpret_cast<uint32_t *>(cp) = word;      // a half's 128 bytes in one store
        } else {
            // the words of the quad's lanes + 1, + 2, + 3 in its first lane, which stores the quad's 4 B bytes (at a multiple of 4 B)
            const uint32_t w1 = lane_xor_bits<1>(word), w2 = lane_xor_bits<2>(word), w3 = lane_xor_bits<2>(w1);
            if (live && (l & 3u) == 0) {
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
    }
    __device__ __forceinline__ static uint32_t load(const uint8_t *p, int64_t lane, bool words) {
        const uint8_t *cp = p + lane * B;      // this lane's B code bytes
        uint32_t word = 0;
        if (words) {
            if (B == 4) word = *reinterpret_cast<const uint32_t *>(cp);
            if (B == 2) word = *reinterpret_cast<const uint16_t *>(cp);
        }
        if (B == 3 || !words) {
#pragma unroll
            for (int k = 0; k < B; ++k) word |= (uint32_t)cp[k] << (8 * k);
        }
        return word;
    }
    __device__ __forceinline__ static float value(uint32_t word, uint32_t sbits, int k) {
        const uint32_t code = (word >> (B * k)) & MASK;
        const float ym = __uint_as_float(sbits) * mag(code);      // (one multiplication)
        return __uint_as_float(__float_as_uint(ym) ^ ((code >> (B - 1)) << 31));
    }
};

struct Lib {
    using Batch = gq_eden_batch;
    static constexpr const char *SCALE_MODES = "GQ_EDEN_UNBIASED or GQ_EDEN_MSE";
    static int check_own(const Batch *b, const char *what) {
        if (b->bits < GQ_EDEN_MIN_BITS || b->bits > GQ_EDEN_MAX_BITS)
            return gqr::fail(GQ_ERR_INVALID_ARG, "%s: bits %d (2, 3 or 4; one bit is libgq_drive.so)", what, b->bits);
        return GQ_OK;
    }
    template <class F>
    static void with_coder(const Batch *b, F f) {
        if (b->bits == 2)
            f(LloydMax<2>{});
        else if (b->bits == 3)
            f(LloydMax<3>{});
        else
            f(LloydMax<4>{});
    }
};

}  // namespace gqe

GQE_API int gq_eden_abi_version(void) { return GQ_EDEN_ABI_VERSION; }

GQE_API const char *gq_eden_last_error(void) { return gqr::err_buf; }

GQE_API int gq_eden_compress_batched(const gq_eden_batch *b, uint8_t *wire, float ef_scale, float *out, void *stream) {
    return gqr::compress<gqe::Lib>("gq_eden_compress_batched", b, wire, ef_scale, out, false, nullptr, stream);
}

GQE_API int gq_eden_compress_batched_stepped(const gq_eden_batch *b, const uint64_t *rotation, uint8_t *wire, float ef_scale, float *out,
                                             void *stream) {
    return gqr::compress<gqe::Lib>("gq_eden_compress_batched_stepped", b, wire, ef_scale, out, true, rotation, stream);
}

GQE_API int gq_eden_decode_sum_batched(const gq_eden_batch *b, const uint8_t *gathered, int64_t user_stride_bytes, int R, float *out, int plain,
                                       void *stream) {
    return gqr::decode_sum<gqe::Lib>("gq_eden_decode_sum_batched", b, gathered, user_stride_bytes, R, out, plain, false, nullptr, stream);
}

GQE_API int gq_eden_decode_sum_batched_stepped(const gq_eden_batch *b, const uint64_t *rotation, const uint8_t *gathered,
                                               int64_t user_stride_bytes, int R, float *out, int plain, void *stream) {
    return gqr::decode_sum<gqe::Lib>("gq_eden_decode_sum_batched_stepped", b, gathered, user_stride_bytes, R, out, plain, true, rotation, stream);
}

GQE_API int gq_eden_compress_batched_streams(const gq_eden_batch *b, const uint64_t *rotation, int32_t stream, uint8_t *wire, float ef_scale,
                                             float *out, void *stream_handle) {
    return gqr::compress<gqe::Lib>("gq_eden_compress_batched_streams", b, wire, ef_scale, out, true, rotation, stream_handle, &stream);
}

GQE_API int gq_eden_decode_sum_batched_streams(const gq_eden_batch *b, const uint64_t *rotation, int32_t first_stream, const uint8_t *gathered,
                                               int64_t user_stride_bytes, int R, float *out, int plain, void *stream_handle) {
    return gqr::decode_sum<gqe::Lib>("gq_eden_decode_sum_batched_streams", b, gathered, user_stride_bytes, R, out, plain, true, rotation,
                                     stream_handle, &first_stream);
}
