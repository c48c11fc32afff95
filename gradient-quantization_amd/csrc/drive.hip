// The rotated 1-bit compressor (DRIVE), multi-tensor (segment table) form -- libgq_drive.so
// (include/gq_drive.h: the contract, to the bit; tests/drive_contract.py restates it in numpy).
//
// The kernels and the host path are csrc/rotq_kernels.hpp's, shared with eden.hip and instantiated here with its one-bit coder
// (Sign1, below); the rotation is csrc/hadamard.hpp's, shared with mxr.hip; this file is the descriptor and the exported names.
#include "gq_drive.h"
#include "gq_lib_prelude.hpp"
#include "hadamard.hpp"
#include "rotq_kernels.hpp"

#define GQD_API extern "C" __attribute__((visibility("default")))

namespace gqd {

static_assert(GQ_DRIVE_BLOCK == gqr::BLOCK && GQ_DRIVE_UNBIASED == gqr::UNBIASED && GQ_DRIVE_MSE == gqr::MSE,
              "csrc/rotq_kernels.hpp codes the blocks, and under the scale modes, of include/gq_drive.h");
static_assert(sizeof(gq_drive_batch) == 80, "gq_drive_batch: the layout the ctypes binding declares (gq_amd/native.py)");

using gqr::BLOCK;
using gqr::block_sum;
using gqr::lane_xor_bits;
using gqr::MSE;
using gqr::PER_LANE;
using gqr::QNAN;
using gqr::UNBIASED;
using gqx::HadLane;

// DRIVE: a code is the sign bit of x', a lane's eight one byte.  |x'| and x' * x' go through the tree; S = Q / L1 (unbiased) or
// L1 / 256 (mse).  The bytes of a quad are gathered into a dword by two DPP moves and the dwords of four quads into 16 bytes by
// three swizzles: a block's 32 code bytes leave as two 16-byte stores.  A decoded value is +-S: the scale's bits under the code's
// sign, no multiplication.
struct Sign1 {
    static constexpr int CODE_BYTES = BLOCK / 8;
    template <int SCALE>
    __device__ __forceinline__ static float encode(const HadLane &x, uint32_t &word, float (&)[PER_LANE]) {
        uint32_t byte = 0;
        float a[PER_LANE], q[PER_LANE];
#pragma unroll
        for (int k = 0; k < PER_LANE; ++k) {
            const uint32_t xb = __float_as_uint(x[k]);
            byte |= (xb >> 31) << k;
            a[k] = __uint_as_float(xb & 0x7fffffffu);
            q[k] = x[k] * x[k];      // (one multiplication; never fused into the tree's additions)
        }
        word = byte;
        const float L1 = block_sum(a);
        float S;
        if (SCALE == UNBIASED) {
            const float Q = block_sum(q);
            S = Q / L1;
        } else {
            S = L1 / 256.0f;
        }
        S = L1 == 0.0f ? 0.0f : S;
        return (__float_as_uint(L1) & 0x7fffffffu) >= 0x7f800000u ? __uint_as_float(QNAN) : S;      // an infinity or a NaN among the x'
    }
    __device__ __forceinline__ static float decoded(float S, uint32_t word, const float (&)[PER_LANE], const HadLane &, int k) {
        return value(word, __float_as_uint(S), k);
    }
    // lane l's byte at byte l of the block: a quad's four into a little-endian dword, four quads' dwords into 16 bytes
    __device__ __forceinline__ static void store(uint8_t *block, uint32_t l, bool live, uint32_t word) {
        uint32_t dw = word << (8 * (l & 3u));
        dw |= lane_xor_bits<1>(dw);
        dw |= lane_xor_bits<2>(dw);
        const uint32_t d1 = lane_xor_bits<4>(dw), d2 = lane_xor_bits<8>(dw), d3 = lane_xor_bits<8>(d1);      // of the lanes + 4, + 8, + 12
        if (live && (l & 15u) == 0) *reinterpret_cast<uint4 *>(block + l) = make_uint4(dw, d1, d2, d3);
    }
    __device__ __forceinline__ static uint32_t load(const uint8_t *p, int64_t lane, bool) { return p[lane]; }
    __device__ __forceinline__ static float value(uint32_t word, uint32_t sbits, int k) {
        return __uint_as_float(sbits ^ (((word >> k) & 1u) << 31));
    }
};

struct Lib {
    using Batch = gq_drive_batch;
    static constexpr const char *SCALE_MODES = "GQ_DRIVE_UNBIASED or GQ_DRIVE_MSE";
    static int check_own(const Batch *, const char *) { return GQ_OK; }
    template <class F>
    static void with_coder(const Batch *, F f) {
        f(Sign1{});
    }
};

}  // namespace gqd

GQD_API int gq_drive_abi_version(void) { return GQ_DRIVE_ABI_VERSION; }

GQD_API const char *gq_drive_last_error(void) { return gqr::err_buf; }

GQD_API int gq_drive_compress_batched(const gq_drive_batch *b, uint8_t *wire, float ef_scale, float *out, void *stream) {
    return gqr::compress<gqd::Lib>("gq_drive_compress_batched", b, wire, ef_scale, out, false, nullptr, stream);
}

GQD_API int gq_drive_compress_batched_stepped(const gq_drive_batch *b, const uint64_t *rotation, uint8_t *wire, float ef_scale, float *out,
                                              void *stream) {
    return gqr::compress<gqd::Lib>("gq_drive_compress_batched_stepped", b, wire, ef_scale, out, true, rotation, stream);
}

GQD_API int gq_drive_decode_sum_batched(const gq_drive_batch *b, const uint8_t *gathered, int64_t user_stride_bytes, int R, float *out, int plain,
                                        void *stream) {
    return gqr::decode_sum<gqd::Lib>("gq_drive_decode_sum_batched", b, gathered, user_stride_bytes, R, out, plain, false, nullptr, stream);
}

GQD_API int gq_drive_decode_sum_batched_stepped(const gq_drive_batch *b, const uint64_t *rotation, const uint8_t *gathered,
                                                int64_t user_stride_bytes, int R, float *out, int plain, void *stream) {
    return gqr::decode_sum<gqd::Lib>("gq_drive_decode_sum_batched_stepped", b, gathered, user_stride_bytes, R, out, plain, true, rotation, stream);
}

GQD_API int gq_drive_compress_batched_streams(const gq_drive_batch *b, const uint64_t *rotation, int32_t stream, uint8_t *wire, float ef_scale,
                                              float *out, void *stream_handle) {
    return gqr::compress<gqd::Lib>("gq_drive_compress_batched_streams", b, wire, ef_scale, out, true, rotation, stream_handle, &stream);
}

GQD_API int gq_drive_decode_sum_batched_streams(const gq_drive_batch *b, const uint64_t *rotation, int32_t first_stream, const uint8_t *gathered,
                                                int64_t user_stride_bytes, int R, float *out, int plain, void *stream_handle) {
    return gqr::decode_sum<gqd::Lib>("gq_drive_decode_sum_batched_streams", b, gathered, user_stride_bytes, R, out, plain, true, rotation,
                                     stream_handle, &first_stream);
}
