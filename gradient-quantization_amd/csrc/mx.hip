// Block-scaled small floats (OCP Microscaling: MXFP4 / MXFP6 / MXFP8) as a gradient compressor, multi-tensor (segment table) form --
// libgq_mx.so (include/gq_mx.h: the contract, to the bit; tests/mx_contract.py restates it in numpy).
//
// The kernels and the host path are csrc/mx_kernels.hpp's (what they do is told there), shared with mxr.hip; the formats and the
// element type are csrc/mx_common.hpp's.  This file is what makes them libgq_mx.so: the policy that transforms nothing, the
// descriptor and the exported names.
#include "gq_mx.h"
#include "mx_common.hpp"
#include "mx_kernels.hpp"

#define GQX_API extern "C" __attribute__((visibility("default")))

namespace gqx {

static_assert(sizeof(gq_mx_batch) == 48, "gq_mx_batch: the layout the ctypes binding declares (gq_amd/native.py)");

// No rotation: x' = w.  Nothing is carried and nothing is executed, so no lane has to stay for another.
struct Plain {
    struct Args {};
    static constexpr int BLOCK = 0;
    static constexpr bool EVERY_LANE = false;
    __device__ __forceinline__ explicit Plain(const Args &) {}
    __device__ __forceinline__ const Lane8 &forward(const Lane8 &w, Lane8 &, bool) const { return w; }
    __device__ __forceinline__ void inverse(Lane8 &, bool) const {}
    static Args args(const gq_mx_batch *) { return Args(); }
};

}  // namespace gqx

GQX_API int gq_mx_abi_version(void) { return GQ_MX_ABI_VERSION; }

GQX_API const char *gq_mx_last_error(void) { return gqx::err_buf; }

GQX_API int gq_mx_compress_batched(const gq_mx_batch *b, uint8_t *wire, int random_mode, const float *r, uint64_t seed, float ef_scale,
                                   float *out, void *stream) {
    return gqx::compress_batched<gqx::Plain, gqx::TT_F32>("gq_mx_compress_batched", b, wire, random_mode, r, seed, ef_scale, out, stream);
}

GQX_API int gq_mx_decode_sum_batched(const gq_mx_batch *b, const uint8_t *gathered, int64_t user_stride_bytes, int R, float *out, int plain,
                                     void *stream) {
    return gqx::decode_sum_batched<gqx::Plain, gqx::TT_F32>("gq_mx_decode_sum_batched", b, gathered, user_stride_bytes, R, out, plain, stream);
}

// the same launches over bf16 sources, `out` and dense-copy sources (include/gq_mx.h, TENSOR-SIDE TYPE); the wire is the f32 twin's
GQX_API int gq_mx_compress_batched_bf16(const gq_mx_batch *b, uint8_t *wire, int random_mode, const float *r, uint64_t seed, float ef_scale,
                                        uint16_t *out, void *stream) {
    return gqx::compress_batched<gqx::Plain, gqx::TT_BF16>("gq_mx_compress_batched_bf16", b, wire, random_mode, r, seed, ef_scale, out, stream);
}

GQX_API int gq_mx_decode_sum_batched_bf16(const gq_mx_batch *b, const uint8_t *gathered, int64_t user_stride_bytes, int R, uint16_t *out,
                                          int plain, void *stream) {
    return gqx::decode_sum_batched<gqx::Plain, gqx::TT_BF16>("gq_mx_decode_sum_batched_bf16", b, gathered, user_stride_bytes, R, out, plain, stream);
}
