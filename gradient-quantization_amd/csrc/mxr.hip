// The microscaling compressor behind a randomized Hadamard rotation, multi-tensor (segment table) form -- libgq_mxr.so
// (include/gq_mxr.h: the contract, to the bit; tests/mxr_contract.py restates it in numpy).
//
// The kernels and the host path are csrc/mx_kernels.hpp's, shared with mx.hip; the rotation -- the policy the kernels are
// instantiated with, and what it calls -- is csrc/hadamard.hpp's, shared with drive.hip; this file is the descriptor and the
// exported names.
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
#include "hadamard.hpp"
#include "mx_common.hpp"
#include "mx_kernels.hpp"

#define GQXR_API extern "C" __attribute__((visibility("default")))

namespace gqx {

static_assert(GQ_MXR_BLOCK == 32 * PER_LANE && STEP % GQ_MXR_BLOCK == 0, "a 32-lane half owns a rotation block");
static_assert(sizeof(gq_mxr_batch) == 80, "gq_mxr_batch: the layout the ctypes binding declares (gq_amd/native.py)");
static_assert(HAD_BLOCK == GQ_MXR_BLOCK && HAD_PER_LANE == PER_LANE, "csrc/hadamard.hpp rotates the blocks, and over the lanes, of csrc/mx_kernels.hpp");

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
