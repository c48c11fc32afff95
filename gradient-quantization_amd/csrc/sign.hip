// signSGD on a 2-bit wire, multi-tensor (segment table) form -- libgq_sign.so (include/gq_sign.h).
//
// The reference (signsgd_compressor.py:4-12) sends torch.sign(v) and decodes it as it is.  torch.sign on an MI355X (ROCm torch
// 2.10; checked on ±0, ±NaN with payloads, ±inf, ±min subnormal, ±FLT_MAX) gives what the CPU gives: +0 for ±0 and for every
// NaN, ±1 for everything else -- never -0, never NaN.  The code of one element is therefore taken from its bits alone, with no
// float compare that a denormal mode could change:
//     m = bits & 0x7fffffff;   code = (1 <= m <= 0x7f800000) ? (sign bit ? 0b11 : 0b01) : 0b00
// and the decoded value is the code read as a two's-complement 2-bit integer (0b10 is reserved and never written).
//
// compress  one workgroup per item of GQ_SIGN_ITEM_BYTES wire bytes (16384 elements).  A lane owns one wire byte = four
//           elements: one float4 load (scalar loads at a tensor's ragged end or an unaligned source), four codes; two
//           shuffles gather four lanes' bytes into one uint32 word that the first of them stores.  Every byte of the section
//           is written, the pad included, so the wire depends on the input alone.  Also: the dense sign(w) (out), error
//           feedback (w back into the source, err = w - sign(w)), and the identity-compressed tensors copied into the wire.
// decode    the same items; a lane reads its byte of each of the R payloads in order, sums the four sign-extended fields as
//           integers (exact) and writes (float)sum / (float)R with a float4 store.
// Every launch's arguments depend on the layout alone: both replay from a HIP graph.
#include <math.h>

#include "gq_lib_prelude.hpp"
#include "gq_sign.h"

#define GQS_API extern "C" __attribute__((visibility("default")))

namespace gqs {

constexpr int THREADS = 256;
constexpr int ITEM_BYTES = GQ_SIGN_ITEM_BYTES;
constexpr int PER_THREAD = ITEM_BYTES / THREADS;      // wire bytes (four elements each) per lane and item
static_assert(ITEM_BYTES % THREADS == 0 && THREADS % 4 == 0, "an item is a whole number of block-wide steps of whole words");
static_assert(sizeof(gq_sign_batch) == 48, "gq_sign_batch: the layout the ctypes binding declares (gq_amd/native.py)");

using gql::aligned16;
using gql::copy_dense;
using gql::err_buf;
using gql::fail;

// the section of a tensor of n elements: ceil(n / 16) words, rounded up to 16 bytes (gq_amd.codecs._up)
__host__ __device__ constexpr int64_t section_bytes(int64_t n) { return (((n + 15) / 16) * 4 + 15) / 16 * 16; }

__device__ __forceinline__ uint32_t code_of(float w) {
    const uint32_t b = __float_as_uint(w);
    const uint32_t m = b & 0x7fffffffu;
    return (m - 1u) < 0x7f800000u ? ((b >> 31) ? 3u : 1u) : 0u;      // (m = 0 wraps above the bound: +0 like a NaN)
}

// the field of element k (0..3) of a wire byte as a signed integer: to the top of the word and back, arithmetically
__device__ __forceinline__ int field(uint32_t byte, int k) { return (int32_t)(byte << (30 - 2 * k)) >> 30; }

template <bool EF>
__global__ __launch_bounds__(THREADS) void sign_compress_kernel(const int64_t *__restrict__ seg_table, const int32_t *__restrict__ item_seg,
                                                                uint8_t *__restrict__ wire, float *__restrict__ out, float ef_scale,
                                                                const int64_t *__restrict__ dense_table, int ndense) {
    copy_dense<THREADS>(dense_table, ndense, wire);
    const int64_t item = blockIdx.x;
    const int seg = item_seg[item];
    const int64_t *rec = seg_table + 8 * (int64_t)seg;
    const int64_t n = rec[1];
    const int64_t sec = section_bytes(n);
    float *v = reinterpret_cast<float *>(rec[0]);
    float *err = EF ? reinterpret_cast<float *>(rec[7]) : nullptr;
    uint32_t *words = reinterpret_cast<uint32_t *>(wire + rec[3]);
    float *o = out ? out + rec[5] : nullptr;
    const int lane = threadIdx.x & 63;
    const int64_t base = (item - rec[2]) * ITEM_BYTES;
#pragma unroll
    for (int s = 0; s < PER_THREAD; ++s) {
        const int64_t t = base + (int64_t)s * THREADS + threadIdx.x;      // this lane's wire byte
        if (base + (int64_t)s * THREADS >= sec) break;                    // (uniform over the workgroup: sec is a multiple of 16)
        const int64_t e = 4 * t;
        float w[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        const bool full = e + 3 < n && aligned16(v + e) && (!EF || !err || aligned16(err + e));
        if (full) {
            const float4 a = *reinterpret_cast<const float4 *>(v + e);
            w[0] = a.x, w[1] = a.y, w[2] = a.z, w[3] = a.w;
            if (EF && err) {
                const float4 r = *reinterpret_cast<const float4 *>(err + e);
                const float rr[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float p = ef_scale * rr[k];      // (-ffp-contract=off: the product rounded, then the sum)
                    w[k] = w[k] + p;
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (e + k < n) {
                    w[k] = v[e + k];
                    if (EF && err) {
                        const float p = ef_scale * err[e + k];
                        w[k] = w[k] + p;
                    }
                }
            }
        }
        uint32_t byte = 0;
        float sg[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t c = e + k < n ? code_of(w[k]) : 0u;
            byte |= c << (2 * k);
            sg[k] = (float)field(c, 0);
        }
        if (e < n) {
            const bool vec = e + 3 < n;
            if (o) {
                if (vec && aligned16(o + e)) {
                    *reinterpret_cast<float4 *>(o + e) = make_float4(sg[0], sg[1], sg[2], sg[3]);
                } else {
                    for (int k = 0; k < 4 && e + k < n; ++k) o[e + k] = sg[k];
                }
            }
            if (EF && err) {
                if (full) {
                    *reinterpret_cast<float4 *>(v + e) = make_float4(w[0], w[1], w[2], w[3]);
                    *reinterpret_cast<float4 *>(err + e) = make_float4(w[0] - sg[0], w[1] - sg[1], w[2] - sg[2], w[3] - sg[3]);
                } else {
                    for (int k = 0; k < 4 && e + k < n; ++k) {
                        v[e + k] = w[k];
                        err[e + k] = w[k] - sg[k];
                    }
                }
            }
        }
        // four lanes' bytes -> one little-endian word (lanes 4q .. 4q+3 hold bytes 0 .. 3 of word t / 4)
        const uint32_t b1 = (uint32_t)__shfl_xor((int)byte, 1, 64);
        const uint32_t half = (lane & 1) ? (b1 | (byte << 8)) : (byte | (b1 << 8));
        const uint32_t h2 = (uint32_t)__shfl_xor((int)half, 2, 64);
        const uint32_t word = (lane & 2) ? (h2 | (half << 16)) : (half | (h2 << 16));
        if ((lane & 3) == 0 && t < sec) words[t >> 2] = word;
    }
}

__global__ __launch_bounds__(THREADS) void sign_decode_kernel(const int64_t *__restrict__ seg_table, const int32_t *__restrict__ item_seg,
                                                              const uint8_t *__restrict__ gathered, int64_t stride, int R,
                                                              float *__restrict__ out, int plain) {
    const int64_t item = blockIdx.x;
    const int seg = item_seg[item];
    const int64_t *rec = seg_table + 8 * (int64_t)seg;
    const int64_t n = rec[1], off = rec[3];
    float *o = out + rec[5];
    const int64_t base = (item - rec[2]) * ITEM_BYTES;
    const bool direct = plain && R == 1;
    const float fR = (float)R;
#pragma unroll
    for (int s = 0; s < PER_THREAD; ++s) {
        const int64_t t = base + (int64_t)s * THREADS + threadIdx.x;
        const int64_t e = 4 * t;
        if (e >= n) break;
        int sum[4] = {0, 0, 0, 0};
        const uint8_t *p = gathered + off + t;
        for (int r = 0; r < R; ++r) {
            const uint32_t b = p[(int64_t)r * stride];
#pragma unroll
            for (int k = 0; k < 4; ++k) sum[k] += field(b, k);
        }
        float f[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) f[k] = direct ? (float)sum[k] : (float)sum[k] / fR;
        if (e + 3 < n && aligned16(o + e)) {
            *reinterpret_cast<float4 *>(o + e) = make_float4(f[0], f[1], f[2], f[3]);
        } else {
            for (int k = 0; k < 4 && e + k < n; ++k) o[e + k] = f[k];
        }
    }
}

static int check_batch(const gq_sign_batch *b, const char *what, bool compress) {
    if (!b || b->struct_bytes != sizeof(gq_sign_batch)) return fail(GQ_ERR_INVALID_ARG, "%s: descriptor missing or of another size", what);
    if (b->nseg < 1 || b->nitems < 1 || b->nitems > 0x7fffffff || b->ndense < 0)
        return fail(GQ_ERR_INVALID_ARG, "%s: bad sizes (nseg %d, nitems %lld, ndense %d)", what, b->nseg, (long long)b->nitems, b->ndense);
    if (!b->seg_table || !b->item_seg) return fail(GQ_ERR_INVALID_ARG, "%s: null table", what);
    if (compress && b->ndense > 0 && !b->dense_table) return fail(GQ_ERR_INVALID_ARG, "%s: null dense table", what);
    return GQ_OK;
}

}  // namespace gqs

GQS_API int gq_sign_abi_version(void) { return GQ_SIGN_ABI_VERSION; }

GQS_API const char *gq_sign_last_error(void) { return gqs::err_buf; }

GQS_API int gq_sign_compress_batched(const gq_sign_batch *b, uint8_t *wire, float ef_scale, float *out, void *stream) {
    using namespace gqs;
    const int rc = check_batch(b, "gq_sign_compress_batched", true);
    if (rc != GQ_OK) return rc;
    if (!wire) return fail(GQ_ERR_INVALID_ARG, "gq_sign_compress_batched: null wire");
    if ((reinterpret_cast<uintptr_t>(wire) & 3) != 0 || (reinterpret_cast<uintptr_t>(out) & 3) != 0)
        return fail(GQ_ERR_INVALID_ARG, "gq_sign_compress_batched: wire and out must be 4-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)b->nitems), block(THREADS);
    if (!isnan(ef_scale))
        hipLaunchKernelGGL(HIP_KERNEL_NAME(sign_compress_kernel<true>), grid, block, 0, st, b->seg_table, b->item_seg, wire, out, ef_scale,
                           b->dense_table, b->ndense);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(sign_compress_kernel<false>), grid, block, 0, st, b->seg_table, b->item_seg, wire, out, 0.0f,
                           b->dense_table, b->ndense);
    GQL_CHECK_LAUNCH("gq_sign_compress_batched");
    return GQ_OK;
}

GQS_API int gq_sign_decode_sum_batched(const gq_sign_batch *b, const uint8_t *gathered, int64_t user_stride_bytes, int R, float *out,
                                       int plain, void *stream) {
    using namespace gqs;
    const int rc = check_batch(b, "gq_sign_decode_sum_batched", false);
    if (rc != GQ_OK) return rc;
    if (!gathered || !out) return fail(GQ_ERR_INVALID_ARG, "gq_sign_decode_sum_batched: null pointer");
    if (R < 1 || (R > 1 && user_stride_bytes < 0))
        return fail(GQ_ERR_INVALID_ARG, "gq_sign_decode_sum_batched: R = %d, user stride %lld", R, (long long)user_stride_bytes);
    if ((reinterpret_cast<uintptr_t>(out) & 3) != 0) return fail(GQ_ERR_INVALID_ARG, "gq_sign_decode_sum_batched: out must be 4-byte aligned");
    hipLaunchKernelGGL(sign_decode_kernel, dim3((unsigned)b->nitems), dim3(THREADS), 0, reinterpret_cast<hipStream_t>(stream), b->seg_table,
                       b->item_seg, gathered, user_stride_bytes, R, out, plain ? 1 : 0);
    GQL_CHECK_LAUNCH("gq_sign_decode_sum_batched");
    return GQ_OK;
}
