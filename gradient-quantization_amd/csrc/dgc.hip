// Momentum correction and momentum factor masking around the top-k select -- libgq_dgc.so (include/gq_dgc.h).
//
//   accumulate   one workgroup per item (GQ_TOPK_CHUNK elements of one tensor): u1 = m * u + g, the product rounded, then the sum
//                (-ffp-contract=off), stored into u and into the select's source s.  A streaming launch: 8 bytes read and 8
//                written per element, as float4 where g, u and s are 16-byte aligned (a gradient view may not be).
//   mask         one workgroup per item: item j of a tensor takes the indices [j * CHUNK, min(k, (j + 1) * CHUNK)) of the section
//                the select has just written and stores +0 into u there; the items past ceil(k / CHUNK) have nothing to do.
// The select between the two is gq_topk_compress_batched with ef_scale = 1 over the state table (source s, error buffer v): it
// forms v1 = s + v, keeps the top k of it and leaves v = v1 - decoded.  Neither launch's arguments depend on the data.
#include "gq_lib_prelude.hpp"
#include "gq_dgc.h"

#define GQD_API extern "C" __attribute__((visibility("default")))

namespace gqd {

constexpr int THREADS = 256;
constexpr int CHUNK = GQ_TOPK_CHUNK;
static_assert(CHUNK % (4 * THREADS) == 0, "an item is a whole number of block-wide float4 steps");
static_assert(sizeof(gq_dgc_batch) == 40, "gq_dgc_batch: the layout the ctypes binding declares (gq_amd/native.py)");

using gql::aligned16;
using gql::err_buf;
using gql::fail;

__device__ __forceinline__ float step(float m, float u, float g) {
    const float t = m * u;
    return t + g;
}

__global__ __launch_bounds__(THREADS) void dgc_accumulate_kernel(const int64_t *__restrict__ grad_table,
                                                                 const int64_t *__restrict__ state_table,
                                                                 const int32_t *__restrict__ item_seg, float m) {
    const int64_t item = blockIdx.x;
    const int seg = item_seg[item];
    const int64_t *rec = state_table + 8 * (int64_t)seg;
    const int64_t n = rec[1];
    const float *g = reinterpret_cast<const float *>(grad_table[8 * (int64_t)seg]);
    float *s = reinterpret_cast<float *>(rec[0]);
    float *u = reinterpret_cast<float *>(rec[6]);
    const int64_t base = (item - rec[2]) * CHUNK;
    const int64_t end = base + CHUNK < n ? base + CHUNK : n;
    if (base >= end) return;
    int64_t done = base;
    if (aligned16(g) && aligned16(s) && aligned16(u)) {      // (base is a multiple of 4 elements: the chunk starts aligned too)
        const int64_t quads = (end - base) >> 2;
        const float4 *g4 = reinterpret_cast<const float4 *>(g + base);
        float4 *u4 = reinterpret_cast<float4 *>(u + base);
        float4 *s4 = reinterpret_cast<float4 *>(s + base);
        for (int64_t q = threadIdx.x; q < quads; q += THREADS) {
            const float4 a = u4[q], b = g4[q];
            float4 r;
            r.x = step(m, a.x, b.x);
            r.y = step(m, a.y, b.y);
            r.z = step(m, a.z, b.z);
            r.w = step(m, a.w, b.w);
            u4[q] = r;
            s4[q] = r;
        }
        done = base + 4 * quads;
    }
    for (int64_t i = done + threadIdx.x; i < end; i += THREADS) {
        const float r = step(m, u[i], g[i]);
        u[i] = r;
        s[i] = r;
    }
}

__global__ __launch_bounds__(THREADS) void dgc_mask_kernel(const int64_t *__restrict__ state_table, const int32_t *__restrict__ item_seg,
                                                           const uint8_t *__restrict__ wire) {
    const int64_t item = blockIdx.x;
    const int seg = item_seg[item];
    const int64_t *rec = state_table + 8 * (int64_t)seg;
    const int64_t n = rec[1], k = rec[4];
    const int64_t lo = (item - rec[2]) * CHUNK;
    const int64_t hi = lo + CHUNK < k ? lo + CHUNK : k;
    if (lo >= hi) return;
    const uint32_t *idx = reinterpret_cast<const uint32_t *>(wire + rec[3]);
    float *u = reinterpret_cast<float *>(rec[6]);
    for (int64_t j = lo + threadIdx.x; j < hi; j += THREADS) {
        const int64_t i = (int64_t)idx[j];
        if (i < n) u[i] = 0.0f;
    }
}

static int check_batch(const gq_dgc_batch *b, const char *what) {
    if (!b || b->struct_bytes != sizeof(gq_dgc_batch)) return fail(GQ_ERR_INVALID_ARG, "%s: descriptor missing or of another size", what);
    if (b->nseg < 1 || b->nitems < 1 || b->nitems > 0x7fffffff)
        return fail(GQ_ERR_INVALID_ARG, "%s: bad sizes (nseg %d, nitems %lld)", what, b->nseg, (long long)b->nitems);
    if (!b->state_table) return fail(GQ_ERR_INVALID_ARG, "%s: null state table", what);
    if (!b->item_seg) return fail(GQ_ERR_INVALID_ARG, "%s: null item table", what);
    return GQ_OK;
}

}  // namespace gqd

GQD_API int gq_dgc_abi_version(void) { return GQ_DGC_ABI_VERSION; }

GQD_API const char *gq_dgc_last_error(void) { return gqd::err_buf; }

GQD_API int gq_dgc_accumulate_batched(const gq_dgc_batch *b, float m, void *stream) {
    const int rc = gqd::check_batch(b, "gq_dgc_accumulate_batched");
    if (rc != GQ_OK) return rc;
    if (!b->grad_table) return gqd::fail(GQ_ERR_INVALID_ARG, "gq_dgc_accumulate_batched: null gradient table");
    if (m != m) return gqd::fail(GQ_ERR_INVALID_ARG, "gq_dgc_accumulate_batched: the momentum is NaN");
    hipLaunchKernelGGL(gqd::dgc_accumulate_kernel, dim3((unsigned)b->nitems), dim3(gqd::THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                       b->grad_table, b->state_table, b->item_seg, m);
    GQL_CHECK_LAUNCH("gq_dgc_accumulate_batched");
    return GQ_OK;
}

GQD_API int gq_dgc_mask_batched(const gq_dgc_batch *b, const uint8_t *wire, void *stream) {
    const int rc = gqd::check_batch(b, "gq_dgc_mask_batched");
    if (rc != GQ_OK) return rc;
    if (!wire) return gqd::fail(GQ_ERR_INVALID_ARG, "gq_dgc_mask_batched: null wire");
    if ((reinterpret_cast<uintptr_t>(wire) & 3) != 0) return gqd::fail(GQ_ERR_INVALID_ARG, "gq_dgc_mask_batched: the wire must be 4-byte aligned");
    hipLaunchKernelGGL(gqd::dgc_mask_kernel, dim3((unsigned)b->nitems), dim3(gqd::THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                       b->state_table, b->item_seg, wire);
    GQL_CHECK_LAUNCH("gq_dgc_mask_batched");
    return GQ_OK;
}
