// Top-k sparsification on a sparse wire, multi-tensor (segment table) form -- libgq_topk.so (include/gq_topk.h).
//
// The reference (topk_sparsification_compressor.py:9-26) keeps torch.topk(abs(v), k) and decodes v * mask.  Here the kept set
// comes from a radix select on the 31-bit key  bits(v) & 0x7fffffff  (NaN -> 0x7fffffff: torch ranks NaN above +inf):
//   hist(p) / pick(p), p = 0, 1, 2   11 / 11 / 9 bits of the key, most significant first.  A hist launch folds every item's
//                                    LDS histogram into the tensor's histogram with integer atomics (order-independent); the
//                                    pick launch (one workgroup per tensor) finds the bin that holds the k-th largest key,
//                                    extends the prefix and clears the histogram it read -- it is zero again for the next step.
//                                    After pass 2 the prefix IS the threshold key T, and `need` = how many of the elements
//                                    with key == T are kept (the lowest indices: DESIGN.md section 2).
//   count                            per item: #(key > T), #(key == T)
//   scan                             per tensor: the items' exclusive prefix sums of both counts, in index order
//   write                            kept = key > T, or key == T and fewer than `need` ties before it.  Position in the wire
//                                    = #(key > T before it) + min(#(key == T before it), need): ascending indices, the same
//                                    bytes whatever order the workgroups run in.  Also the dense decoded tensor and, with
//                                    error feedback, the residual; the identity-compressed tensors are copied into the wire.
// decode                             one workgroup per chunk of the output: for every payload in order, the run of its
//                                    (ascending) indices that falls into the chunk is found by binary search and added into
//                                    an LDS accumulator -- no float atomics, a fixed order of additions.
// Every launch's arguments depend on the layout alone: the eight compress launches replay from a HIP graph.
#include <math.h>

#include "gq_lib_prelude.hpp"
#include "gq_topk.h"
#include "sparse_kernels.hpp"

#define GQT_API extern "C" __attribute__((visibility("default")))

namespace gqt {

using gql::copy_dense;
using gql::err_buf;
using gql::fail;
using gqsp::block_exclusive_scan;
using gqsp::key_of;
using gqsp::load_w;
using gqsp::NO_KEY;
using gqsp::THREADS;
using gqsp::WAVES;

struct Sizes {      // what the select's kernels (csrc/sparse_kernels.hpp) are instantiated over
    static constexpr int CHUNK = GQ_TOPK_CHUNK, BINS = GQ_TOPK_HIST_BINS;
};
constexpr int CHUNK = Sizes::CHUNK;
constexpr int PER_THREAD = CHUNK / THREADS;
static_assert(CHUNK % THREADS == 0, "an item is a whole number of block-wide steps");
static_assert(sizeof(gq_topk_batch) == 72, "gq_topk_batch: the layout the ctypes binding declares (gq_amd/native.py)");

template <bool EF>
__global__ __launch_bounds__(THREADS) void topk_count_kernel(const int64_t *__restrict__ seg_table, const int32_t *__restrict__ item_seg,
                                                             const int32_t *__restrict__ state, int32_t *__restrict__ counts,
                                                             float ef_scale) {
    __shared__ uint32_t lds[2][WAVES];
    const int64_t item = blockIdx.x;
    const int seg = item_seg[item];
    const int64_t *rec = seg_table + 8 * (int64_t)seg;
    const int64_t n = rec[1];
    const uint32_t T = (uint32_t)state[4 * seg];
    uint32_t gt = 0, eq = 0;
    if (T != NO_KEY) {
        const float *v = reinterpret_cast<const float *>(rec[0]);
        const float *err = EF ? reinterpret_cast<const float *>(rec[7]) : nullptr;
        const int64_t base = (item - rec[2]) * CHUNK;
        const int64_t end = base + CHUNK < n ? base + CHUNK : n;
        for (int64_t i = base + threadIdx.x; i < end; i += THREADS) {
            const uint32_t key = key_of(load_w<EF>(v, err, i, ef_scale));
            gt += key > T ? 1u : 0u;
            eq += key == T ? 1u : 0u;
        }
    }
    uint32_t tg, te;
    block_exclusive_scan(gt, lds[0], &tg);
    block_exclusive_scan(eq, lds[1], &te);
    if (threadIdx.x == 0) {
        counts[2 * item] = (int32_t)tg;
        counts[2 * item + 1] = (int32_t)te;
    }
}

// one workgroup per tensor: the items' two counts -> their exclusive prefix sums (in place), in index order
__global__ __launch_bounds__(THREADS) void topk_scan_kernel(const int64_t *__restrict__ seg_table, int32_t *__restrict__ counts) {
    const int64_t *rec = seg_table + 8 * (int64_t)blockIdx.x;
    const int64_t n = rec[1], first = rec[2];
    uint32_t total[2];
    gqsp::scan_item_counts<2, 0>(counts, first, (n + CHUNK - 1) / CHUNK, total);
}

template <bool EF>
__global__ __launch_bounds__(THREADS) void topk_write_kernel(const int64_t *__restrict__ seg_table, const int32_t *__restrict__ item_seg,
                                                             const int32_t *__restrict__ state, const int32_t *__restrict__ counts,
                                                             uint8_t *__restrict__ wire, float *__restrict__ out, float ef_scale,
                                                             const int64_t *__restrict__ dense_table, int ndense) {
    copy_dense<THREADS>(dense_table, ndense, wire);
    const int64_t item = blockIdx.x;
    const int seg = item_seg[item];
    const int64_t *rec = seg_table + 8 * (int64_t)seg;
    const int64_t n = rec[1], k = rec[4];
    const uint32_t T = (uint32_t)state[4 * seg], need = (uint32_t)state[4 * seg + 1];
    uint32_t gt_before = (uint32_t)counts[2 * item], eq_before = (uint32_t)counts[2 * item + 1];
    float *v = reinterpret_cast<float *>(rec[0]);
    float *err = EF ? reinterpret_cast<float *>(rec[7]) : nullptr;
    uint32_t *idx = reinterpret_cast<uint32_t *>(wire + rec[3]);
    float *val = reinterpret_cast<float *>(wire + rec[3] + 4 * k);
    float *o = out ? out + rec[5] : nullptr;
    const int64_t base = (item - rec[2]) * CHUNK;
    const int64_t end = base + CHUNK < n ? base + CHUNK : n;
#pragma unroll 1
    for (int s = 0; s < PER_THREAD; ++s) {
        const int64_t i = base + (int64_t)s * THREADS + threadIdx.x;
        const bool valid = i < end;
        float w = 0.0f;
        uint32_t key = 0;
        if (valid) {
            w = load_w<EF>(v, err, i, ef_scale);
            key = key_of(w);
        }
        const bool is_gt = valid && key > T;
        const bool is_eq = valid && key == T;
        const gqsp::Rank r = gqsp::rank_step<true>(s, is_gt, is_eq, gt_before, eq_before);
        const bool kept = r.kept(is_gt, is_eq, need);
        if (kept) {
            const uint32_t pos = r.pos(need);
            if (pos < (uint64_t)k) {
                idx[pos] = (uint32_t)i;
                val[pos] = w;
            }
        }
        if (valid) gqsp::store_decoded<EF>(v, err, o, i, w, w * (kept ? 1.0f : 0.0f));      // the reference's v * mask
        gt_before += r.tg;
        eq_before += r.te;
    }
}

__global__ __launch_bounds__(THREADS) void topk_decode_kernel(const int64_t *__restrict__ seg_table, const int32_t *__restrict__ item_seg,
                                                              const uint8_t *__restrict__ gathered, int64_t stride, int R,
                                                              float *__restrict__ out, int plain) {
    __shared__ float acc[CHUNK];
    const int64_t item = blockIdx.x;
    const int seg = item_seg[item];
    const int64_t *rec = seg_table + 8 * (int64_t)seg;
    const int64_t n = rec[1], k = rec[4], off = rec[3];
    float *o = out + rec[5];
    const int64_t base = (item - rec[2]) * CHUNK;
    const int64_t end = base + CHUNK < n ? base + CHUNK : n;
    const uint32_t len = (uint32_t)(end - base);
    gqsp::decode_clear<CHUNK>(acc);
    const bool direct = plain && R == 1;
    for (int r = 0; r < R; ++r) {
        const uint8_t *p = gathered + (int64_t)r * stride + off;
        const uint32_t *idx = reinterpret_cast<const uint32_t *>(p);
        const float *val = reinterpret_cast<const float *>(p + 4 * k);
        gqsp::decode_add_pairs(acc, idx, val, k, base, end, len, direct);
    }
    gqsp::decode_store_mean(acc, o, base, len, R, direct);
}

static int check_batch(const gq_topk_batch *b, const char *what, bool compress) {
    const int rc = gqsp::check_batch_common(b, what);
    if (rc != GQ_OK) return rc;
    if (compress && (!b->hist || !b->state || !b->counts || (b->ndense > 0 && !b->dense_table)))
        return fail(GQ_ERR_INVALID_ARG, "%s: null scratch buffer", what);
    return GQ_OK;
}

}  // namespace gqt

GQT_API int gq_topk_abi_version(void) { return GQ_TOPK_ABI_VERSION; }

GQT_API const char *gq_topk_last_error(void) { return gqt::err_buf; }

template <bool EF>
static int topk_compress(const gq_topk_batch *b, uint8_t *wire, float ef_scale, float *out, hipStream_t st) {
    using namespace gqt;
    const dim3 items((unsigned)b->nitems), segs((unsigned)b->nseg), block(THREADS);
    for (int p = 0; p < 3; ++p) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(gqsp::hist_kernel<Sizes, EF>), items, block, 0, st, b->seg_table, b->item_seg, b->state, b->hist, p,
                           ef_scale);
        GQL_CHECK_LAUNCH("gq_topk_compress_batched (hist)");
        hipLaunchKernelGGL(gqsp::pick_kernel<Sizes>, segs, block, 0, st, b->seg_table, b->state, b->hist, p);
        GQL_CHECK_LAUNCH("gq_topk_compress_batched (pick)");
    }
    hipLaunchKernelGGL(HIP_KERNEL_NAME(topk_count_kernel<EF>), items, block, 0, st, b->seg_table, b->item_seg, b->state, b->counts, ef_scale);
    GQL_CHECK_LAUNCH("gq_topk_compress_batched (count)");
    hipLaunchKernelGGL(topk_scan_kernel, segs, block, 0, st, b->seg_table, b->counts);
    GQL_CHECK_LAUNCH("gq_topk_compress_batched (scan)");
    hipLaunchKernelGGL(HIP_KERNEL_NAME(topk_write_kernel<EF>), items, block, 0, st, b->seg_table, b->item_seg, b->state, b->counts, wire, out,
                       ef_scale, b->dense_table, b->ndense);
    GQL_CHECK_LAUNCH("gq_topk_compress_batched (write)");
    return GQ_OK;
}

GQT_API int gq_topk_compress_batched(const gq_topk_batch *b, uint8_t *wire, float ef_scale, float *out, void *stream) {
    const int rc = gqt::check_batch(b, "gq_topk_compress_batched", true);
    if (rc != GQ_OK) return rc;
    if (!wire) return gqt::fail(GQ_ERR_INVALID_ARG, "gq_topk_compress_batched: null wire");
    const bool ef = !isnan(ef_scale);
    if (ef && !out) return gqt::fail(GQ_ERR_INVALID_ARG, "gq_topk_compress_batched: error feedback needs `out` (the decoded tensors)");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return ef ? topk_compress<true>(b, wire, ef_scale, out, st) : topk_compress<false>(b, wire, 0.0f, out, st);
}

GQT_API int gq_topk_decode_sum_batched(const gq_topk_batch *b, const uint8_t *gathered, int64_t user_stride_bytes, int R, float *out,
                                       int plain, void *stream) {
    int rc = gqt::check_batch(b, "gq_topk_decode_sum_batched", false);
    if (rc == GQ_OK) rc = gqsp::check_decode("gq_topk_decode_sum_batched", gathered, out, user_stride_bytes, R);
    if (rc != GQ_OK) return rc;
    hipLaunchKernelGGL(gqt::topk_decode_kernel, dim3((unsigned)b->nitems), dim3(gqt::THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                       b->seg_table, b->item_seg, gathered, user_stride_bytes, R, out, plain ? 1 : 0);
    GQL_CHECK_LAUNCH("gq_topk_decode_sum_batched");
    return GQ_OK;
}
