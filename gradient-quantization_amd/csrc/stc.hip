// Sparse ternary compression on a 16-bit wire, multi-tensor (segment table) form -- libgq_stc.so (include/gq_stc.h).
//
// The kept set is top-k's (csrc/topk.hip is the map: the radix select on the 31-bit key, three hist / pick pairs -- the kernels of
// csrc/sparse_kernels.hpp, which both libraries instantiate -- then count, scan, write).  What is new sits in the last three launches:
//   count    also the item's float64 sum s[t] of the |w| with key > T: slot j = 256 s + thread of the item is step s of that
//            thread, so the header's halvings 2048 ... 256 add a thread's own sixteen values, 128 and 64 cross the waves through
//            LDS and 32 ... 1 are lane shifts of wave 0 -- a fixed tree, no atomics.
//   scan     also the tensor's S: item t belongs to thread t % 256, so every halving down to 256 is a thread's own read-add-write
//            of `sums` (no barrier), the last 256 values take the same tree as an item; then mu into state[2].
//   write    the item's words into LDS at their rank inside the item, then the run start[t] .. start[t + 1] - 1 of the wire
//            in 4-byte stores (a 2-byte store where the run starts or ends on an odd word); the tensor's first item also writes
//            the header and the zero bytes behind the last word.  Also the dense decoded tensor and, with error feedback, the
//            residual; the identity-compressed tensors are copied into the wire.
// decode     one workgroup per item: start[t] names its words, no search; every payload in order into an LDS accumulator.
// Every launch's arguments depend on the layout alone: the eight compress launches replay from a HIP graph.
#include <math.h>

#include "gq_lib_prelude.hpp"
#include "gq_stc.h"
#include "sparse_kernels.hpp"

#define GQS_API extern "C" __attribute__((visibility("default")))

namespace gqs {

using gql::copy_dense;
using gql::err_buf;
using gql::fail;
using gqsp::block_exclusive_scan;
using gqsp::kept_before;
using gqsp::key_of;
using gqsp::load_w;
using gqsp::NO_KEY;
using gqsp::THREADS;
using gqsp::WAVES;

struct Sizes {      // what the select's kernels (csrc/sparse_kernels.hpp) are instantiated over
    static constexpr int CHUNK = GQ_STC_CHUNK, BINS = GQ_STC_HIST_BINS;
};
constexpr int CHUNK = Sizes::CHUNK;
constexpr int PER_THREAD = CHUNK / THREADS;
static_assert(CHUNK == 4096 && THREADS == 256, "the sum tree of include/gq_stc.h is written out for 16 steps of 256 threads");
static_assert(sizeof(gq_stc_batch) == 80, "gq_stc_batch: the layout the ctypes binding declares (gq_amd/native.py)");

// halve(x, 256) of include/gq_stc.h over the threads' values: x[t] + x[t + h] for h = 128, 64 (LDS), 32 ... 1 (lane shifts).
// The result is thread 0's.  lds: THREADS doubles, free on entry.
__device__ __forceinline__ double block_halve(double x, double *lds) {
    const int t = threadIdx.x;
    lds[t] = x;
    __syncthreads();
    double r = 0.0;
    if (t < 64) {
        r = (lds[t] + lds[t + 128]) + (lds[t + 64] + lds[t + 192]);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) r = r + __shfl_down(r, d, 64);
    }
    return r;
}

// per item: #(key > T), #(key == T) and s[t], the float64 sum of the |w| with key > T in the header's order
template <bool EF>
__global__ __launch_bounds__(THREADS) void stc_count_kernel(const int64_t *__restrict__ seg_table, const int32_t *__restrict__ item_seg,
                                                            const int32_t *__restrict__ state, int32_t *__restrict__ counts,
                                                            double *__restrict__ sums, float ef_scale) {
    __shared__ uint32_t lds[2][WAVES];
    __shared__ double tree[THREADS];
    const int64_t item = blockIdx.x;
    const int seg = item_seg[item];
    const int64_t *rec = seg_table + 8 * (int64_t)seg;
    const int64_t n = rec[1];
    const uint32_t T = (uint32_t)state[4 * seg];
    uint32_t gt = 0, eq = 0;
    double x = 0.0;
    if (T != NO_KEY) {
        const float *v = reinterpret_cast<const float *>(rec[0]);
        const float *err = EF ? reinterpret_cast<const float *>(rec[7]) : nullptr;
        const int64_t base = (item - rec[2]) * CHUNK;
        const int64_t end = base + CHUNK < n ? base + CHUNK : n;
        double b[PER_THREAD / 2];      // the halving 2048: step s + step s + 8
#pragma unroll
        for (int s = 0; s < PER_THREAD / 2; ++s) {
            double pair[2] = {0.0, 0.0};
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int64_t i = base + (int64_t)(s + u * (PER_THREAD / 2)) * THREADS + threadIdx.x;
                if (i < end) {
                    const float w = load_w<EF>(v, err, i, ef_scale);
                    const uint32_t key = key_of(w);
                    gt += key > T ? 1u : 0u;
                    eq += key == T ? 1u : 0u;
                    if (key > T) pair[u] = (double)fabsf(w);
                }
            }
            b[s] = pair[0] + pair[1];
        }
        // the halvings 1024, 512 and 256
        x = ((b[0] + b[4]) + (b[2] + b[6])) + ((b[1] + b[5]) + (b[3] + b[7]));
    }
    uint32_t tg, te;
    block_exclusive_scan(gt, lds[0], &tg);
    block_exclusive_scan(eq, lds[1], &te);
    const double s = block_halve(x, tree);
    if (threadIdx.x == 0) {
        counts[2 * item] = (int32_t)tg;
        counts[2 * item + 1] = (int32_t)te;
        sums[item] = s;
    }
}

// one workgroup per tensor: the items' counts -> their exclusive prefix sums (in place), in index order; the items' sums -> S,
// and mu into state[2]
__global__ __launch_bounds__(THREADS) void stc_scan_kernel(const int64_t *__restrict__ seg_table, int32_t *__restrict__ state,
                                                           int32_t *__restrict__ counts, double *sums) {
    __shared__ double tree[THREADS];
    const int seg = blockIdx.x;
    const int64_t *rec = seg_table + 8 * (int64_t)seg;
    const int64_t n = rec[1], first = rec[2], k = rec[4];
    const int64_t nit = (n + CHUNK - 1) / CHUNK;
    uint32_t total[2];
    gqsp::scan_item_counts<2, 0>(counts, first, nit, total);
    // halve(s, P): slot j and slot j + h belong to one thread while h >= 256; a slot past the tensor's items is +0.0, and
    // x + +0.0 is x for every x a sum of magnitudes can be
    double *s = sums + first;
    int64_t P = 1;
    while (P < nit) P <<= 1;
    for (int64_t h = P >> 1; h >= THREADS; h >>= 1)
        for (int64_t j = threadIdx.x; j < h && j + h < nit; j += THREADS) s[j] = s[j] + s[j + h];
    const double S0 = block_halve(threadIdx.x < nit ? s[threadIdx.x] : 0.0, tree);
    if (threadIdx.x == 0) {
        uint32_t mu = 0u;
        if (k != 0) {
            const double ties = (double)(uint32_t)state[4 * seg + 1] * (double)__uint_as_float((uint32_t)state[4 * seg]);
            const float m = (float)((S0 + ties) / (double)k);
            mu = m != m ? GQ_STC_NAN : __float_as_uint(m);
        }
        state[4 * seg + 2] = (int32_t)mu;
    }
}

template <bool EF>
__global__ __launch_bounds__(THREADS) void stc_write_kernel(const int64_t *__restrict__ seg_table, const int32_t *__restrict__ item_seg,
                                                            const int32_t *__restrict__ state, const int32_t *__restrict__ counts,
                                                            uint8_t *__restrict__ wire, float *__restrict__ out, float ef_scale,
                                                            const int64_t *__restrict__ dense_table, int ndense) {
    copy_dense<THREADS>(dense_table, ndense, wire);
    __shared__ uint16_t words[CHUNK];          // the item's words at their rank inside the item
    const int64_t item = blockIdx.x;
    const int seg = item_seg[item];
    const int64_t *rec = seg_table + 8 * (int64_t)seg;
    const int64_t n = rec[1], k = rec[4];
    const int64_t nit = (n + CHUNK - 1) / CHUNK, t = item - rec[2];
    const uint32_t T = (uint32_t)state[4 * seg], need = (uint32_t)state[4 * seg + 1];
    const uint32_t mu = (uint32_t)state[4 * seg + 2] & 0x7fffffffu;
    uint32_t gt_before = (uint32_t)counts[2 * item], eq_before = (uint32_t)counts[2 * item + 1];
    const uint32_t start = kept_before(gt_before, eq_before, need);
    float *v = reinterpret_cast<float *>(rec[0]);
    float *err = EF ? reinterpret_cast<float *>(rec[7]) : nullptr;
    uint32_t *head = reinterpret_cast<uint32_t *>(wire + rec[3]);
    uint16_t *word = reinterpret_cast<uint16_t *>(wire + rec[3] + GQ_STC_HEADER_BYTES + 4 * nit);      // (4-byte aligned)
    float *o = out ? out + rec[5] : nullptr;
    const int64_t base = t * CHUNK;
    const int64_t end = base + CHUNK < n ? base + CHUNK : n;
    if (threadIdx.x == 0) head[4 + t] = start;
    if (t == 0) {
        if (threadIdx.x == 0) {
            head[0] = (uint32_t)k;
            head[1] = (uint32_t)state[4 * seg + 2];
            head[2] = (uint32_t)nit;
            head[3] = 0u;
        }
        const int64_t pad = (GQ_STC_SECTION_BYTES(n, k) - (GQ_STC_HEADER_BYTES + 4 * nit + 2 * k)) / 2;      // 0 ... 7 words
        if (threadIdx.x < pad) word[k + threadIdx.x] = 0;
    }
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
        const uint32_t sign = __float_as_uint(w) & 0x80000000u;
        if (kept) {
            const uint32_t local = r.pos(need) - start;
            if (local < (uint32_t)CHUNK) words[local] = (uint16_t)((uint32_t)(s * THREADS + threadIdx.x) | (sign >> 16));
        }
        if (valid) gqsp::store_decoded<EF>(v, err, o, i, w, __uint_as_float(kept ? (mu | sign) : 0u));
        gt_before += r.tg;
        eq_before += r.te;
    }
    __syncthreads();
    // the run [lo, hi) of the tensor's words, two words a store where both are the item's
    const uint32_t stop = kept_before(gt_before, eq_before, need);
    const uint32_t lo = start < (uint64_t)k ? start : (uint32_t)k, hi = stop < (uint64_t)k ? stop : (uint32_t)k;
    for (uint32_t d = (lo >> 1) + threadIdx.x; d < (hi + 1) >> 1; d += THREADS) {
        const uint32_t g0 = 2 * d, g1 = g0 + 1;
        const bool in0 = g0 >= lo, in1 = g1 < hi;      // (g0 < hi and g1 >= lo hold for every d of the loop)
        if (in0 && in1) {
            if (g1 - start < (uint32_t)CHUNK)
                *reinterpret_cast<uint32_t *>(word + g0) = (uint32_t)words[g0 - start] | ((uint32_t)words[g1 - start] << 16);
        } else if (in0) {
            if (g0 - start < (uint32_t)CHUNK) word[g0] = words[g0 - start];
        } else if (in1) {
            if (g1 - start < (uint32_t)CHUNK) word[g1] = words[g1 - start];
        }
    }
}

__global__ __launch_bounds__(THREADS) void stc_decode_kernel(const int64_t *__restrict__ seg_table, const int32_t *__restrict__ item_seg,
                                                             const uint8_t *__restrict__ gathered, int64_t stride, int R,
                                                             float *__restrict__ out, int plain) {
    __shared__ float acc[CHUNK];
    const int64_t item = blockIdx.x;
    const int seg = item_seg[item];
    const int64_t *rec = seg_table + 8 * (int64_t)seg;
    const int64_t n = rec[1], off = rec[3];
    const uint32_t k = (uint32_t)rec[4];
    const int64_t nit = (n + CHUNK - 1) / CHUNK, t = item - rec[2];
    float *o = out + rec[5];
    const int64_t base = t * CHUNK;
    const int64_t end = base + CHUNK < n ? base + CHUNK : n;
    const uint32_t len = (uint32_t)(end - base);
    gqsp::decode_clear<CHUNK>(acc);
    const bool direct = plain && R == 1;
    for (int r = 0; r < R; ++r) {
        const uint8_t *p = gathered + (int64_t)r * stride + off;
        const uint32_t *head = reinterpret_cast<const uint32_t *>(p);
        const uint16_t *word = reinterpret_cast<const uint16_t *>(p + GQ_STC_HEADER_BYTES + 4 * nit);
        const uint32_t mu = head[1] & 0x7fffffffu;
        const uint32_t a = head[4 + t], b = t + 1 < nit ? head[4 + t + 1] : k;
        const uint32_t lo = a < k ? a : k, hi = b < k ? b : k;
        for (uint32_t j = lo + threadIdx.x; j < hi; j += THREADS) {
            const uint32_t wd = word[j];
            const uint32_t u = wd & 0x7fffu;
            const float c = __uint_as_float(mu | ((wd & 0x8000u) << 16));
            if (u < len) acc[u] = direct ? c : acc[u] + c;
        }
        __syncthreads();      // payloads in order: r + 1 adds to what r left
    }
    gqsp::decode_store_mean(acc, o, base, len, R, direct);
}

static int check_batch(const gq_stc_batch *b, const char *what, bool compress) {
    const int rc = gqsp::check_batch_common(b, what);
    if (rc != GQ_OK) return rc;
    if (compress && (!b->hist || !b->state || !b->counts || !b->sums || (b->ndense > 0 && !b->dense_table)))
        return fail(GQ_ERR_INVALID_ARG, "%s: null scratch buffer", what);
    return GQ_OK;
}

}  // namespace gqs

GQS_API int gq_stc_abi_version(void) { return GQ_STC_ABI_VERSION; }

GQS_API const char *gq_stc_last_error(void) { return gqs::err_buf; }

template <bool EF>
static int stc_compress(const gq_stc_batch *b, uint8_t *wire, float ef_scale, float *out, hipStream_t st) {
    using namespace gqs;
    const dim3 items((unsigned)b->nitems), segs((unsigned)b->nseg), block(THREADS);
    for (int p = 0; p < 3; ++p) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(gqsp::hist_kernel<Sizes, EF>), items, block, 0, st, b->seg_table, b->item_seg, b->state, b->hist, p,
                           ef_scale);
        GQL_CHECK_LAUNCH("gq_stc_compress_batched (hist)");
        hipLaunchKernelGGL(gqsp::pick_kernel<Sizes>, segs, block, 0, st, b->seg_table, b->state, b->hist, p);
        GQL_CHECK_LAUNCH("gq_stc_compress_batched (pick)");
    }
    hipLaunchKernelGGL(HIP_KERNEL_NAME(stc_count_kernel<EF>), items, block, 0, st, b->seg_table, b->item_seg, b->state, b->counts, b->sums,
                       ef_scale);
    GQL_CHECK_LAUNCH("gq_stc_compress_batched (count)");
    hipLaunchKernelGGL(stc_scan_kernel, segs, block, 0, st, b->seg_table, b->state, b->counts, b->sums);
    GQL_CHECK_LAUNCH("gq_stc_compress_batched (scan)");
    hipLaunchKernelGGL(HIP_KERNEL_NAME(stc_write_kernel<EF>), items, block, 0, st, b->seg_table, b->item_seg, b->state, b->counts, wire, out,
                       ef_scale, b->dense_table, b->ndense);
    GQL_CHECK_LAUNCH("gq_stc_compress_batched (write)");
    return GQ_OK;
}

GQS_API int gq_stc_compress_batched(const gq_stc_batch *b, uint8_t *wire, float ef_scale, float *out, void *stream) {
    const int rc = gqs::check_batch(b, "gq_stc_compress_batched", true);
    if (rc != GQ_OK) return rc;
    if (!wire || (reinterpret_cast<uintptr_t>(wire) & 3) != 0)
        return gqs::fail(GQ_ERR_INVALID_ARG, "gq_stc_compress_batched: the wire must be a 4-byte aligned device address");
    if ((reinterpret_cast<uintptr_t>(b->sums) & 7) != 0) return gqs::fail(GQ_ERR_INVALID_ARG, "gq_stc_compress_batched: sums must be 8-byte aligned");
    const bool ef = !isnan(ef_scale);
    if (ef && !out) return gqs::fail(GQ_ERR_INVALID_ARG, "gq_stc_compress_batched: error feedback needs `out` (the decoded tensors)");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return ef ? stc_compress<true>(b, wire, ef_scale, out, st) : stc_compress<false>(b, wire, 0.0f, out, st);
}

GQS_API int gq_stc_decode_sum_batched(const gq_stc_batch *b, const uint8_t *gathered, int64_t user_stride_bytes, int R, float *out,
                                      int plain, void *stream) {
    int rc = gqs::check_batch(b, "gq_stc_decode_sum_batched", false);
    if (rc == GQ_OK) rc = gqsp::check_decode("gq_stc_decode_sum_batched", gathered, out, user_stride_bytes, R);
    if (rc != GQ_OK) return rc;
    hipLaunchKernelGGL(gqs::stc_decode_kernel, dim3((unsigned)b->nitems), dim3(gqs::THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                       b->seg_table, b->item_seg, gathered, user_stride_bytes, R, out, plain ? 1 : 0);
    GQL_CHECK_LAUNCH("gq_stc_decode_sum_batched");
    return GQ_OK;
}
