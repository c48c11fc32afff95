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

#define GQT_API extern "C" __attribute__((visibility("default")))

namespace gqt {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int CHUNK = GQ_TOPK_CHUNK;
constexpr int PER_THREAD = CHUNK / THREADS;
constexpr int BINS = GQ_TOPK_HIST_BINS;
constexpr uint32_t NO_KEY = 0x80000000u;      // above every key: the threshold of a tensor with k == 0 (nothing kept)
static_assert(CHUNK % THREADS == 0, "an item is a whole number of block-wide steps");
static_assert(sizeof(gq_topk_batch) == 72, "gq_topk_batch: the layout the ctypes binding declares (gq_amd/native.py)");

using gql::copy_dense;
using gql::err_buf;
using gql::fail;

// pass p of the select: the key bits [shift, shift + nb)
__host__ __device__ constexpr int pass_shift(int p) { return p == 0 ? 20 : (p == 1 ? 9 : 0); }
__host__ __device__ constexpr int pass_bits(int p) { return p == 2 ? 9 : 11; }

__device__ __forceinline__ uint32_t key_of(float w) {
    const uint32_t a = __float_as_uint(w) & 0x7fffffffu;
    return a > 0x7f800000u ? 0x7fffffffu : a;
}

// the value the compress works on: v, or v + ef_scale * err (ps_quantizer.py:35; -ffp-contract=off keeps the two roundings)
template <bool EF>
__device__ __forceinline__ float load_w(const float *__restrict__ v, const float *__restrict__ err, int64_t i, float ef_scale) {
    float w = v[i];
    if (EF && err) {
        const float p = ef_scale * err[i];
        w = w + p;
    }
    return w;
}

// exclusive prefix sum over the workgroup in thread order; *total = the workgroup's sum.  lds: WAVES words, free on entry
// (the caller separates two uses of the same words by a barrier).
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t x, uint32_t *lds, uint32_t *total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t incl = x;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(incl, d, 64);
        if (lane >= d) incl += y;
    }
    if (lane == 63) lds[w] = incl;
    __syncthreads();
    uint32_t before = 0, tot = 0;
#pragma unroll
    for (int j = 0; j < WAVES; ++j) {
        const uint32_t t = lds[j];
        if (j < w) before += t;
        tot += t;
    }
    *total = tot;
    return before + incl - x;
}

template <bool EF>
__global__ __launch_bounds__(THREADS) void topk_hist_kernel(const int64_t *__restrict__ seg_table, const int32_t *__restrict__ item_seg,
                                                            const int32_t *__restrict__ state, uint32_t *__restrict__ hist, int pass,
                                                            float ef_scale) {
    __shared__ uint32_t h[BINS];
    const int64_t item = blockIdx.x;
    const int seg = item_seg[item];
    const int64_t *rec = seg_table + 8 * (int64_t)seg;
    const int64_t n = rec[1], k = rec[4];
    if (k == 0) return;
    const int shift = pass_shift(pass), nb = pass_bits(pass), hi = shift + nb;
    const uint32_t nbins = 1u << nb;
    const uint32_t prefix = pass == 0 ? 0u : (uint32_t)state[4 * seg];
    for (uint32_t b = threadIdx.x; b < nbins; b += THREADS) h[b] = 0u;
    __syncthreads();
    const float *v = reinterpret_cast<const float *>(rec[0]);
    const float *err = EF ? reinterpret_cast<const float *>(rec[7]) : nullptr;
    const int64_t base = (item - rec[2]) * CHUNK;
    const int64_t end = base + CHUNK < n ? base + CHUNK : n;
    for (int64_t i = base + threadIdx.x; i < end; i += THREADS) {
        const uint32_t key = key_of(load_w<EF>(v, err, i, ef_scale));
        if (pass == 0 || (key >> hi) == (prefix >> hi)) atomicAdd(&h[(key >> shift) & (nbins - 1u)], 1u);
    }
    __syncthreads();
    uint32_t *g = hist + (int64_t)seg * BINS;
    for (uint32_t b = threadIdx.x; b < nbins; b += THREADS) {
        const uint32_t c = h[b];
        if (c) atomicAdd(&g[b], c);
    }
}

// one workgroup per tensor: state[0] = prefix (after pass 2: the threshold key T), state[1] = the rank, among the keys that
// share the prefix, of the k-th largest one (after pass 2: how many keys == T are kept)
__global__ __launch_bounds__(THREADS) void topk_pick_kernel(const int64_t *__restrict__ seg_table, int32_t *__restrict__ state,
                                                            uint32_t *__restrict__ hist, int pass) {
    __shared__ uint32_t lds[WAVES];
    const int seg = blockIdx.x;
    const int64_t k = seg_table[8 * (int64_t)seg + 4];
    int32_t *st = state + 4 * seg;
    if (k == 0) {
        if (pass == 2 && threadIdx.x == 0) {
            st[0] = (int32_t)NO_KEY;
            st[1] = 0;
        }
        return;
    }
    const int shift = pass_shift(pass), nb = pass_bits(pass);
    const uint32_t nbins = 1u << nb;
    const int per = (int)(nbins / THREADS);       // 8 or 2 bins per thread, thread 0 the highest ones
    const uint32_t kr = pass == 0 ? (uint32_t)k : (uint32_t)st[1];
    const uint32_t prefix = pass == 0 ? 0u : (uint32_t)st[0];
    uint32_t *g = hist + (int64_t)seg * BINS;
    const uint32_t top = nbins - (uint32_t)per * threadIdx.x;
    uint32_t c[8];
    uint32_t sum = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        c[j] = 0;
        if (j < per) {
            c[j] = g[top - 1 - j];
            g[top - 1 - j] = 0u;      // the only reader of this bin: the histogram is clean for the next pass / step
            sum += c[j];
        }
    }
    uint32_t total;
    const uint32_t before = block_exclusive_scan(sum, lds, &total);   // (the barrier inside orders the reads of st above)
    if (before < kr && kr <= before + sum) {
        uint32_t cum = before;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (j < per) {
                if (kr <= cum + c[j]) {
                    st[0] = (int32_t)(prefix | ((top - 1 - (uint32_t)j) << shift));
                    st[1] = (int32_t)(kr - cum);
                    break;
                }
                cum += c[j];
            }
        }
    }
}

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

// one workgroup per tensor: the items' counts -> their exclusive prefix sums (in place), in index order
__global__ __launch_bounds__(THREADS) void topk_scan_kernel(const int64_t *__restrict__ seg_table, int32_t *__restrict__ counts) {
    __shared__ uint32_t lds[2][WAVES];
    const int64_t *rec = seg_table + 8 * (int64_t)blockIdx.x;
    const int64_t n = rec[1], first = rec[2];
    const int64_t nit = (n + CHUNK - 1) / CHUNK;
    uint32_t cg = 0, ce = 0;
    for (int64_t b0 = 0; b0 < nit; b0 += THREADS) {
        const int64_t it = b0 + threadIdx.x;
        uint32_t g = 0, e = 0;
        if (it < nit) {
            g = (uint32_t)counts[2 * (first + it)];
            e = (uint32_t)counts[2 * (first + it) + 1];
        }
        uint32_t tg, te;
        const uint32_t bg = block_exclusive_scan(g, lds[0], &tg);
        const uint32_t be = block_exclusive_scan(e, lds[1], &te);
        if (it < nit) {
            counts[2 * (first + it)] = (int32_t)(cg + bg);
            counts[2 * (first + it) + 1] = (int32_t)(ce + be);
        }
        cg += tg;
        ce += te;
        __syncthreads();      // (the next round rewrites lds)
    }
}

template <bool EF>
__global__ __launch_bounds__(THREADS) void topk_write_kernel(const int64_t *__restrict__ seg_table, const int32_t *__restrict__ item_seg,
                                                             const int32_t *__restrict__ state, const int32_t *__restrict__ counts,
                                                             uint8_t *__restrict__ wire, float *__restrict__ out, float ef_scale,
                                                             const int64_t *__restrict__ dense_table, int ndense) {
    copy_dense<THREADS>(dense_table, ndense, wire);
    __shared__ uint32_t lds[2][2][WAVES];      // [step parity][> T, == T][wave]
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
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
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
        const uint64_t mg = __ballot(is_gt), me = __ballot(is_eq);
        if (lane == 0) {
            lds[s & 1][0][wv] = (uint32_t)__popcll(mg);
            lds[s & 1][1][wv] = (uint32_t)__popcll(me);
        }
        __syncthreads();      // (parity: a wave still reading step s's words is not overwritten before step s + 2)
        uint32_t pg = 0, pe = 0, tg = 0, te = 0;
#pragma unroll
        for (int j = 0; j < WAVES; ++j) {
            const uint32_t a = lds[s & 1][0][j], b = lds[s & 1][1][j];
            if (j < wv) {
                pg += a;
                pe += b;
            }
            tg += a;
            te += b;
        }
        const uint32_t gb = gt_before + pg + (uint32_t)__popcll(mg & below);
        const uint32_t eb = eq_before + pe + (uint32_t)__popcll(me & below);
        const bool kept = is_gt || (is_eq && eb < need);
        if (kept) {
            const uint32_t pos = gb + (eb < need ? eb : need);
            if (pos < (uint64_t)k) {
                idx[pos] = (uint32_t)i;
                val[pos] = w;
            }
        }
        if (valid) {
            const float dec = w * (kept ? 1.0f : 0.0f);      // the reference's v * mask
            if (o) o[i] = dec;
            if (EF && err) {
                v[i] = w;
                err[i] = w - dec;
            }
        }
        gt_before += tg;
        eq_before += te;
    }
}

__device__ __forceinline__ int64_t lower_bound_u32(const uint32_t *__restrict__ a, int64_t n, int64_t x) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)a[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
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
    for (int t = threadIdx.x; t < CHUNK; t += THREADS) acc[t] = 0.0f;
    __syncthreads();
    const bool direct = plain && R == 1;
    for (int r = 0; r < R; ++r) {
        const uint8_t *p = gathered + (int64_t)r * stride + off;
        const uint32_t *idx = reinterpret_cast<const uint32_t *>(p);
        const float *val = reinterpret_cast<const float *>(p + 4 * k);
        const int64_t lo = lower_bound_u32(idx, k, base), hi = lower_bound_u32(idx, k, end);
        for (int64_t j = lo + threadIdx.x; j < hi; j += THREADS) {
            const uint32_t u = idx[j] - (uint32_t)base;
            if (u < len) acc[u] = direct ? val[j] : acc[u] + val[j];
        }
        __syncthreads();      // payloads in order: r + 1 adds to what r left
    }
    const float fR = (float)R;
    for (uint32_t t = threadIdx.x; t < len; t += THREADS) o[base + t] = direct ? acc[t] : acc[t] / fR;
}

static int check_batch(const gq_topk_batch *b, const char *what, bool compress) {
    if (!b || b->struct_bytes != sizeof(gq_topk_batch)) return fail(GQ_ERR_INVALID_ARG, "%s: descriptor missing or of another size", what);
    if (b->nseg < 1 || b->nitems < 1 || b->nitems > 0x7fffffff || b->ndense < 0)
        return fail(GQ_ERR_INVALID_ARG, "%s: bad sizes (nseg %d, nitems %lld, ndense %d)", what, b->nseg, (long long)b->nitems, b->ndense);
    if (!b->seg_table || !b->item_seg) return fail(GQ_ERR_INVALID_ARG, "%s: null table", what);
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
        hipLaunchKernelGGL(HIP_KERNEL_NAME(topk_hist_kernel<EF>), items, block, 0, st, b->seg_table, b->item_seg, b->state, b->hist, p,
                           ef_scale);
        GQL_CHECK_LAUNCH("gq_topk_compress_batched (hist)");
        hipLaunchKernelGGL(topk_pick_kernel, segs, block, 0, st, b->seg_table, b->state, b->hist, p);
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
    const int rc = gqt::check_batch(b, "gq_topk_decode_sum_batched", false);
    if (rc != GQ_OK) return rc;
    if (!gathered || !out) return gqt::fail(GQ_ERR_INVALID_ARG, "gq_topk_decode_sum_batched: null pointer");
    if (R < 1 || (R > 1 && (user_stride_bytes < 0 || (user_stride_bytes & 3) != 0)))
        return gqt::fail(GQ_ERR_INVALID_ARG, "gq_topk_decode_sum_batched: R = %d, user stride %lld", R, (long long)user_stride_bytes);
    if ((reinterpret_cast<uintptr_t>(gathered) & 3) != 0)
        return gqt::fail(GQ_ERR_INVALID_ARG, "gq_topk_decode_sum_batched: the gathered wire must be 4-byte aligned");
    hipLaunchKernelGGL(gqt::topk_decode_kernel, dim3((unsigned)b->nitems), dim3(gqt::THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                       b->seg_table, b->item_seg, gathered, user_stride_bytes, R, out, plain ? 1 : 0);
    GQL_CHECK_LAUNCH("gq_topk_decode_sum_batched");
    return GQ_OK;
}
