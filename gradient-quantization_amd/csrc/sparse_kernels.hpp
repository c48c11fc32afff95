// What the sparsifiers with an index / value wire share: libgq_topk.so (topk.hip), libgq_stc.so (stc.hip), libgq_thr.so (thr.hip)
// and, for the load and the scan alone, libgq_maurey.so (maurey.hip).  Everything here is a template or __forceinline__ with internal
// linkage: each library compiles its own copy, and a file brings the names into its namespace with using-declarations.
//   the key        key_of: bits(w) & 0x7fffffff, NaN above +inf; load_w: the value a compress works on
//   the select     hist_kernel / pick_kernel: the radix select of the k-th largest key, three passes of 11 / 11 / 9 bits (topk.hip's
//                  header comment is the map of the launches; stc.hip runs the same ones)
//   the compaction scan_item_counts: the items' counts -> their exclusive prefix sums in index order (the scan launches);
//                  rank_step: an element's rank among the kept ones inside its item (the write launches), with the tie rule
//                   in Rank::kept / kept_before; store_decoded: the dense decoded tensor and the residual
//   the decode     decode_clear / decode_add_pairs / decode_store_mean: one workgroup per chunk of the output, every payload in
//                  order into an LDS accumulator -- no float atomics, a fixed order of additions
//   the host side  check_batch_common, check_payloads, check_decode: the checks whose texts differ by the function's name alone
#pragma once
#include "gq_lib_prelude.hpp"

namespace gqsp {

using gql::fail;

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr uint32_t NO_KEY = 0x80000000u;      // above every key: the threshold of a tensor with k == 0 (nothing kept)

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

// ---- the select ----------------------------------------------------------------------------------------------------------------------
// Lib: the library's sizes, struct { static constexpr int CHUNK, BINS; } = elements per item, words of histogram per tensor
// (GQ_TOPK_CHUNK / _HIST_BINS, GQ_STC_CHUNK / _HIST_BINS).  A type of the library's own, not the two numbers: two libraries in one
// process then hold kernels of different names.
template <class Lib, bool EF>
__global__ __launch_bounds__(THREADS) void hist_kernel(const int64_t *__restrict__ seg_table, const int32_t *__restrict__ item_seg,
                                                       const int32_t *__restrict__ state, uint32_t *__restrict__ hist, int pass,
                                                       float ef_scale) {
    constexpr int CHUNK = Lib::CHUNK, BINS = Lib::BINS;
    static_assert(BINS >= 1 << pass_bits(0) && BINS >= 1 << pass_bits(1) && BINS >= 1 << pass_bits(2), "a pass's bins fit the histogram");
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
template <class Lib>
__global__ __launch_bounds__(THREADS) void pick_kernel(const int64_t *__restrict__ seg_table, int32_t *__restrict__ state,
                                                       uint32_t *__restrict__ hist, int pass) {
    static_assert((1 << pass_bits(0)) <= 8 * THREADS && (1 << pass_bits(2)) % THREADS == 0, "a thread reads up to eight whole bins");
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
    uint32_t *g = hist + (int64_t)seg * Lib::BINS;
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

// ---- the compaction ------------------------------------------------------------------------------------------------------------------
// The body of a scan launch (one workgroup per tensor): N counts per item -> their exclusive prefix sums over the tensor's `nit`
// items first .. first + nit - 1 (in place), in index order; total[j] = the tensor's sum of count j.  An item has two words of
// `counts`; the N scanned ones start at word WORD.
template <int N, int WORD>
__device__ __forceinline__ void scan_item_counts(int32_t *__restrict__ counts, int64_t first, int64_t nit, uint32_t (&total)[N]) {
    static_assert(N >= 1 && WORD >= 0 && WORD + N <= 2, "an item's two words");
    __shared__ uint32_t lds[N][WAVES];
#pragma unroll
    for (int j = 0; j < N; ++j) total[j] = 0;
    for (int64_t b0 = 0; b0 < nit; b0 += THREADS) {
        const int64_t it = b0 + threadIdx.x;
        uint32_t x[N], before[N], sum[N];
#pragma unroll
        for (int j = 0; j < N; ++j) x[j] = 0;
        if (it < nit) {
#pragma unroll
            for (int j = 0; j < N; ++j) x[j] = (uint32_t)counts[2 * (first + it) + WORD + j];
        }
#pragma unroll
        for (int j = 0; j < N; ++j) before[j] = block_exclusive_scan(x[j], lds[j], &sum[j]);
        if (it < nit) {
#pragma unroll
            for (int j = 0; j < N; ++j) counts[2 * (first + it) + WORD + j] = (int32_t)(total[j] + before[j]);
        }
#pragma unroll
        for (int j = 0; j < N; ++j) total[j] += sum[j];
        __syncthreads();      // (the next round rewrites lds)
    }
}

// how many kept elements lie before one that has g keys > T and e keys == T before it: of the ties, the `need` lowest indices
// are kept
__device__ __forceinline__ uint32_t kept_before(uint32_t g, uint32_t e, uint32_t need) { return g + (e < need ? e : need); }

// what rank_step tells a lane about its element: gb / eb = the keys > T / == T before it in the tensor, tg / te = this step's
// totals over the workgroup (the caller adds them to its running counts)
struct Rank {
    uint32_t gb, eb, tg, te;
    __device__ __forceinline__ bool kept(bool is_gt, bool is_eq, uint32_t need) const { return is_gt || (is_eq && eb < need); }
    __device__ __forceinline__ uint32_t pos(uint32_t need) const { return kept_before(gb, eb, need); }
};

// Step s of a write loop: every thread brings one element (is_gt: key > T, is_eq: key == T; both false past the item's end) and
// the counts before this step.  TIES = false (a threshold that keeps every key above it, no ties: thr.hip): is_eq is not read,
// eb = te = 0.  One barrier per step: the waves' popcounts go through LDS words of the step's parity, so a wave still reading
// step s's words is not overwritten before step s + 2, and the barrier of step s + 1 lies in between.
template <bool TIES>
__device__ __forceinline__ Rank rank_step(int s, bool is_gt, bool is_eq, uint32_t gt_before, uint32_t eq_before) {
    __shared__ uint32_t lds[2][TIES ? 2 : 1][WAVES];      // [step parity][> T, == T][wave]
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    const uint64_t mg = __ballot(is_gt), me = TIES ? __ballot(is_eq) : 0ull;
    if (lane == 0) {
        lds[s & 1][0][wv] = (uint32_t)__popcll(mg);
        if (TIES) lds[s & 1][1][wv] = (uint32_t)__popcll(me);
    }
    __syncthreads();
    uint32_t pg = 0, pe = 0, tg = 0, te = 0;
#pragma unroll
    for (int j = 0; j < WAVES; ++j) {
        const uint32_t a = lds[s & 1][0][j], b = TIES ? lds[s & 1][1][j] : 0u;
        if (j < wv) {
            pg += a;
            pe += b;
        }
        tg += a;
        te += b;
    }
    return {gt_before + pg + (uint32_t)__popcll(mg & below), eq_before + pe + (uint32_t)__popcll(me & below), tg, te};
}

// the tail of a write step for a valid element: the dense decoded tensor and, with error feedback, w and the residual
template <bool EF>
__device__ __forceinline__ void store_decoded(float *__restrict__ v, float *__restrict__ err, float *__restrict__ o, int64_t i, float w,
                                              float dec) {
    if (o) o[i] = dec;
    if (EF && err) {
        v[i] = w;
        err[i] = w - dec;
    }
}

// ---- the decode-mean -----------------------------------------------------------------------------------------------------------------
// One workgroup per chunk [base, end) of a tensor's output, len = end - base; acc: CHUNK floats of LDS.  decode_clear, then every
// payload in order (decode_add_pairs, or the library's own loop followed by a barrier), then decode_store_mean.
// direct: plain && R == 1, the one payload's values as they are (-0 stays -0).
template <int CHUNK>
__device__ __forceinline__ void decode_clear(float *acc) {
    for (int t = threadIdx.x; t < CHUNK; t += THREADS) acc[t] = 0.0f;
    __syncthreads();
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

// one payload's k pairs (ascending indices): the run of them that falls into the chunk is found by binary search and added
__device__ __forceinline__ void decode_add_pairs(float *acc, const uint32_t *idx, const float *val, int64_t k, int64_t base, int64_t end,
                                                 uint32_t len, bool direct) {
    const int64_t lo = lower_bound_u32(idx, k, base), hi = lower_bound_u32(idx, k, end);
    for (int64_t j = lo + threadIdx.x; j < hi; j += THREADS) {
        const uint32_t u = idx[j] - (uint32_t)base;
        if (u < len) acc[u] = direct ? val[j] : acc[u] + val[j];
    }
    __syncthreads();      // payloads in order: r + 1 adds to what r left
}

// o: the tensor's output
__device__ __forceinline__ void decode_store_mean(const float *acc, float *__restrict__ o, int64_t base, uint32_t len, int R, bool direct) {
    const float fR = (float)R;
    for (uint32_t t = threadIdx.x; t < len; t += THREADS) o[base + t] = direct ? acc[t] : acc[t] / fR;
}

// ---- the host side -------------------------------------------------------------------------------------------------------------------
// what: the exported function's name, the head of every text.  Batch: gq_topk_batch, gq_stc_batch or gq_thr_batch -- the fields
// read here have the same names in all three; a library's check_batch goes on with its own fields.
template <class Batch>
static int check_batch_common(const Batch *b, const char *what) {
    if (!b || b->struct_bytes != sizeof(Batch)) return fail(GQ_ERR_INVALID_ARG, "%s: descriptor missing or of another size", what);
    if (b->nseg < 1 || b->nitems < 1 || b->nitems > 0x7fffffff || b->ndense < 0)
        return fail(GQ_ERR_INVALID_ARG, "%s: bad sizes (nseg %d, nitems %lld, ndense %d)", what, b->nseg, (long long)b->nitems, b->ndense);
    if (!b->seg_table || !b->item_seg) return fail(GQ_ERR_INVALID_ARG, "%s: null table", what);
    return GQ_OK;
}

// the arguments of a *_decode_sum_batched behind its descriptor: the pointers, R and the users' stride ...
static inline int check_payloads(const char *what, const uint8_t *gathered, const float *out, int64_t user_stride_bytes, int R) {
    if (!gathered || !out) return fail(GQ_ERR_INVALID_ARG, "%s: null pointer", what);
    if (R < 1 || (R > 1 && (user_stride_bytes < 0 || (user_stride_bytes & 3) != 0)))
        return fail(GQ_ERR_INVALID_ARG, "%s: R = %d, user stride %lld", what, R, (long long)user_stride_bytes);
    return GQ_OK;
}

// ... and the gathered wire's alignment
static inline int check_decode(const char *what, const uint8_t *gathered, const float *out, int64_t user_stride_bytes, int R) {
    const int rc = check_payloads(what, gathered, out, user_stride_bytes, R);
    if (rc != GQ_OK) return rc;
    if ((reinterpret_cast<uintptr_t>(gathered) & 3) != 0) return fail(GQ_ERR_INVALID_ARG, "%s: the gathered wire must be 4-byte aligned", what);
    return GQ_OK;
}

}  // namespace gqsp
