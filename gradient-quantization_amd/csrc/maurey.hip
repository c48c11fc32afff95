// Maurey sparsification on a sparse wire, multi-tensor (segment table) form -- libgq_maurey.so (include/gq_maurey.h).
//
// The reference (maurey_sparsification.py:21-36) makes k draws with P(i) = |v_i| / ||v||_1 and sends sign(v_i) * ||v||_1 / k
// per draw.  Here a draw is an inverse-CDF sample of a uniform u: the smallest i with u * T < C_i, C the f64 running sum of |w|
// in the fixed order the header states.  That order is a tree -- 16 elements to a thread, 16 threads to a group, 16 groups to an
// item, the items of a tensor to 256 runs -- whose every level is added left to right and whose pieces therefore tile the level
// above exactly: a piece of weight zero is an empty interval, C never decreases, and the same two device functions (item_scan,
// full_cdf) give the same bits wherever they are called.
//   sum      per item: S, the item's f64 sum (one read of the gradient)
//   scan     per tensor: the run / in-run prefixes of the items, every item's last C, T, the header; clears the draw counts
//   count    per draw: t = u * T -> its item by binary search over the items' last C; integer atomics count the item's draws
//   offsets  per tensor: the exclusive scan of the counts = every item's first output word
//   place    per draw: u into its item's bucket (any order)
//   item     one workgroup per item: C of its 4096 elements into LDS, every bucketed u to its element by binary search, LDS
//            integer atomics count the hits per element, their scan, and output word p of the item is the element whose
//            inclusive hit count first exceeds p -- ascending indices with no sort, the same bytes whatever the bucket order.
//            Also the dense D, error feedback, and the identity-compressed tensors copied into the wire.
// decode     one workgroup per chunk of the output (topk_decode_kernel's shape): for every payload in order, the run of its
//            words that falls into the chunk is found by binary search and counted into an LDS integer accumulator (+-1 per
//            word), then D = scale * (float)count is added into the LDS sum -- no float atomics, a fixed order of additions.
#include <math.h>

#include "gq_common.hpp"
#include "gq_lib_prelude.hpp"
#include "gq_maurey.h"
#include "sparse_kernels.hpp"

#define GQM_API extern "C" __attribute__((visibility("default")))

namespace gqm {

using gql::copy_dense;
using gql::err_buf;
using gql::fail;
using gqsp::block_exclusive_scan;
using gqsp::load_w;
using gqsp::THREADS;
using gqsp::WAVES;

constexpr int CHUNK = GQ_MAUREY_CHUNK;
constexpr int PER_THREAD = CHUNK / THREADS;           // 16 consecutive elements
constexpr int HEADER = GQ_MAUREY_HEADER_BYTES;
constexpr int PADDED = CHUNK + CHUNK / PER_THREAD;    // an LDS array of one word per element, one pad word behind every thread's 16
static_assert(PER_THREAD == 16 && THREADS == 256, "the order of additions (gq_maurey.h) is 16 x 16 x 16");
static_assert(sizeof(gq_maurey_batch) == 96, "gq_maurey_batch: the layout the ctypes binding declares (gq_amd/native.py)");

// element e of an item in an LDS array: a thread's 16 words are contiguous, the pad spreads the threads over the banks
__device__ __forceinline__ int phys(int e) { return e + (e >> 4); }

// this thread's 16 elements of the item that starts at `base` (elements past `end` read as +0)
template <bool EF>
__device__ __forceinline__ void load_item(const float *__restrict__ v, const float *__restrict__ err, int64_t base, int64_t end,
                                          float ef_scale, float (&w)[PER_THREAD]) {
    const int64_t i0 = base + (int64_t)threadIdx.x * PER_THREAD;
    const bool whole = i0 + PER_THREAD <= end;
    if (whole && (reinterpret_cast<uintptr_t>(v + i0) & 15) == 0 && (!(EF && err) || (reinterpret_cast<uintptr_t>(err + i0) & 15) == 0)) {
#pragma unroll
        for (int q = 0; q < PER_THREAD / 4; ++q) {
            const float4 x = reinterpret_cast<const float4 *>(v + i0)[q];
            w[4 * q] = x.x, w[4 * q + 1] = x.y, w[4 * q + 2] = x.z, w[4 * q + 3] = x.w;
            if (EF && err) {
                const float4 e = reinterpret_cast<const float4 *>(err + i0)[q];
                const float p0 = ef_scale * e.x, p1 = ef_scale * e.y, p2 = ef_scale * e.z, p3 = ef_scale * e.w;
                w[4 * q] = w[4 * q] + p0, w[4 * q + 1] = w[4 * q + 1] + p1, w[4 * q + 2] = w[4 * q + 2] + p2, w[4 * q + 3] = w[4 * q + 3] + p3;
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < PER_THREAD; ++j) w[j] = i0 + j < end ? load_w<EF>(v, err, i0 + j, ef_scale) : 0.0f;
    }
}

// The item's level of the sum (gq_maurey.h): s[j] = this thread's running sum through element j, B = the totals of the threads
// before it in its group, G = the totals of the groups before its group, S = the item's sum; all left to right.
// lds_tot: THREADS doubles, lds_grp: 16 doubles, both free on entry and not reused by the caller without a barrier.
__device__ __forceinline__ void item_scan(const float (&w)[PER_THREAD], double (&s)[PER_THREAD], double *lds_tot, double *lds_grp,
                                          double &B, double &G, double &S) {
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < PER_THREAD; ++j) {
        acc = acc + (double)fabsf(w[j]);
        s[j] = acc;
    }
    lds_tot[threadIdx.x] = acc;
    __syncthreads();
    const int g = threadIdx.x >> 4, pos = threadIdx.x & 15;
    double b = 0.0, bv = 0.0;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        if (c == pos) bv = b;
        b = b + lds_tot[16 * g + c];
    }
    if (pos == 0) lds_grp[g] = b;
    __syncthreads();
    double gg = 0.0, gv = 0.0;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        if (c == g) gv = gg;
        gg = gg + lds_grp[c];
    }
    B = bv, G = gv, S = gg;
}

// C of an element from the pieces of every level, innermost first
__device__ __forceinline__ double full_cdf(double run_base, double in_run, double G, double B, double s) {
    double c = B + s;
    c = G + c;
    c = in_run + c;
    return run_base + c;
}

__device__ __forceinline__ bool degenerate(double T) { return !(T > 0.0) || !(T < INFINITY); }

// t of a draw: u * T, or the largest double below T when that is not below T (T > 0 and finite here)
__device__ __forceinline__ double draw_t(float u, double T) {
    double t = (double)u * T;
    if (!(t < T)) t = __longlong_as_double(__double_as_longlong(T) - 1);
    return t;
}

__device__ __forceinline__ float draw_u(int random_mode, const float *__restrict__ r, uint64_t seed, int64_t d) {
    return random_mode == GQ_RANDOM_GIVEN ? r[d] : gq::uniform01(seed, (uint64_t)d);
}

template <bool EF>
__global__ __launch_bounds__(THREADS) void maurey_sum_kernel(const int64_t *__restrict__ seg_table, const int32_t *__restrict__ item_seg,
                                                             double *__restrict__ sums, float ef_scale) {
    __shared__ double lds_tot[THREADS], lds_grp[16];
    const int64_t item = blockIdx.x;
    const int64_t *rec = seg_table + 8 * (int64_t)item_seg[item];
    const int64_t n = rec[1];
    const float *v = reinterpret_cast<const float *>(rec[0]);
    const float *err = EF ? reinterpret_cast<const float *>(rec[7]) : nullptr;
    const int64_t base = (item - rec[2]) * CHUNK;
    const int64_t end = base + CHUNK < n ? base + CHUNK : n;
    float w[PER_THREAD];
    double s[PER_THREAD], B, G, S;
    load_item<EF>(v, err, base, end, ef_scale, w);
    item_scan(w, s, lds_tot, lds_grp, B, G, S);
    if (threadIdx.x == 0) sums[4 * item] = S;
}

// one workgroup per tensor: thread t owns the run of m consecutive items t * m ... (gq_maurey.h)
__global__ __launch_bounds__(THREADS) void maurey_scan_kernel(const int64_t *__restrict__ seg_table, double *__restrict__ sums,
                                                              double *__restrict__ totals, int32_t *__restrict__ counts,
                                                              uint8_t *__restrict__ wire) {
    __shared__ double lds_tot[THREADS];
    const int seg = blockIdx.x;
    const int64_t *rec = seg_table + 8 * (int64_t)seg;
    const int64_t n = rec[1], first = rec[2], k = rec[4];
    const int64_t nit = (n + CHUNK - 1) / CHUNK;
    const int64_t m = (nit + THREADS - 1) / THREADS;
    const int64_t lo = (int64_t)threadIdx.x * m < nit ? (int64_t)threadIdx.x * m : nit;
    const int64_t hi = lo + m < nit ? lo + m : nit;
    double acc = 0.0;
    for (int64_t it = lo; it < hi; ++it) acc = acc + sums[4 * (first + it)];
    lds_tot[threadIdx.x] = acc;
    __syncthreads();
    double b = 0.0, run_base = 0.0;
    for (int c = 0; c < THREADS; ++c) {
        if (c == (int)threadIdx.x) run_base = b;
        b = b + lds_tot[c];
    }
    const double T = b;
    acc = 0.0;
    for (int64_t it = lo; it < hi; ++it) {
        double *rec_it = sums + 4 * (first + it);
        rec_it[1] = run_base;
        rec_it[2] = acc;
        acc = acc + rec_it[0];
        rec_it[3] = run_base + acc;
        counts[3 * (first + it)] = 0;
    }
    if (threadIdx.x == 0) {
        totals[seg] = T;
        uint32_t *hdr = reinterpret_cast<uint32_t *>(wire + rec[3]);
        hdr[0] = __float_as_uint((float)T / (float)k);
        hdr[1] = hdr[2] = hdr[3] = 0u;
        uint32_t *words = hdr + HEADER / 4;
        for (int64_t p = k; p < ((k + 3) & ~(int64_t)3); ++p) words[p] = 0u;      // the section's padding
    }
}

// the tensor of draw d: the last one whose first draw is <= d (first draws ascend with the tensor index, no gaps)
__device__ __forceinline__ int seg_of_draw(const int64_t *__restrict__ seg_table, int nseg, int64_t d) {
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (seg_table[8 * (int64_t)mid + 6] <= d) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(THREADS) void maurey_count_kernel(const int64_t *__restrict__ seg_table, int nseg, int64_t ndraws,
                                                               const double *__restrict__ sums, const double *__restrict__ totals,
                                                               int32_t *__restrict__ counts, int32_t *__restrict__ draw_item,
                                                               int random_mode, const float *__restrict__ r, uint64_t seed) {
    gq::resolve_seed(random_mode, seed);
    const int64_t d = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (d >= ndraws) return;
    const int seg = seg_of_draw(seg_table, nseg, d);
    const int64_t *rec = seg_table + 8 * (int64_t)seg;
    const int64_t n = rec[1], first = rec[2];
    if (d < rec[6] || d - rec[6] >= rec[4]) {      // (a table whose draws have gaps: not a draw of any tensor)
        draw_item[d] = -1;
        return;
    }
    const double T = totals[seg];
    int64_t it = 0;
    if (!degenerate(T)) {
        const double t = draw_t(draw_u(random_mode, r, seed, d), T);
        int64_t lo = 0, hi = (n + CHUNK - 1) / CHUNK - 1;      // the smallest item whose last C is above t (the last one's is T)
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (t < sums[4 * (first + mid) + 3]) hi = mid;
            else lo = mid + 1;
        }
        it = lo;
    }
    draw_item[d] = (int32_t)(first + it);
    atomicAdd(&counts[3 * (first + it)], 1);
}

// one workgroup per tensor: counts -> every item's first output word (and the cursor the place launch advances)
__global__ __launch_bounds__(THREADS) void maurey_offsets_kernel(const int64_t *__restrict__ seg_table, int32_t *__restrict__ counts) {
    __shared__ uint32_t lds[WAVES];
    const int64_t *rec = seg_table + 8 * (int64_t)blockIdx.x;
    const int64_t n = rec[1], first = rec[2];
    const int64_t nit = (n + CHUNK - 1) / CHUNK;
    uint32_t carry = 0;
    for (int64_t b0 = 0; b0 < nit; b0 += THREADS) {
        const int64_t it = b0 + threadIdx.x;
        const uint32_t c = it < nit ? (uint32_t)counts[3 * (first + it)] : 0u;
        uint32_t tot;
        const uint32_t before = block_exclusive_scan(c, lds, &tot);
        if (it < nit) {
            counts[3 * (first + it) + 1] = (int32_t)(carry + before);
            counts[3 * (first + it) + 2] = (int32_t)(carry + before);
        }
        carry += tot;
        __syncthreads();      // (the next round rewrites lds)
    }
}

__global__ __launch_bounds__(THREADS) void maurey_place_kernel(const int64_t *__restrict__ seg_table, int nseg, int64_t ndraws,
                                                               int32_t *__restrict__ counts, const int32_t *__restrict__ draw_item,
                                                               float *__restrict__ bucket, int random_mode,
                                                               const float *__restrict__ r, uint64_t seed) {
    gq::resolve_seed(random_mode, seed);
    const int64_t d = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (d >= ndraws) return;
    const int32_t item = draw_item[d];
    if (item < 0) return;
    const int seg = seg_of_draw(seg_table, nseg, d);
    const int64_t *rec = seg_table + 8 * (int64_t)seg;
    const int64_t pos = (int64_t)(uint32_t)atomicAdd(&counts[3 * (int64_t)item + 2], 1);
    if (pos < rec[4]) bucket[rec[6] + pos] = draw_u(random_mode, r, seed, d);
}

template <bool EF>
__global__ __launch_bounds__(THREADS) void maurey_item_kernel(const int64_t *__restrict__ seg_table, const int32_t *__restrict__ item_seg,
                                                              const double *__restrict__ sums, const double *__restrict__ totals,
                                                              const int32_t *__restrict__ counts, const float *__restrict__ bucket,
                                                              uint8_t *__restrict__ wire, float *__restrict__ out, float ef_scale,
                                                              const int64_t *__restrict__ dense_table, int ndense) {
    copy_dense<THREADS>(dense_table, ndense, wire);
    __shared__ double cdf[PADDED];
    __shared__ uint32_t hit[PADDED];
    __shared__ double lds_tot[THREADS], lds_grp[16];
    __shared__ uint32_t sgn[THREADS], lds_scan[WAVES];
    const int64_t item = blockIdx.x;
    const int seg = item_seg[item];
    const int64_t *rec = seg_table + 8 * (int64_t)seg;
    const int64_t n = rec[1], k = rec[4];
    const double T = totals[seg];
    const bool degen = degenerate(T);
    const float scale = (float)T / (float)k;
    const uint32_t start = (uint32_t)counts[3 * item + 1];
    const uint32_t cnt = (uint32_t)counts[3 * item + 2] - start;      // (the place launch left the cursor behind the item's last draw)
    float *v = reinterpret_cast<float *>(rec[0]);
    float *err = EF ? reinterpret_cast<float *>(rec[7]) : nullptr;
    float *o = out ? out + rec[5] : nullptr;
    const bool dense_wanted = o != nullptr || (EF && err != nullptr);
    if (cnt == 0 && !dense_wanted) return;
    const int64_t base = (item - rec[2]) * CHUNK;
    const int64_t end = base + CHUNK < n ? base + CHUNK : n;
    const int len = (int)(end - base);
    float w[PER_THREAD];
    load_item<EF>(v, err, base, end, ef_scale, w);
    uint32_t neg = 0;
    if (!degen) {
#pragma unroll
        for (int j = 0; j < PER_THREAD; ++j) neg |= (__float_as_uint(w[j]) >> 31) << j;
    }
    uint32_t m[PER_THREAD];
#pragma unroll
    for (int j = 0; j < PER_THREAD; ++j) m[j] = 0u;
    const int e0 = (int)threadIdx.x * PER_THREAD;
    if (cnt != 0) {
        if (!degen) {
            double s[PER_THREAD], B, G, S;
            item_scan(w, s, lds_tot, lds_grp, B, G, S);
            const double run_base = sums[4 * item + 1], in_run = sums[4 * item + 2];
#pragma unroll
            for (int j = 0; j < PER_THREAD; ++j) cdf[phys(e0 + j)] = full_cdf(run_base, in_run, G, B, s[j]);
        }
        sgn[threadIdx.x] = neg;
#pragma unroll
        for (int j = 0; j < PER_THREAD; ++j) hit[phys(e0 + j)] = 0u;
        __syncthreads();
        // the item's draws, however many (one dominant element takes all k of a tensor): each to the smallest element whose C is above t
        const float *bk = bucket + rec[6] + start;
        for (uint32_t p = threadIdx.x; p < cnt; p += THREADS) {
            int e = 0;
            if (!degen) {
                const double t = draw_t(bk[p], T);
                int lo = 0, hi = CHUNK - 1;      // (elements past the tensor's end repeat the last C: never the smallest)
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (t < cdf[phys(mid)]) hi = mid;
                    else lo = mid + 1;
                }
                e = lo < len ? lo : len - 1;
            }
            atomicAdd(&hit[phys(e)], 1u);
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < PER_THREAD; ++j) m[j] = hit[phys(e0 + j)];
    }
    if (dense_wanted) {
        const int64_t i0 = base + e0;
#pragma unroll
        for (int j = 0; j < PER_THREAD; ++j) {
            if (i0 + j < end) {
                float dec = 0.0f;
                if (m[j] != 0u) dec = scale * ((neg >> j) & 1u ? -(float)m[j] : (float)m[j]);      // the reference's scale * recover
                if (o) o[i0 + j] = dec;
                if (EF && err) {
                    v[i0 + j] = w[j];
                    err[i0 + j] = w[j] - dec;
                }
            }
        }
    }
    if (cnt == 0) return;
    // inclusive hit counts in element order, in place; output word p is the first element whose count is above p
    uint32_t mine = 0;
#pragma unroll
    for (int j = 0; j < PER_THREAD; ++j) mine += m[j];
    uint32_t tot;
    uint32_t run = block_exclusive_scan(mine, lds_scan, &tot);
#pragma unroll
    for (int j = 0; j < PER_THREAD; ++j) {
        run += m[j];
        hit[phys(e0 + j)] = run;
    }
    __syncthreads();
    uint32_t *words = reinterpret_cast<uint32_t *>(wire + rec[3] + HEADER);
    for (uint32_t p = threadIdx.x; p < cnt; p += THREADS) {
        int lo = 0, hi = CHUNK - 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (p < hit[phys(mid)]) hi = mid;
            else lo = mid + 1;
        }
        const uint32_t sign = (sgn[lo >> 4] >> (lo & 15)) & 1u;
        if ((int64_t)start + p < k) words[start + p] = (uint32_t)(base + lo) | (sign << 31);
    }
}

// the first word of a[0, n) whose index (the low 31 bits) is >= x
__device__ __forceinline__ int64_t lower_bound_index(const uint32_t *__restrict__ a, int64_t n, int64_t x) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)(a[mid] & 0x7fffffffu) < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(THREADS) void maurey_decode_kernel(const int64_t *__restrict__ seg_table, const int32_t *__restrict__ item_seg,
                                                                const uint8_t *__restrict__ gathered, int64_t stride, int R,
                                                                float *__restrict__ out, int plain) {
    __shared__ float acc[CHUNK];
    __shared__ int32_t cnt[CHUNK];
    const int64_t item = blockIdx.x;
    const int seg = item_seg[item];
    const int64_t *rec = seg_table + 8 * (int64_t)seg;
    const int64_t n = rec[1], k = rec[4], off = rec[3];
    float *o = out + rec[5];
    const int64_t base = (item - rec[2]) * CHUNK;
    const int64_t end = base + CHUNK < n ? base + CHUNK : n;
    const uint32_t len = (uint32_t)(end - base);
    for (int t = threadIdx.x; t < CHUNK; t += THREADS) {
        acc[t] = 0.0f;
        cnt[t] = 0;
    }
    __syncthreads();
    const bool direct = plain && R == 1;
    for (int r = 0; r < R; ++r) {
        const uint8_t *p = gathered + (int64_t)r * stride + off;
        const float scale = *reinterpret_cast<const float *>(p);
        const uint32_t *words = reinterpret_cast<const uint32_t *>(p + HEADER);
        const int64_t lo = lower_bound_index(words, k, base), hi = lower_bound_index(words, k, end);
        for (int64_t j = lo + threadIdx.x; j < hi; j += THREADS) {
            const uint32_t wd = words[j];
            const uint32_t u = (wd & 0x7fffffffu) - (uint32_t)base;
            if (u < len) atomicAdd(&cnt[u], (wd >> 31) ? -1 : 1);      // integers: any order gives the same count
        }
        __syncthreads();
        for (uint32_t t = threadIdx.x; t < len; t += THREADS) {
            const int32_t c = cnt[t];
            if (c != 0) {
                const float d = scale * (float)c;      // one rounding: the reference's scale * recover
                acc[t] = direct ? d : acc[t] + d;
                cnt[t] = 0;
            }
        }
        __syncthreads();      // payloads in order: r + 1 adds to what r left
    }
    const float fR = (float)R;
    for (uint32_t t = threadIdx.x; t < len; t += THREADS) o[base + t] = direct ? acc[t] : acc[t] / fR;
}

static int check_batch(const gq_maurey_batch *b, const char *what, bool compress) {
    if (!b || b->struct_bytes != sizeof(gq_maurey_batch)) return fail(GQ_ERR_INVALID_ARG, "%s: descriptor missing or of another size", what);
    if (b->nseg < 1 || b->nitems < 1 || b->nitems > 0x7fffffff || b->ndense < 0)
        return fail(GQ_ERR_INVALID_ARG, "%s: bad sizes (nseg %d, nitems %lld, ndense %d)", what, b->nseg, (long long)b->nitems, b->ndense);
    if (!b->seg_table || !b->item_seg) return fail(GQ_ERR_INVALID_ARG, "%s: null table", what);
    if (compress) {
        if (b->ndraws < b->nseg || (b->ndraws + gqm::THREADS - 1) / gqm::THREADS > 0x7fffffff)
            return fail(GQ_ERR_INVALID_ARG, "%s: ndraws = %lld for %d tensors (k >= 1 each)", what, (long long)b->ndraws, b->nseg);
        if (!b->sums || !b->totals || !b->counts || !b->draw_item || !b->bucket || (b->ndense > 0 && !b->dense_table))
            return fail(GQ_ERR_INVALID_ARG, "%s: null scratch buffer", what);
    }
    return GQ_OK;
}

}  // namespace gqm

GQM_API int gq_maurey_abi_version(void) { return GQ_MAUREY_ABI_VERSION; }

GQM_API const char *gq_maurey_last_error(void) { return gqm::err_buf; }

template <bool EF>
static int maurey_compress(const gq_maurey_batch *b, uint8_t *wire, int random_mode, const float *r, uint64_t seed, float ef_scale,
                           float *out, hipStream_t st) {
    using namespace gqm;
    const dim3 items((unsigned)b->nitems), segs((unsigned)b->nseg), draws((unsigned)((b->ndraws + THREADS - 1) / THREADS)), block(THREADS);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(maurey_sum_kernel<EF>), items, block, 0, st, b->seg_table, b->item_seg, b->sums, ef_scale);
    GQL_CHECK_LAUNCH("gq_maurey_compress_batched (sum)");
    hipLaunchKernelGGL(maurey_scan_kernel, segs, block, 0, st, b->seg_table, b->sums, b->totals, b->counts, wire);
    GQL_CHECK_LAUNCH("gq_maurey_compress_batched (scan)");
    hipLaunchKernelGGL(maurey_count_kernel, draws, block, 0, st, b->seg_table, b->nseg, b->ndraws, b->sums, b->totals, b->counts,
                       b->draw_item, random_mode, r, seed);
    GQL_CHECK_LAUNCH("gq_maurey_compress_batched (count)");
    hipLaunchKernelGGL(maurey_offsets_kernel, segs, block, 0, st, b->seg_table, b->counts);
    GQL_CHECK_LAUNCH("gq_maurey_compress_batched (offsets)");
    hipLaunchKernelGGL(maurey_place_kernel, draws, block, 0, st, b->seg_table, b->nseg, b->ndraws, b->counts, b->draw_item, b->bucket,
                       random_mode, r, seed);
    GQL_CHECK_LAUNCH("gq_maurey_compress_batched (place)");
    hipLaunchKernelGGL(HIP_KERNEL_NAME(maurey_item_kernel<EF>), items, block, 0, st, b->seg_table, b->item_seg, b->sums, b->totals, b->counts,
                       b->bucket, wire, out, ef_scale, b->dense_table, b->ndense);
    GQL_CHECK_LAUNCH("gq_maurey_compress_batched (item)");
    return GQ_OK;
}

GQM_API int gq_maurey_compress_batched(const gq_maurey_batch *b, uint8_t *wire, int random_mode, const float *r, uint64_t seed,
                                       float ef_scale, float *out, void *stream) {
    const int rc = gqm::check_batch(b, "gq_maurey_compress_batched", true);
    if (rc != GQ_OK) return rc;
    if (!wire || (reinterpret_cast<uintptr_t>(wire) & 3) != 0)
        return gqm::fail(GQ_ERR_INVALID_ARG, "gq_maurey_compress_batched: the wire must be a 4-byte aligned device buffer");
    if (random_mode != GQ_RANDOM_GIVEN && random_mode != GQ_RANDOM_DEVICE && random_mode != GQ_RANDOM_DEVICE_COUNTER)
        return gqm::fail(GQ_ERR_INVALID_ARG, "gq_maurey_compress_batched: random_mode %d (given, device or device counter)", random_mode);
    if (random_mode == GQ_RANDOM_GIVEN && !r) return gqm::fail(GQ_ERR_INVALID_ARG, "gq_maurey_compress_batched: GQ_RANDOM_GIVEN without draws");
    if (random_mode == GQ_RANDOM_DEVICE_COUNTER && (seed == 0 || (seed & 7) != 0))
        return gqm::fail(GQ_ERR_INVALID_ARG, "gq_maurey_compress_batched: GQ_RANDOM_DEVICE_COUNTER needs the address of a { seed, step } pair");
    const bool ef = !isnan(ef_scale);
    if (ef && !out) return gqm::fail(GQ_ERR_INVALID_ARG, "gq_maurey_compress_batched: error feedback needs `out` (the decoded tensors)");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return ef ? maurey_compress<true>(b, wire, random_mode, r, seed, ef_scale, out, st)
              : maurey_compress<false>(b, wire, random_mode, r, seed, 0.0f, out, st);
}

GQM_API int gq_maurey_decode_sum_batched(const gq_maurey_batch *b, const uint8_t *gathered, int64_t user_stride_bytes, int R, float *out,
                                         int plain, void *stream) {
    const int rc = gqm::check_batch(b, "gq_maurey_decode_sum_batched", false);
    if (rc != GQ_OK) return rc;
    if (!gathered || !out) return gqm::fail(GQ_ERR_INVALID_ARG, "gq_maurey_decode_sum_batched: null pointer");
    if (R < 1 || (R > 1 && (user_stride_bytes < 0 || (user_stride_bytes & 3) != 0)))
        return gqm::fail(GQ_ERR_INVALID_ARG, "gq_maurey_decode_sum_batched: R = %d, user stride %lld", R, (long long)user_stride_bytes);
    if ((reinterpret_cast<uintptr_t>(gathered) & 3) != 0)
        return gqm::fail(GQ_ERR_INVALID_ARG, "gq_maurey_decode_sum_batched: the gathered wire must be 4-byte aligned");
    hipLaunchKernelGGL(gqm::maurey_decode_kernel, dim3((unsigned)b->nitems), dim3(gqm::THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                       b->seg_table, b->item_seg, gathered, user_stride_bytes, R, out, plain ? 1 : 0);
    GQL_CHECK_LAUNCH("gq_maurey_decode_sum_batched");
    return GQ_OK;
}
