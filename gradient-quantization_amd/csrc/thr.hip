// Threshold sparsification on a sparse wire with a variable count, multi-tensor (segment table) form -- libgq_thr.so
// (include/gq_thr.h, which defines every value here to the bit).
//
//   reduce(s) / pick(s), s = 1 .. S   the fit: a reduce launch leaves every fit item's count and f64 sum of |w| - eta_{s-1} over the
//                                     finite elements above eta_{s-1} (the contract's balanced tree: two levels inside a float4,
//                                     six across the wave, two across the waves, two across the four quarters of the item); the
//                                     pick launch (one workgroup per tensor) sums the items in the contract's tree and moves eta.
//   count / scan / write              top-k's compaction without the tie bookkeeping (csrc/sparse_kernels.hpp): per-item counts of
//                                     key > eta, their exclusive scan in index order, then every kept pair at its position --
//                                     ascending indices, the same bytes whatever order the workgroups run in -- plus the header,
//                                     the pad slots, the dense decoded tensor and the residual.
//   decode                            top-k's chunked binary-search decode-mean (the same header's) behind a header read and a clamp.
// No float or double atomics; every launch's arguments depend on the layout (and the caller's eta) alone.
#include <math.h>
#include <string.h>

#include "gq_lib_prelude.hpp"
#include "gq_thr.h"
#include "sparse_kernels.hpp"

#define GQH_API extern "C" __attribute__((visibility("default")))

namespace gqh {

using gql::copy_dense;
using gql::err_buf;
using gql::fail;
using gqsp::block_exclusive_scan;
using gqsp::key_of;
using gqsp::load_w;
using gqsp::THREADS;
using gqsp::WAVES;

constexpr int CHUNK = GQ_THR_CHUNK;
constexpr int PER_THREAD = CHUNK / THREADS;
constexpr int HDR = GQ_THR_HEADER_BYTES;
constexpr uint32_t INF_KEY = 0x7f800000u;
constexpr uint32_t MAX_ETA = 0x7f7fffffu;     // bits(FLT_MAX)
constexpr int RUN_LEVELS = 12;                // a thread of the pick launch sums a run of up to 2^11 fit items (n < 2^31: 2^19 items)
static_assert(CHUNK == 4 * 4 * THREADS, "the reduce launch's tree: four float4 per thread");
static_assert(sizeof(gq_thr_batch) == 88, "gq_thr_batch: the layout the ctypes binding declares (gq_amd/native.py)");

__device__ __forceinline__ int64_t cap_of(const int64_t *rec) { return rec[6] & 0xffffffffll; }
__device__ __forceinline__ int64_t stride_of(const int64_t *rec) {
    const int64_t m = rec[6] >> 32;
    return m < 1 ? 1 : m;
}

// six levels of the balanced tree across the wave: the neighbour at lane distance d is the slot at stride 4 d elements (a + b is
// b + a, so both lanes of a pair hold the pair's sum)
__device__ __forceinline__ double wave_tree(double s) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) s = s + __shfl_xor(s, d, 64);
    return s;
}

// the contract's gq_ln: f64 +, -, *, / in the header's order
__device__ __forceinline__ double gq_ln(double x) {
    const uint64_t b = (uint64_t)__double_as_longlong(x);
    int e = (int)(b >> 52) - 1023;
    uint64_t mb = (b & 0x000fffffffffffffull) | 0x3ff0000000000000ull;
    double mant = __longlong_as_double((long long)mb);
    if (mb > 0x3FF6A09E667F3BCDull) {
        mant = mant * 0.5;
        e = e + 1;
    }
    const double z = (mant - 1.0) / (mant + 1.0);
    const double y = z * z;
    const uint64_t C[12] = {0x3FF0000000000000ull, 0x3FD5555555555555ull, 0x3FC999999999999Aull, 0x3FC2492492492492ull,
                            0x3FBC71C71C71C71Cull, 0x3FB745D1745D1746ull, 0x3FB3B13B13B13B14ull, 0x3FB1111111111111ull,
                            0x3FAE1E1E1E1E1E1Eull, 0x3FAAF286BCA1AF28ull, 0x3FA8618618618618ull, 0x3FA642C8590B2164ull};
    double p = __longlong_as_double((long long)C[11]);
#pragma unroll
    for (int j = 10; j >= 0; --j) {
        p = p * y;
        p = p + __longlong_as_double((long long)C[j]);
    }
    const double a = (double)e * __longlong_as_double(0x3FE62E42FEFA39EFll);
    const double t = 2.0 * z;
    const double c = t * p;
    return a + c;
}

// one element's term of Sigma_s and of c_s
__device__ __forceinline__ double fit_term(float w, uint32_t eta_bits, double eta, uint32_t *c) {
    const uint32_t key = key_of(w);
    if (key > eta_bits && key < INF_KEY) {
        *c += 1u;
        return (double)__uint_as_float(key) - eta;
    }
    return 0.0;
}

// stage s of the fit, a workgroup per item (items that are no fit items leave at once): sums[item], counts[2 * item]
template <bool EF>
__global__ __launch_bounds__(THREADS) void thr_reduce_kernel(const int64_t *__restrict__ seg_table, const int32_t *__restrict__ item_seg,
                                                             const int32_t *__restrict__ state, double *__restrict__ sums,
                                                             int32_t *__restrict__ counts, int stage, float ef_scale) {
    __shared__ double part[4][WAVES];
    __shared__ uint32_t cpart[WAVES];
    const int64_t item = blockIdx.x;
    const int seg = item_seg[item];
    const int64_t *rec = seg_table + 8 * (int64_t)seg;
    const int64_t n = rec[1], li = item - rec[2];
    if (li % stride_of(rec) != 0) return;
    const uint32_t eta_bits = stage == 1 ? 0u : (uint32_t)state[4 * seg];
    const double eta = (double)__uint_as_float(eta_bits);
    const float *v = reinterpret_cast<const float *>(rec[0]);
    const float *err = EF ? reinterpret_cast<const float *>(rec[7]) : nullptr;
    const int64_t base = li * CHUNK;
    const int64_t end = base + CHUNK < n ? base + CHUNK : n;
    const bool vec = gql::aligned16(v) && (!err || gql::aligned16(err));
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t c = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t i = base + 4 * ((int64_t)q * THREADS + threadIdx.x);
        float w[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        bool in[4] = {i < end, i + 1 < end, i + 2 < end, i + 3 < end};
        if (vec && in[3]) {
            const float4 a = *reinterpret_cast<const float4 *>(v + i);
            w[0] = a.x, w[1] = a.y, w[2] = a.z, w[3] = a.w;
            if (EF && err) {
                const float4 r = *reinterpret_cast<const float4 *>(err + i);
                const float p0 = ef_scale * r.x, p1 = ef_scale * r.y, p2 = ef_scale * r.z, p3 = ef_scale * r.w;
                w[0] = w[0] + p0, w[1] = w[1] + p1, w[2] = w[2] + p2, w[3] = w[3] + p3;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (in[j]) w[j] = load_w<EF>(v, err, i + j, ef_scale);
        }
        double d[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            d[j] = 0.0;
            if (in[j]) d[j] = fit_term(w[j], eta_bits, eta, &c);
        }
        const double d01 = d[0] + d[1], d23 = d[2] + d[3];      // levels 0 and 1
        const double s = wave_tree(d01 + d23);                   // levels 2 .. 7
        if (lane == 0) part[q][wv] = s;
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) c += __shfl_xor(c, d, 64);
    if (lane == 0) cpart[wv] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        double a[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double lo = part[q][0] + part[q][1], hi = part[q][2] + part[q][3];      // levels 8 and 9
            a[q] = lo + hi;
        }
        const double lo = a[0] + a[1], hi = a[2] + a[3];      // levels 10 and 11
        sums[item] = lo + hi;
        counts[2 * item] = (int32_t)(cpart[0] + cpart[1] + cpart[2] + cpart[3]);
    }
}

// one workgroup per tensor: eta_s from the fit items' sums and counts -> state[0]
__global__ __launch_bounds__(THREADS) void thr_pick_kernel(const int64_t *__restrict__ seg_table, int32_t *__restrict__ state,
                                                           const double *__restrict__ sums, const int32_t *__restrict__ counts, int stage,
                                                           int stages) {
    __shared__ double part[WAVES];
    __shared__ uint32_t cpart[WAVES];
    const int seg = blockIdx.x;
    const int64_t *rec = seg_table + 8 * (int64_t)seg;
    const int64_t n = rec[1], first = rec[2], k = rec[4], m = stride_of(rec);
    const int64_t nit = (n + CHUNK - 1) / CHUNK;
    const int64_t nfit = (nit + m - 1) / m;                 // fit items: 0, m, 2 m, ...
    int64_t Q = 1;
    while (Q < nfit) Q <<= 1;
    const int64_t run = Q > THREADS ? Q / THREADS : 1;      // slots per thread, a power of two (at most 2^(RUN_LEVELS - 1))
    // the balanced tree over this thread's run: acc[l] holds the sum of a finished block of 2^l slots waiting for its neighbour
    double acc[RUN_LEVELS];
#pragma unroll
    for (int l = 0; l < RUN_LEVELS; ++l) acc[l] = 0.0;
    uint32_t c = 0;
    double s = 0.0;
    for (int64_t j = 0; j < run; ++j) {
        const int64_t slot = (int64_t)threadIdx.x * run + j;
        double carry = 0.0;
        if (slot < nfit) {
            carry = sums[first + slot * m];
            c += (uint32_t)counts[2 * (first + slot * m)];
        }
        bool placed = false;
#pragma unroll
        for (int l = 0; l < RUN_LEVELS; ++l) {
            if (!placed) {
                if ((j >> l) & 1) {
                    carry = acc[l] + carry;
                } else {
                    acc[l] = carry;
                    placed = true;
                }
            }
        }
        s = carry;      // (after the run's last slot: the whole run)
    }
    s = wave_tree(s);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) c += __shfl_xor(c, d, 64);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) {
        part[wv] = s;
        cpart[wv] = c;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double lo = part[0] + part[1], hi = part[2] + part[3];
    const double sigma = lo + hi;
    const uint32_t cs = cpart[0] + cpart[1] + cpart[2] + cpart[3];
    const uint32_t prev = stage == 1 ? 0u : (uint32_t)state[4 * seg];
    uint32_t next = prev;
    const int64_t last = (nfit - 1) * m;
    const int64_t n_fit = (nfit - 1) * CHUNK + (n - last * CHUNK < CHUNK ? n - last * CHUNK : CHUNK);
    const double cn = (double)cs * (double)n;
    const double chat = cn / (double)n_fit;
    if (cs != 0u && chat > (double)k) {
        const double beta = sigma / (double)cs;
        const double ratio = chat / (double)k;
        const double L = gq_ln(ratio) / (double)(stages - stage + 1);
        const double bl = beta * L;
        const double t = (double)__uint_as_float(prev) + bl;
        const uint32_t f = __float_as_uint((float)t);
        next = (f & 0x7fffffffu) >= INF_KEY ? MAX_ETA : f;
    }
    state[4 * seg] = (int32_t)next;
}

template <bool EF>
__global__ __launch_bounds__(THREADS) void thr_count_kernel(const int64_t *__restrict__ seg_table, const int32_t *__restrict__ item_seg,
                                                            const int32_t *__restrict__ state, int32_t *__restrict__ counts, int fixed,
                                                            uint32_t fixed_eta, float ef_scale) {
    __shared__ uint32_t lds[WAVES];
    const int64_t item = blockIdx.x;
    const int seg = item_seg[item];
    const int64_t *rec = seg_table + 8 * (int64_t)seg;
    const int64_t n = rec[1];
    const uint32_t T = fixed ? fixed_eta : (uint32_t)state[4 * seg];
    const float *v = reinterpret_cast<const float *>(rec[0]);
    const float *err = EF ? reinterpret_cast<const float *>(rec[7]) : nullptr;
    const int64_t base = (item - rec[2]) * CHUNK;
    const int64_t end = base + CHUNK < n ? base + CHUNK : n;
    uint32_t gt = 0;
    for (int64_t i = base + threadIdx.x; i < end; i += THREADS) gt += key_of(load_w<EF>(v, err, i, ef_scale)) > T ? 1u : 0u;
    uint32_t tg;
    block_exclusive_scan(gt, lds, &tg);
    if (threadIdx.x == 0) counts[2 * item + 1] = (int32_t)tg;
}

// one workgroup per tensor: the items' counts -> their exclusive prefix sums (in place), in index order; state[1] = found
__global__ __launch_bounds__(THREADS) void thr_scan_kernel(const int64_t *__restrict__ seg_table, int32_t *__restrict__ counts,
                                                           int32_t *__restrict__ state, int fixed, uint32_t fixed_eta) {
    const int64_t *rec = seg_table + 8 * (int64_t)blockIdx.x;
    const int64_t n = rec[1], first = rec[2];
    uint32_t found[1];
    gqsp::scan_item_counts<1, 1>(counts, first, (n + CHUNK - 1) / CHUNK, found);
    if (threadIdx.x == 0) {
        if (fixed) state[4 * blockIdx.x] = (int32_t)fixed_eta;
        state[4 * blockIdx.x + 1] = (int32_t)found[0];
    }
}

template <bool EF>
__global__ __launch_bounds__(THREADS) void thr_write_kernel(const int64_t *__restrict__ seg_table, const int32_t *__restrict__ item_seg,
                                                            const int32_t *__restrict__ state, const int32_t *__restrict__ counts,
                                                            uint8_t *__restrict__ wire, float *__restrict__ out, float ef_scale,
                                                            const int64_t *__restrict__ dense_table, int ndense) {
    copy_dense<THREADS>(dense_table, ndense, wire);
    const int64_t item = blockIdx.x;
    const int seg = item_seg[item];
    const int64_t *rec = seg_table + 8 * (int64_t)seg;
    const int64_t n = rec[1], cap = cap_of(rec), li = item - rec[2];
    const uint32_t T = (uint32_t)state[4 * seg], found = (uint32_t)state[4 * seg + 1];
    const uint32_t kept_n = found < (uint64_t)cap ? found : (uint32_t)cap;
    uint32_t gt_before = (uint32_t)counts[2 * item + 1];
    float *v = reinterpret_cast<float *>(rec[0]);
    float *err = EF ? reinterpret_cast<float *>(rec[7]) : nullptr;
    uint32_t *hdr = reinterpret_cast<uint32_t *>(wire + rec[3]);
    uint32_t *idx = hdr + HDR / 4;
    float *val = reinterpret_cast<float *>(idx + cap);
    float *o = out ? out + rec[5] : nullptr;
    // the header, the slots that hold no pair and the section's last zero bytes: shared out among the tensor's items
    const int64_t nit = (n + CHUNK - 1) / CHUNK;
    if (li == 0 && threadIdx.x < 4) {
        hdr[threadIdx.x] = threadIdx.x == 0 ? kept_n : (threadIdx.x == 1 ? found : (threadIdx.x == 2 ? T : 0u));
        if ((cap & 1) && threadIdx.x < 2) reinterpret_cast<uint32_t *>(val + cap)[threadIdx.x] = 0u;
    }
    for (int64_t j = (int64_t)kept_n + li * THREADS + threadIdx.x; j < cap; j += nit * THREADS) {
        idx[j] = GQ_THR_NO_INDEX;
        val[j] = 0.0f;
    }
    const int64_t base = li * CHUNK;
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
        const gqsp::Rank r = gqsp::rank_step<false>(s, is_gt, false, gt_before, 0u);
        const bool kept = is_gt && r.gb < (uint64_t)cap;
        if (kept) {
            idx[r.gb] = (uint32_t)i;
            val[r.gb] = w;
        }
        if (valid) gqsp::store_decoded<EF>(v, err, o, i, w, w * (kept ? 1.0f : 0.0f));
        gt_before += r.tg;
    }
}

__global__ __launch_bounds__(THREADS) void thr_decode_kernel(const int64_t *__restrict__ seg_table, const int32_t *__restrict__ item_seg,
                                                             const uint8_t *__restrict__ gathered, int64_t stride, int R,
                                                             float *__restrict__ out, int plain) {
    __shared__ float acc[CHUNK];
    const int64_t item = blockIdx.x;
    const int seg = item_seg[item];
    const int64_t *rec = seg_table + 8 * (int64_t)seg;
    const int64_t n = rec[1], cap = cap_of(rec), off = rec[3];
    float *o = out + rec[5];
    const int64_t base = (item - rec[2]) * CHUNK;
    const int64_t end = base + CHUNK < n ? base + CHUNK : n;
    const uint32_t len = (uint32_t)(end - base);
    gqsp::decode_clear<CHUNK>(acc);
    const bool direct = plain && R == 1;
    for (int r = 0; r < R; ++r) {
        const uint8_t *p = gathered + (int64_t)r * stride + off;
        const uint32_t kept = *reinterpret_cast<const uint32_t *>(p);
        const int64_t kk = kept < (uint64_t)cap ? (int64_t)kept : cap;
        gqsp::decode_add_pairs(acc, reinterpret_cast<const uint32_t *>(p + HDR), reinterpret_cast<const float *>(p + HDR + 4 * cap), kk, base, end,
                               len, direct);
    }
    gqsp::decode_store_mean(acc, o, base, len, R, direct);
}

static int check_batch(const gq_thr_batch *b, const char *what, bool compress) {
    const int rc = gqsp::check_batch_common(b, what);
    if (rc != GQ_OK) return rc;
    if (b->min_k < 1 || b->min_cap < 1 || b->min_stride < 1)
        return fail(GQ_ERR_INVALID_ARG, "%s: k = %d, cap = %d, fit stride = %d (each must be at least 1)", what, b->min_k, b->min_cap,
                    b->min_stride);
    if (compress && (!b->sums || !b->state || !b->counts || (b->ndense > 0 && !b->dense_table)))
        return fail(GQ_ERR_INVALID_ARG, "%s: null scratch buffer", what);
    return GQ_OK;
}

}  // namespace gqh

GQH_API int gq_thr_abi_version(void) { return GQ_THR_ABI_VERSION; }

GQH_API const char *gq_thr_last_error(void) { return gqh::err_buf; }

template <bool EF>
static int thr_compress(const gq_thr_batch *b, uint8_t *wire, uint32_t eta_bits, float ef_scale, float *out, hipStream_t st) {
    using namespace gqh;
    const dim3 items((unsigned)b->nitems), segs((unsigned)b->nseg), block(THREADS);
    const int S = b->stages, fixed = S == 0 ? 1 : 0;
    for (int s = 1; s <= S; ++s) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(thr_reduce_kernel<EF>), items, block, 0, st, b->seg_table, b->item_seg, b->state, b->sums,
                           b->counts, s, ef_scale);
        GQL_CHECK_LAUNCH("gq_thr_compress_batched (reduce)");
        hipLaunchKernelGGL(thr_pick_kernel, segs, block, 0, st, b->seg_table, b->state, b->sums, b->counts, s, S);
        GQL_CHECK_LAUNCH("gq_thr_compress_batched (pick)");
    }
    hipLaunchKernelGGL(HIP_KERNEL_NAME(thr_count_kernel<EF>), items, block, 0, st, b->seg_table, b->item_seg, b->state, b->counts, fixed,
                       eta_bits, ef_scale);
    GQL_CHECK_LAUNCH("gq_thr_compress_batched (count)");
    hipLaunchKernelGGL(thr_scan_kernel, segs, block, 0, st, b->seg_table, b->counts, b->state, fixed, eta_bits);
    GQL_CHECK_LAUNCH("gq_thr_compress_batched (scan)");
    hipLaunchKernelGGL(HIP_KERNEL_NAME(thr_write_kernel<EF>), items, block, 0, st, b->seg_table, b->item_seg, b->state, b->counts, wire, out,
                       ef_scale, b->dense_table, b->ndense);
    GQL_CHECK_LAUNCH("gq_thr_compress_batched (write)");
    return GQ_OK;
}

GQH_API int gq_thr_compress_batched(const gq_thr_batch *b, uint8_t *wire, float eta, float ef_scale, float *out, void *stream) {
    const int rc = gqh::check_batch(b, "gq_thr_compress_batched", true);
    if (rc != GQ_OK) return rc;
    if (!wire || (reinterpret_cast<uintptr_t>(wire) & 15) != 0)
        return gqh::fail(GQ_ERR_INVALID_ARG, "gq_thr_compress_batched: the wire must be a 16-byte aligned device address");
    if ((reinterpret_cast<uintptr_t>(out) & 3) != 0) return gqh::fail(GQ_ERR_INVALID_ARG, "gq_thr_compress_batched: `out` must be 4-byte aligned");
    if (b->stages < 0 || b->stages > GQ_THR_MAX_STAGES)
        return gqh::fail(GQ_ERR_INVALID_ARG, "gq_thr_compress_batched: stages = %d (0 ... %d)", b->stages, GQ_THR_MAX_STAGES);
    uint32_t eta_bits = 0;
    if (b->stages == 0) {
        memcpy(&eta_bits, &eta, 4);
        if (eta_bits > gqh::MAX_ETA)      // (a set sign bit, an infinity and every NaN compare above bits(FLT_MAX))
            return gqh::fail(GQ_ERR_INVALID_ARG, "gq_thr_compress_batched: a fixed threshold must lie in [+0, FLT_MAX], got bits 0x%08x", eta_bits);
    }
    const bool ef = !isnan(ef_scale);
    if (ef && !out) return gqh::fail(GQ_ERR_INVALID_ARG, "gq_thr_compress_batched: error feedback needs `out` (the decoded tensors)");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return ef ? thr_compress<true>(b, wire, eta_bits, ef_scale, out, st) : thr_compress<false>(b, wire, eta_bits, 0.0f, out, st);
}

GQH_API int gq_thr_decode_sum_batched(const gq_thr_batch *b, const uint8_t *gathered, int64_t user_stride_bytes, int R, float *out,
                                      int plain, void *stream) {
    int rc = gqh::check_batch(b, "gq_thr_decode_sum_batched", false);
    if (rc == GQ_OK) rc = gqsp::check_payloads("gq_thr_decode_sum_batched", gathered, out, user_stride_bytes, R);
    if (rc != GQ_OK) return rc;
    if (plain && R != 1) return gqh::fail(GQ_ERR_INVALID_ARG, "gq_thr_decode_sum_batched: plain takes one payload, got R = %d", R);
    if ((reinterpret_cast<uintptr_t>(gathered) & 3) != 0 || (reinterpret_cast<uintptr_t>(out) & 3) != 0)
        return gqh::fail(GQ_ERR_INVALID_ARG, "gq_thr_decode_sum_batched: the gathered wire and `out` must be 4-byte aligned");
    hipLaunchKernelGGL(gqh::thr_decode_kernel, dim3((unsigned)b->nitems), dim3(gqh::THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                       b->seg_table, b->item_seg, gathered, user_stride_bytes, R, out, plain ? 1 : 0);
    GQL_CHECK_LAUNCH("gq_thr_decode_sum_batched");
    return GQ_OK;
}
