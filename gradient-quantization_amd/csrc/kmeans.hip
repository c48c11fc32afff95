// Lloyd k-means for HSQ codebooks, bit-defined -- libgq_kmeans.so (include/gq_kmeans.h states the contract; the step numbers
// below are its).
//
// zero      the workspace (S, n) to zero, once per call; every update launch leaves it zero again.
// assign    the plain exact form.  A lane keeps P points' d floats in registers (P = 4, 2 or 1, so that at most 64 registers
//           hold points); the codebook sits in LDS in chunks of `rows` rows (row stride 4 * D4 floats, D4 = ceil(d / 4), with
//           the half norms behind it) and is read as broadcasts, one ds_read_b128 feeding 4 * P fused multiply-adds per lane.
//           k is walked in order, over the chunks in order, with a strict `>`, so the lowest index wins a tie within a chunk
//           and across chunks.  A workgroup strides over passes of THREADS * P points; with more than one chunk it stages the
//           codebook again for every pass (K * d floats from L2 against THREADS * P * K * d multiply-adds).
//           Accumulation (step 4): 64-bit integer atomic adds, into per-workgroup partial sums in LDS that the workgroup folds
//           into the workspace when it ends (non-zero words only), or, where K * (d + 1) words do not fit, into the workspace
//           directly.  Integer sums do not depend on the order, so both give the same bits.
// update    one lane per centroid row (step 5): the row, counts[k] = n_k, and the row's words of the workspace back to zero.
#include <math.h>

#include "gq_kmeans.h"
#include "gq_lib_prelude.hpp"

#define GQK_API extern "C" __attribute__((visibility("default")))

namespace gqk {

using gql::aligned16;
using gql::err_buf;
using gql::fail;

constexpr int THREADS = GQ_KMEANS_THREADS;
constexpr int LDS_BYTES = 61440;      // dynamic LDS of the assign launch at the most: partial sums + codebook chunk + half norms
constexpr int ACC_NONE = 0, ACC_LDS = 1, ACC_GLOBAL = 2;

__host__ __device__ constexpr int points_per_lane(int D4) { return D4 <= 4 ? 4 : D4 <= 8 ? 2 : 1; }

typedef unsigned long long u64;

__global__ __launch_bounds__(THREADS) void kmeans_zero_kernel(u64 *__restrict__ ws, int64_t words) {
    for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < words; i += (int64_t)gridDim.x * THREADS) ws[i] = 0;
}

// S_kj += sign * q_ij, n_k += 1 for one point (step 4); S and n are the workgroup's partials in LDS or the workspace
template <int D4>
__device__ __forceinline__ void accumulate(u64 *S, u64 *n, const float (&x)[4 * D4], int d, int label, bool negative) {
    u64 *row = S + (size_t)label * d;
#pragma unroll
    for (int j = 0; j < 4 * D4; ++j) {
        if (j < 4 * (D4 - 1) || j < d) {
            const long long q = __double2ll_rn((double)x[j] * 0x1p40);
            atomicAdd(row + j, (u64)(negative ? -q : q));
        }
    }
    atomicAdd(n + label, (u64)1);
}

template <int D4, int METRIC>
__global__ __launch_bounds__(THREADS) void kmeans_assign_kernel(const float *__restrict__ X, int N, int d, const float *__restrict__ C, int K,
                                                                int rows, int acc_mode, int32_t *__restrict__ labels,
                                                                int8_t *__restrict__ signs, u64 *__restrict__ S, u64 *__restrict__ n) {
    constexpr int P = points_per_lane(D4), STRIDE = 4 * D4;
    extern __shared__ __align__(16) unsigned char smem[];
    // [ partial S: K * d words | partial n: K words ] (ACC_LDS only, padded to 16 bytes) [ chunk: rows * STRIDE floats ] [ h: rows floats ]
    const int part_words = acc_mode == ACC_LDS ? K * (d + 1) : 0;
    u64 *Sl = reinterpret_cast<u64 *>(smem), *nl = Sl + (size_t)K * d;
    float *cb = reinterpret_cast<float *>(smem + (((size_t)part_words * 8 + 15) & ~(size_t)15));
    float *hl = cb + (size_t)rows * STRIDE;
    const int tid = threadIdx.x;
    for (int i = tid; i < part_words; i += THREADS) Sl[i] = 0;
    const int nchunks = (K + rows - 1) / rows;
    const bool vec = aligned16(X) && (d & 3) == 0;
    const int per_pass = THREADS * P;
    const int passes = (N + per_pass - 1) / per_pass;
    for (int pass = blockIdx.x; pass < passes; pass += gridDim.x) {
        float x[P][STRIDE];
        int idx[P];
#pragma unroll
        for (int p = 0; p < P; ++p) {
            idx[p] = pass * per_pass + p * THREADS + tid;
            const bool live = idx[p] < N;
            const float *src = X + (size_t)(live ? idx[p] : 0) * d;
            if (vec) {
#pragma unroll
                for (int g = 0; g < D4; ++g) {
                    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    if (live && 4 * g < d) v = *reinterpret_cast<const float4 *>(src + 4 * g);
                    x[p][4 * g] = v.x, x[p][4 * g + 1] = v.y, x[p][4 * g + 2] = v.z, x[p][4 * g + 3] = v.w;
                }
            } else {
#pragma unroll
                for (int j = 0; j < STRIDE; ++j) x[p][j] = live && j < d ? src[j] : 0.0f;
            }
        }
        float best[P], bdot[P];
        int bk[P];
#pragma unroll
        for (int p = 0; p < P; ++p) best[p] = 0.0f, bdot[p] = 0.0f, bk[p] = 0;
        for (int chunk = 0; chunk < nchunks; ++chunk) {
            const int k0 = chunk * rows, nrows = min(rows, K - k0);
            if (nchunks > 1 || pass == (int)blockIdx.x) {      // (uniform over the workgroup) one chunk: staged once and kept
                __syncthreads();                                // the previous chunk's readers are done
                for (int i = tid; i < nrows * d; i += THREADS) {
                    const int r = i / d, j = i - r * d;
                    cb[r * STRIDE + j] = C[(size_t)k0 * d + i];
                }
                __syncthreads();
                if (METRIC == GQ_KMEANS_EUCLID) {
                    for (int r = tid; r < nrows; r += THREADS) {      // step 1
                        float hn = 0.0f;
                        for (int j = 0; j < d; ++j) hn = fmaf(cb[r * STRIDE + j], cb[r * STRIDE + j], hn);
                        hl[r] = 0.5f * hn;
                    }
                    __syncthreads();
                }
            }
            for (int r = 0; r < nrows; ++r) {
                const float4 *crow = reinterpret_cast<const float4 *>(cb + r * STRIDE);
                float acc[P];
#pragma unroll
                for (int p = 0; p < P; ++p) acc[p] = 0.0f;
#pragma unroll
                for (int g = 0; g < D4; ++g) {
                    const float4 c4 = crow[g];      // the same address in every lane: a broadcast
                    const float c[4] = {c4.x, c4.y, c4.z, c4.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if (g < D4 - 1 || 4 * g + e < d) {      // (the words of a row past d are never multiplied: the chain has d steps)
#pragma unroll
                            for (int p = 0; p < P; ++p) acc[p] = fmaf(x[p][4 * g + e], c[e], acc[p]);      // step 2
                        }
                    }
                }
                const float h = METRIC == GQ_KMEANS_EUCLID ? hl[r] : 0.0f;
                const int k = k0 + r;
#pragma unroll
                for (int p = 0; p < P; ++p) {
                    const float t = METRIC == GQ_KMEANS_EUCLID ? acc[p] - h : fabsf(acc[p]);
                    if (k == 0 || t > best[p]) best[p] = t, bdot[p] = acc[p], bk[p] = k;      // step 3
                }
            }
        }
#pragma unroll
        for (int p = 0; p < P; ++p) {
            if (idx[p] < N) {
                const bool negative = METRIC == GQ_KMEANS_ABSDOT && bdot[p] < 0.0f;
                labels[idx[p]] = bk[p];
                if (signs) signs[idx[p]] = negative ? -1 : 1;
                if (acc_mode == ACC_LDS) accumulate<D4>(Sl, nl, x[p], d, bk[p], negative);
                else if (acc_mode == ACC_GLOBAL) accumulate<D4>(S, n, x[p], d, bk[p], negative);
            }
        }
    }
    if (acc_mode == ACC_LDS) {      // fold this workgroup's partials into the workspace (S and n are one run of words there too)
        __syncthreads();
        for (int i = tid; i < part_words; i += THREADS) {
            const u64 v = Sl[i];
            if (v) atomicAdd(S + i, v);
        }
    }
}

// step 5, one lane per row; leaves the row's words of the workspace zero for the next iteration
__global__ __launch_bounds__(THREADS) void kmeans_update_kernel(float *__restrict__ C, int K, int d, int metric, u64 *__restrict__ S,
                                                                u64 *__restrict__ n, int64_t *__restrict__ counts) {
    const int k = blockIdx.x * THREADS + threadIdx.x;
    if (k >= K) return;
    const long long nk = (long long)n[k];
    u64 *row = S + (size_t)k * d;
    float *c = C + (size_t)k * d;
    counts[k] = nk;
    n[k] = 0;
    if (nk != 0) {
        if (metric == GQ_KMEANS_EUCLID) {
            const double den = (double)nk * 0x1p40;
            for (int j = 0; j < d; ++j) c[j] = (float)((double)(long long)row[j] / den);
        } else {
            double ss = 0.0;
            for (int j = 0; j < d; ++j) {
                const double f = (double)(long long)row[j];
                const double sq = f * f;
                ss = ss + sq;
            }
            const double r = sqrt(ss);
            if (r != 0.0)
                for (int j = 0; j < d; ++j) c[j] = (float)((double)(long long)row[j] / r);
        }
    }
    for (int j = 0; j < d; ++j) row[j] = 0;
}

struct Plan {
    int D4, rows, acc_mode, grid;
    size_t lds;
};

static Plan plan(int N, int d, int K, int acc_mode) {
    Plan p;
    p.D4 = (d + 3) / 4;
    if (acc_mode == ACC_LDS && (size_t)8 * K * (d + 1) > GQ_KMEANS_LDS_PARTIAL_BYTES) acc_mode = ACC_GLOBAL;
    p.acc_mode = acc_mode;
    const size_t part = acc_mode == ACC_LDS ? (((size_t)8 * K * (d + 1) + 15) & ~(size_t)15) : 0;
    const size_t row_bytes = (size_t)4 * (4 * p.D4 + 1);
    const size_t fit = (LDS_BYTES - part) / row_bytes;
    p.rows = (int)(fit < (size_t)K ? fit : (size_t)K);
    p.lds = part + p.rows * row_bytes;
    const int per_pass = THREADS * points_per_lane(p.D4);
    const int64_t passes = ((int64_t)N + per_pass - 1) / per_pass, cap = (int64_t)gql::cu_count() * GQ_KMEANS_BLOCKS_PER_CU;
    p.grid = (int)(passes < cap ? passes : cap);
    return p;
}

template <int D4>
static void launch_assign(const Plan &p, int metric, hipStream_t st, const float *X, int N, int d, const float *C, int K, int32_t *labels,
                          int8_t *signs, u64 *S, u64 *n) {
    if (metric == GQ_KMEANS_EUCLID)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(kmeans_assign_kernel<D4, GQ_KMEANS_EUCLID>), dim3(p.grid), dim3(THREADS), p.lds, st, X, N, d, C, K,
                           p.rows, p.acc_mode, labels, signs, S, n);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(kmeans_assign_kernel<D4, GQ_KMEANS_ABSDOT>), dim3(p.grid), dim3(THREADS), p.lds, st, X, N, d, C, K,
                           p.rows, p.acc_mode, labels, signs, S, n);
}

static void assign(const Plan &p, int metric, hipStream_t st, const float *X, int N, int d, const float *C, int K, int32_t *labels,
                   int8_t *signs, u64 *S, u64 *n) {
    switch (p.D4) {
#define GQK_CASE(D4) case D4: launch_assign<D4>(p, metric, st, X, N, d, C, K, labels, signs, S, n); break;
        GQK_CASE(1) GQK_CASE(2) GQK_CASE(3) GQK_CASE(4) GQK_CASE(5) GQK_CASE(6) GQK_CASE(7) GQK_CASE(8)
        GQK_CASE(9) GQK_CASE(10) GQK_CASE(11) GQK_CASE(12) GQK_CASE(13) GQK_CASE(14) GQK_CASE(15) GQK_CASE(16)
#undef GQK_CASE
    }
}

static int check(const char *what, const void *X, int64_t N, int d, const void *C, int K, int metric, const void *labels) {
    if (!X || !C || !labels) return fail(GQ_ERR_INVALID_ARG, "%s: null pointer", what);
    if (N < 1 || d < 1 || K < 1) return fail(GQ_ERR_INVALID_ARG, "%s: N = %lld, d = %d, K = %d (each must be at least 1)", what, (long long)N, d, K);
    if (metric != GQ_KMEANS_EUCLID && metric != GQ_KMEANS_ABSDOT) return fail(GQ_ERR_INVALID_ARG, "%s: unknown metric %d", what, metric);
    if (N > GQ_KMEANS_MAX_N || d > GQ_KMEANS_MAX_D || K > GQ_KMEANS_MAX_K)
        return fail(GQ_ERR_UNSUPPORTED, "%s: N = %lld, d = %d, K = %d (supported: N <= %d, d <= %d, K <= %d)", what, (long long)N, d, K,
                    GQ_KMEANS_MAX_N, GQ_KMEANS_MAX_D, GQ_KMEANS_MAX_K);
    if (((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(C) | reinterpret_cast<uintptr_t>(labels)) & 3) != 0)
        return fail(GQ_ERR_INVALID_ARG, "%s: X, C and labels must be 4-byte aligned", what);
    return GQ_OK;
}

}  // namespace gqk

GQK_API int gq_kmeans_abi_version(void) { return GQ_KMEANS_ABI_VERSION; }

GQK_API const char *gq_kmeans_last_error(void) { return gqk::err_buf; }

GQK_API size_t gq_kmeans_workspace_bytes(int K, int d) {
    if (K < 1 || K > GQ_KMEANS_MAX_K || d < 1 || d > GQ_KMEANS_MAX_D) return 0;
    return (size_t)8 * K * (d + 1);
}

GQK_API int gq_kmeans_assign(const float *X, int64_t N, int d, const float *C, int K, int metric, int32_t *labels, int8_t *signs,
                             void *stream) {
    using namespace gqk;
    const int rc = check("gq_kmeans_assign", X, N, d, C, K, metric, labels);
    if (rc != GQ_OK) return rc;
    assign(plan((int)N, d, K, ACC_NONE), metric, reinterpret_cast<hipStream_t>(stream), X, (int)N, d, C, K, labels, signs, nullptr, nullptr);
    GQL_CHECK_LAUNCH("gq_kmeans_assign");
    return GQ_OK;
}

GQK_API int gq_kmeans_run(const float *X, int64_t N, int d, float *C, int K, int metric, int iters, int32_t *labels, int8_t *signs,
                          int64_t *counts, void *workspace, void *stream) {
    using namespace gqk;
    const bool global = metric >= 0 && (metric & GQ_KMEANS_GLOBAL_ATOMICS) != 0;
    if (global) metric &= ~GQ_KMEANS_GLOBAL_ATOMICS;
    const int rc = check("gq_kmeans_run", X, N, d, C, K, metric, labels);
    if (rc != GQ_OK) return rc;
    if (!counts || !workspace) return fail(GQ_ERR_INVALID_ARG, "gq_kmeans_run: null pointer");
    if (iters < 1) return fail(GQ_ERR_INVALID_ARG, "gq_kmeans_run: iters = %d (must be at least 1)", iters);
    if (((reinterpret_cast<uintptr_t>(counts) | reinterpret_cast<uintptr_t>(workspace)) & 7) != 0)
        return fail(GQ_ERR_INVALID_ARG, "gq_kmeans_run: counts and workspace must be 8-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    u64 *S = reinterpret_cast<u64 *>(workspace), *n = S + (size_t)K * d;
    const int64_t words = (int64_t)K * (d + 1);
    const Plan p = plan((int)N, d, K, global ? ACC_GLOBAL : ACC_LDS);
    const int64_t zero_blocks = (words + THREADS - 1) / THREADS;
    hipLaunchKernelGGL(kmeans_zero_kernel, dim3((unsigned)(zero_blocks < 1024 ? zero_blocks : 1024)), dim3(THREADS), 0, st, S, words);
    GQL_CHECK_LAUNCH("gq_kmeans_run (zero)");
    for (int it = 0; it < iters; ++it) {
        assign(p, metric, st, X, (int)N, d, C, K, labels, signs, S, n);
        GQL_CHECK_LAUNCH("gq_kmeans_run (assign)");
        hipLaunchKernelGGL(kmeans_update_kernel, dim3((K + THREADS - 1) / THREADS), dim3(THREADS), 0, st, C, K, d, metric, S, n, counts);
        GQL_CHECK_LAUNCH("gq_kmeans_run (update)");
    }
    return GQ_OK;
}
