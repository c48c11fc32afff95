// Low-rank gradient compression (PowerSGD, rank 1 / 2 / 4), multi-tensor (segment table) form -- libgq_psgd.so
// (include/gq_psgd.h: every operation and the shape of every reduction).
//
// A record is four launches, five where the residual or the dense decode is asked for:
//   (A) project      one workgroup per item (whole rows, or one piece of a long row).  Streams M (error feedback: M' = M + s * e,
//                    stored into e so that (C) and (D) read one array).  Short rows: a wave per row, the header's 256 strided
//                    accumulators as four per lane, its halvings 128 and 64 inside the lane, 32 ... 1 as lane shifts.  A piece of a
//                    long row: a thread per accumulator, 128 and 64 through LDS.  The same tree either way.  Partial P -> pwork.
//   (B) orthogonalise one workgroup per tensor.  Folds the pieces, then modified Gram-Schmidt in place in the wire's Ph region:
//                    thread t owns rows t, t + 256, ... throughout, so only the dot products cross threads.  Writes the header
//                    and the reset flags.
//   (C) back-project one workgroup per tile of 64 rows x 256 columns: a lane owns a column, the block's Ph rows sit in LDS, the
//                    chain runs down the rows; partials -> cpart.
//   (C') fold        the tiles of row block 0: the blocks' partials in order -> Q' into the wire and into the warm start (Q0's
//                    column where the flag says so), the section's zero bytes.
//   (D) residual     the decode kernel over the wire just written: e = M' - D and / or the dense decode.
// decode-mean        one workgroup per tile; a wave owns 16 rows, a lane 4 columns: a payload's 4 x r values of Q' stay in
//                    registers over the 16 rows, Ph's row values are wave-uniform loads; 16-byte stores where `out` allows.
// No atomics; every launch's arguments depend on the layout alone.
#include <math.h>

#include "gq_common.hpp"
#include "gq_lib_prelude.hpp"
#include "gq_psgd.h"

#define GQP_API extern "C" __attribute__((visibility("default")))

namespace gqp {

constexpr int THREADS = 256;
constexpr int PIECE = GQ_PSGD_PIECE;
constexpr int RB = GQ_PSGD_ROW_BLOCK;
constexpr int TC = GQ_PSGD_TILE_COLS;
static_assert(THREADS == 256 && TC == 256 && RB == 64, "the tree of include/gq_psgd.h is written out for 256 accumulators; a tile is 4 waves x 16 rows");
static_assert(sizeof(gq_psgd_batch) == 112, "gq_psgd_batch: the layout the ctypes binding declares (gq_amd/native.py)");

using gql::aligned16;
using gql::copy_dense;
using gql::err_buf;
using gql::fail;

// the halvings 32 ... 1 of the tree over the lanes of a wave; lane 0 has the result
__device__ __forceinline__ float wave_tree(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = v + __shfl_down(v, d, 64);
    return v;
}

// tree(x) over the workgroup's 256 values, the result to every thread.  lds: 257 floats, free on entry and on return.
__device__ __forceinline__ float block_tree(float x, float *lds) {
    const int t = threadIdx.x;
    lds[t] = x;
    __syncthreads();
    if (t < 64) {
        const float v = wave_tree((lds[t] + lds[t + 128]) + (lds[t + 64] + lds[t + 192]));
        if (t == 0) lds[256] = v;
    }
    __syncthreads();
    const float r = lds[256];
    __syncthreads();
    return r;
}

template <int R_, bool EF>
__global__ __launch_bounds__(THREADS) void psgd_project_kernel(const int64_t *__restrict__ seg_table, const int64_t *__restrict__ lay,
                                                               const int32_t *__restrict__ aitem_seg, const int64_t *__restrict__ state,
                                                               float *__restrict__ pwork, uint8_t *__restrict__ wire, float ef_scale,
                                                               const int64_t *__restrict__ dense_table, int ndense) {
    copy_dense<THREADS>(dense_table, ndense, wire);
    __shared__ float lds[R_][THREADS];
    const int64_t item = blockIdx.x;
    const int seg = aitem_seg[item];
    const int64_t *rec = seg_table + 8 * (int64_t)seg;
    const int64_t *L = lay + 4 * (int64_t)seg;
    const int64_t n = rec[4], m = rec[1] / n, t = item - L[0];
    const float *M = reinterpret_cast<const float *>(rec[0]);
    float *e = EF ? reinterpret_cast<float *>(rec[7]) : nullptr;
    const float *Q = reinterpret_cast<const float *>(state[2 * (int64_t)seg]);
    float *pw = pwork + L[1];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (m <= PIECE) {
        const int64_t per = PIECE / m > 1 ? PIECE / m : 1;
        const int64_t row0 = t * per, row1 = row0 + per < n ? row0 + per : n;
        for (int64_t i = row0 + wv; i < row1; i += THREADS / 64) {
            float acc[4][R_];
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int j = 0; j < R_; ++j) acc[k][j] = 0.0f;
            for (int64_t c0 = 0; c0 < m; c0 += 256) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int64_t c = c0 + 64 * k + lane;
                    if (c < m) {
                        float x = M[i * m + c];
                        if (EF) {
                            const float p = ef_scale * e[i * m + c];
                            x = x + p;
                            e[i * m + c] = x;
                        }
#pragma unroll
                        for (int j = 0; j < R_; ++j) acc[k][j] = fmaf(x, Q[c * R_ + j], acc[k][j]);
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < R_; ++j) {
                const float v = wave_tree((acc[0][j] + acc[2][j]) + (acc[1][j] + acc[3][j]));
                if (lane == 0) pw[i * R_ + j] = v;
            }
        }
    } else {
        const int64_t pieces = (m + PIECE - 1) / PIECE;
        const int64_t i = t / pieces, q = t % pieces;
        const int64_t c0 = q * PIECE, c1 = c0 + PIECE < m ? c0 + PIECE : m;
        float acc[R_];
#pragma unroll
        for (int j = 0; j < R_; ++j) acc[j] = 0.0f;
        for (int64_t c = c0 + threadIdx.x; c < c1; c += THREADS) {
            float x = M[i * m + c];
            if (EF) {
                const float p = ef_scale * e[i * m + c];
                x = x + p;
                e[i * m + c] = x;
            }
#pragma unroll
            for (int j = 0; j < R_; ++j) acc[j] = fmaf(x, Q[c * R_ + j], acc[j]);
        }
#pragma unroll
        for (int j = 0; j < R_; ++j) lds[j][threadIdx.x] = acc[j];
        __syncthreads();
        if (threadIdx.x < 64) {
#pragma unroll
            for (int j = 0; j < R_; ++j) {
                const float v = wave_tree((lds[j][lane] + lds[j][lane + 128]) + (lds[j][lane + 64] + lds[j][lane + 192]));
                if (lane == 0) pw[(i * pieces + q) * R_ + j] = v;
            }
        }
    }
}

// one workgroup per tensor; thread t owns the rows t, t + 256, ... of Ph (in the wire) in every step
template <int R_>
__global__ __launch_bounds__(THREADS) void psgd_orth_kernel(const int64_t *__restrict__ seg_table, const int64_t *__restrict__ lay,
                                                            const float *__restrict__ pwork, uint8_t *wire, int32_t *__restrict__ flags) {
    __shared__ float lds[THREADS + 1];
    const int seg = blockIdx.x;
    const int64_t *rec = seg_table + 8 * (int64_t)seg;
    const int64_t n = rec[4], m = rec[1] / n;
    const int64_t pieces = m <= PIECE ? 1 : (m + PIECE - 1) / PIECE;
    const float *pw = pwork + lay[4 * (int64_t)seg + 1];
    uint32_t *head = reinterpret_cast<uint32_t *>(wire + rec[3]);
    float *ph = reinterpret_cast<float *>(wire + rec[3] + GQ_PSGD_HEADER_BYTES);
    if (threadIdx.x == 0) {
        head[0] = (uint32_t)n;
        head[1] = (uint32_t)m;
        head[2] = (uint32_t)R_;
        head[3] = 0u;
    }
    for (int64_t i = threadIdx.x; i < n; i += THREADS) {
#pragma unroll
        for (int j = 0; j < R_; ++j) {
            float v = pw[i * pieces * R_ + j];
            for (int64_t q = 1; q < pieces; ++q) v = v + pw[(i * pieces + q) * R_ + j];
            ph[i * R_ + j] = v;
        }
    }
#pragma unroll 1
    for (int j = 0; j < R_; ++j) {
#pragma unroll 1
        for (int k = 0; k < j; ++k) {
            float x = 0.0f;
            for (int64_t i = threadIdx.x; i < n; i += THREADS) x = fmaf(ph[i * R_ + k], ph[i * R_ + j], x);
            const float d = block_tree(x, lds);
            for (int64_t i = threadIdx.x; i < n; i += THREADS) ph[i * R_ + j] = fmaf(-d, ph[i * R_ + k], ph[i * R_ + j]);
        }
        float x = 0.0f;
        for (int64_t i = threadIdx.x; i < n; i += THREADS) x = fmaf(ph[i * R_ + j], ph[i * R_ + j], x);
        const float nrm = sqrtf(block_tree(x, lds));      // (correctly rounded: hipcc expands sqrtf that way by default; __fsqrt_rn is the bare v_sqrt_f32, 1 ulp)
        const float den = nrm + 1e-8f;
        for (int64_t i = threadIdx.x; i < n; i += THREADS) ph[i * R_ + j] = ph[i * R_ + j] / den;
        if (threadIdx.x == 0) flags[4 * seg + j] = (nrm == 0.0f || !isfinite(nrm)) ? 1 : 0;
    }
}

template <int R_, bool EF>
__global__ __launch_bounds__(THREADS) void psgd_back_kernel(const int64_t *__restrict__ seg_table, const int64_t *__restrict__ lay,
                                                            const int32_t *__restrict__ item_seg, const uint8_t *__restrict__ wire,
                                                            float *__restrict__ cpart) {
    __shared__ float phl[RB * R_];
    const int64_t item = blockIdx.x;
    const int seg = item_seg[item];
    const int64_t *rec = seg_table + 8 * (int64_t)seg;
    const int64_t n = rec[4], m = rec[1] / n, t = item - rec[2];
    const int64_t ctiles = (m + TC - 1) / TC;
    const int64_t rb = t / ctiles, ct = t % ctiles;
    const int64_t i0 = rb * RB, rows = i0 + RB < n ? RB : n - i0;
    const float *src = reinterpret_cast<const float *>(EF ? rec[7] : rec[0]);
    const float *ph = reinterpret_cast<const float *>(wire + rec[3] + GQ_PSGD_HEADER_BYTES);
    for (int64_t x = threadIdx.x; x < rows * R_; x += THREADS) phl[x] = ph[i0 * R_ + x];
    __syncthreads();
    const int64_t c = ct * TC + threadIdx.x;
    if (c >= m) return;
    float acc[R_];
#pragma unroll
    for (int j = 0; j < R_; ++j) acc[j] = 0.0f;
    for (int64_t rr = 0; rr < rows; ++rr) {
        const float x = src[(i0 + rr) * m + c];
#pragma unroll
        for (int j = 0; j < R_; ++j) acc[j] = fmaf(x, phl[rr * R_ + j], acc[j]);
    }
    float *cp = cpart + lay[4 * (int64_t)seg + 2] + (rb * m + c) * R_;
#pragma unroll
    for (int j = 0; j < R_; ++j) cp[j] = acc[j];
}

template <int R_>
__global__ __launch_bounds__(THREADS) void psgd_fold_kernel(const int64_t *__restrict__ seg_table, const int64_t *__restrict__ lay,
                                                            const int32_t *__restrict__ item_seg, const int64_t *__restrict__ state,
                                                            const float *__restrict__ cpart, const int32_t *__restrict__ flags,
                                                            uint8_t *__restrict__ wire, uint64_t seed) {
    const int64_t item = blockIdx.x;
    const int seg = item_seg[item];
    const int64_t *rec = seg_table + 8 * (int64_t)seg;
    const int64_t n = rec[4], m = rec[1] / n, t = item - rec[2];
    const int64_t ctiles = (m + TC - 1) / TC;
    if (t >= ctiles) return;      // (row block 0's tiles fold; the others have nothing to do)
    const int64_t nb = (n + RB - 1) / RB;
    uint32_t *sec = reinterpret_cast<uint32_t *>(wire + rec[3]);
    if (t == 0) {
        const int64_t words = 4 + (int64_t)R_ * (n + m), pad = GQ_PSGD_SECTION_BYTES(n, m, R_) / 4 - words;      // 0 ... 3
        if (threadIdx.x < pad) sec[words + threadIdx.x] = 0u;
    }
    const int64_t c = t * TC + threadIdx.x;
    if (c >= m) return;
    const float *cp = cpart + lay[4 * (int64_t)seg + 2];
    float *qw = reinterpret_cast<float *>(sec + 4 + n * R_);
    float *Q = reinterpret_cast<float *>(state[2 * (int64_t)seg]);
    const uint64_t key = (uint64_t)(lay[4 * (int64_t)seg + 3] | state[2 * (int64_t)seg + 1]) << 32;
#pragma unroll
    for (int j = 0; j < R_; ++j) {
        float v = cp[c * R_ + j];
        for (int64_t b = 1; b < nb; ++b) v = v + cp[(b * m + c) * R_ + j];
        qw[c * R_ + j] = v;
        const float u = gq::uniform01(seed, key | (uint64_t)(c * R_ + j));
        Q[c * R_ + j] = flags[4 * seg + j] ? 2.0f * u - 1.0f : v;
    }
}

// RESID: launch (D) -- one payload, the wire just written; e = M' - D where e is given (it holds M'), D into out where given.
// Otherwise the decode-mean of R payloads.
template <int R_, bool RESID>
__global__ __launch_bounds__(THREADS) void psgd_decode_kernel(const int64_t *__restrict__ seg_table, const int32_t *__restrict__ item_seg,
                                                              const uint8_t *__restrict__ gathered, int64_t stride, int R,
                                                              float *__restrict__ out, int with_err) {
    const int64_t item = blockIdx.x;
    const int seg = item_seg[item];
    const int64_t *rec = seg_table + 8 * (int64_t)seg;
    const int64_t n = rec[4], m = rec[1] / n, t = item - rec[2];
    const int64_t ctiles = (m + TC - 1) / TC;
    const int64_t rb = t / ctiles, ct = t % ctiles;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t i0 = rb * RB + 16 * wv, cb = ct * TC + 4 * lane;
    float acc[16][4];
#pragma unroll
    for (int rr = 0; rr < 16; ++rr)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[rr][k] = 0.0f;
    for (int rho = 0; rho < R; ++rho) {
        const float *ph = reinterpret_cast<const float *>(gathered + (int64_t)rho * stride + rec[3] + GQ_PSGD_HEADER_BYTES);
        const float *q = ph + n * R_;
        float qv[4][R_];
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int j = 0; j < R_; ++j) qv[k][j] = cb + k < m ? q[(cb + k) * R_ + j] : 0.0f;
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            const int64_t i = i0 + rr;
            if (i < n) {
                float pv[R_];
#pragma unroll
                for (int j = 0; j < R_; ++j) pv[j] = ph[i * R_ + j];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float d = pv[0] * qv[k][0];
#pragma unroll
                    for (int j = 1; j < R_; ++j) d = fmaf(pv[j], qv[k][j], d);
                    acc[rr][k] = rho == 0 ? d : acc[rr][k] + d;
                }
            }
        }
    }
    if (cb >= m) return;
    const float fR = (float)R;
    float *o = out ? out + rec[5] : nullptr;
    float *e = (RESID && with_err) ? reinterpret_cast<float *>(rec[7]) : nullptr;
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) {
        const int64_t i = i0 + rr;
        if (i >= n) break;
        const int64_t at = i * m + cb;
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = RESID ? acc[rr][k] : acc[rr][k] / fR;
        if (e) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (cb + k < m) e[at + k] = e[at + k] - v[k];
        }
        if (o) {
            if (cb + 3 < m && aligned16(o + at)) {
                *reinterpret_cast<float4 *>(o + at) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (cb + k < m) o[at + k] = v[k];
            }
        }
    }
}

static int check_batch(const gq_psgd_batch *b, const char *what, bool compress) {
    if (!b || b->struct_bytes != sizeof(gq_psgd_batch)) return fail(GQ_ERR_INVALID_ARG, "%s: descriptor missing or of another size", what);
    if (b->nseg < 1 || b->nitems < 1 || b->nitems > 0x7fffffff || b->ndense < 0)
        return fail(GQ_ERR_INVALID_ARG, "%s: bad sizes (nseg %d, tiles %lld, ndense %d)", what, b->nseg, (long long)b->nitems, b->ndense);
    if (b->rank != 1 && b->rank != 2 && b->rank != 4) return fail(GQ_ERR_INVALID_ARG, "%s: rank %d (1, 2 or 4)", what, b->rank);
    if (!b->seg_table || !b->item_seg) return fail(GQ_ERR_INVALID_ARG, "%s: null table", what);
    if (compress) {
        if (b->naitems < 1 || b->naitems > 0x7fffffff) return fail(GQ_ERR_INVALID_ARG, "%s: %lld items", what, (long long)b->naitems);
        if (!b->lay || !b->aitem_seg || !b->state || !b->pwork || !b->cpart || !b->flags || (b->ndense > 0 && !b->dense_table))
            return fail(GQ_ERR_INVALID_ARG, "%s: null table or scratch buffer (a record needs the state table of its user)", what);
    }
    return GQ_OK;
}

template <int R_, bool EF>
static int compress(const gq_psgd_batch *b, uint8_t *wire, float ef_scale, float *out, hipStream_t st) {
    const dim3 items((unsigned)b->naitems), tiles((unsigned)b->nitems), segs((unsigned)b->nseg), block(THREADS);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(psgd_project_kernel<R_, EF>), items, block, 0, st, b->seg_table, b->lay, b->aitem_seg, b->state,
                       b->pwork, wire, ef_scale, b->dense_table, b->ndense);
    GQL_CHECK_LAUNCH("gq_psgd_compress_batched (project)");
    hipLaunchKernelGGL(HIP_KERNEL_NAME(psgd_orth_kernel<R_>), segs, block, 0, st, b->seg_table, b->lay, b->pwork, wire, b->flags);
    GQL_CHECK_LAUNCH("gq_psgd_compress_batched (orthogonalise)");
    hipLaunchKernelGGL(HIP_KERNEL_NAME(psgd_back_kernel<R_, EF>), tiles, block, 0, st, b->seg_table, b->lay, b->item_seg, wire, b->cpart);
    GQL_CHECK_LAUNCH("gq_psgd_compress_batched (back-project)");
    hipLaunchKernelGGL(HIP_KERNEL_NAME(psgd_fold_kernel<R_>), tiles, block, 0, st, b->seg_table, b->lay, b->item_seg, b->state, b->cpart,
                       b->flags, wire, b->seed);
    GQL_CHECK_LAUNCH("gq_psgd_compress_batched (fold)");
    if (EF || out) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(psgd_decode_kernel<R_, true>), tiles, block, 0, st, b->seg_table, b->item_seg, wire, (int64_t)0, 1,
                           out, EF ? 1 : 0);
        GQL_CHECK_LAUNCH("gq_psgd_compress_batched (residual)");
    }
    return GQ_OK;
}

template <int R_>
static int decode(const gq_psgd_batch *b, const uint8_t *gathered, int64_t stride, int R, float *out, hipStream_t st) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(psgd_decode_kernel<R_, false>), dim3((unsigned)b->nitems), dim3(THREADS), 0, st, b->seg_table,
                       b->item_seg, gathered, stride, R, out, 0);
    GQL_CHECK_LAUNCH("gq_psgd_decode_sum_batched");
    return GQ_OK;
}

}  // namespace gqp

GQP_API int gq_psgd_abi_version(void) { return GQ_PSGD_ABI_VERSION; }

GQP_API const char *gq_psgd_last_error(void) { return gqp::err_buf; }

GQP_API int gq_psgd_compress_batched(const gq_psgd_batch *b, uint8_t *wire, float ef_scale, float *out, void *stream) {
    using namespace gqp;
    const int rc = check_batch(b, "gq_psgd_compress_batched", true);
    if (rc != GQ_OK) return rc;
    if (!wire || (reinterpret_cast<uintptr_t>(wire) & 3) != 0)
        return fail(GQ_ERR_INVALID_ARG, "gq_psgd_compress_batched: the wire must be a 4-byte aligned device address");
    if (out && (reinterpret_cast<uintptr_t>(out) & 3) != 0) return fail(GQ_ERR_INVALID_ARG, "gq_psgd_compress_batched: out must be 4-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const bool ef = !isnan(ef_scale);
    switch (b->rank * 2 + (ef ? 1 : 0)) {
    case 2: return compress<1, false>(b, wire, 0.0f, out, st);
    case 3: return compress<1, true>(b, wire, ef_scale, out, st);
    case 4: return compress<2, false>(b, wire, 0.0f, out, st);
    case 5: return compress<2, true>(b, wire, ef_scale, out, st);
    case 8: return compress<4, false>(b, wire, 0.0f, out, st);
    default: return compress<4, true>(b, wire, ef_scale, out, st);
    }
}

GQP_API int gq_psgd_decode_sum_batched(const gq_psgd_batch *b, const uint8_t *gathered, int64_t user_stride_bytes, int R, float *out,
                                       int plain, void *stream) {
    using namespace gqp;
    (void)plain;
    const int rc = check_batch(b, "gq_psgd_decode_sum_batched", false);
    if (rc != GQ_OK) return rc;
    if (!gathered || !out) return fail(GQ_ERR_INVALID_ARG, "gq_psgd_decode_sum_batched: null pointer");
    if (R < 1 || (R > 1 && (user_stride_bytes < 0 || (user_stride_bytes & 3) != 0)))
        return fail(GQ_ERR_INVALID_ARG, "gq_psgd_decode_sum_batched: R = %d, user stride %lld", R, (long long)user_stride_bytes);
    if ((reinterpret_cast<uintptr_t>(gathered) & 3) != 0 || (reinterpret_cast<uintptr_t>(out) & 3) != 0)
        return fail(GQ_ERR_INVALID_ARG, "gq_psgd_decode_sum_batched: the gathered wire and out must be 4-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (b->rank == 1) return decode<1>(b, gathered, user_stride_bytes, R, out, st);
    if (b->rank == 2) return decode<2>(b, gathered, user_stride_bytes, R, out, st);
    return decode<4>(b, gathered, user_stride_bytes, R, out, st);
}
