// Low-rank gradient compression at rank 16 and 32 on the matrix cores -- libgq_psgd.so beside csrc/psgd.hip (include/gq_psgd.h,
// RANKS 16 AND 32).  The same five launches and the decode, the same tables, wire and scratch names:
//   (A) project      a workgroup per item = 64 rows x one piece of GQ_PSGD_WIDE_PIECE columns.  M' comes in as whole 256-byte row
//                    pieces, 64 columns at a time, through LDS into the A operand of the f32 MFMA whose 32 (16) columns are the
//                    rank; the matching 64 rows of Q are the B operand, in LDS too.  Partial P -> pwork.  The next chunk's loads
//                    are in flight while this one multiplies.  Every workgroup copies a slice of the identity tensors.
//   (B) orthogonalise a workgroup of 16 waves per tensor, no serial sweep: folds the pieces into P (in the wire's Ph region) and
//                    forms the Gram matrix G = P^T P in float64 (v_mfma_f64_16x16x4_f64) in ONE pass; wave 0 factors G = L L^T with
//                    a lane per row, L's row in registers, and inverts L; a second pass writes Ph = P L^-T, float64 MFMA again.
//   (C) back-project a workgroup per tile of 64 rows x 256 columns, a wave 64 columns: 32 (16) consecutive columns of a row of M'
//                    ARE the A operand of M'^T, straight from global; the block's Ph rows are the B operand, from LDS -> cpart.
//   (C') fold        every tile's workgroup folds a share of its column tile's Q' values over the row blocks, in block order.
//   (D) / decode     a tile of `out` is one contraction over k = R * r, payload after payload through LDS (a payload's 64 x r of
//                    Ph and 256 x r of Q'), v_mfma_f32_32x32x2_f32 at both ranks with Q' as the A side: a lane then holds four
//                    neighbouring columns of one row, one 16-byte store.
// No atomics, no data-dependent launch argument; the order of additions is fixed by this file.
#include <math.h>

#include "gq_common.hpp"
#include "gq_lib_prelude.hpp"
#include "gq_psgd.h"
#include "psgd_wide.hpp"

namespace gqpw {

constexpr int THREADS = 256;
constexpr int ORTH_THREADS = 1024;
constexpr int WP = GQ_PSGD_WIDE_PIECE;
constexpr int RB = GQ_PSGD_ROW_BLOCK;
constexpr int TC = GQ_PSGD_TILE_COLS;
constexpr int CH = 64;      // columns of M per pass of (A) through LDS: a 256-byte piece of each of the 64 rows
static_assert(THREADS == 256 && RB == 64 && TC == 256 && WP % CH == 0, "four waves a workgroup; a tile is 64 rows x 4 waves x 64 columns");

using gql::aligned16;

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

// The f32 MFMA whose N side is the rank.  Operands: lane l gives A[l % MN][l / MN] and B[l / MN][l % MN]; register v of lane l
// holds D[drow(l, v)][l % MN].
template <int R_>
struct Tile;
template <>
struct Tile<32> {
    typedef f32x16 acc_t;
    static constexpr int MN = 32, K = 2, NV = 16;
    static __device__ __forceinline__ acc_t mma(float a, float b, acc_t c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ int drow(int lane, int v) { return 8 * (v >> 2) + 4 * (lane >> 5) + (v & 3); }
};
template <>
struct Tile<16> {
    typedef f32x4 acc_t;
    static constexpr int MN = 16, K = 4, NV = 4;
    static __device__ __forceinline__ acc_t mma(float a, float b, acc_t c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ int drow(int lane, int v) { return 4 * (lane >> 4) + v; }
};

// v_mfma_f64_16x16x4_f64: lane l gives A[l % 16][l / 16] and B[l / 16][l % 16]; register v of lane l holds D[4 * v + l / 16][l % 16]
__device__ __forceinline__ f64x4 mma64(double a, double b, f64x4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// x of lane `lane` (wave-uniform) to every lane
__device__ __forceinline__ double lane_value(double x, int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), lane), hi = __builtin_amdgcn_readlane(__double2hiint(x), lane);
    return __hiloint2double(hi, lo);
}

template <int R_, bool EF>
__global__ __launch_bounds__(THREADS) void wide_project_kernel(const int64_t *__restrict__ seg_table, const int64_t *__restrict__ lay,
                                                               const int32_t *__restrict__ aitem_seg, const int64_t *__restrict__ state,
                                                               float *__restrict__ pwork, uint8_t *__restrict__ wire, float ef_scale,
                                                               const int64_t *__restrict__ dense_table, int ndense) {
    typedef Tile<R_> T;
    constexpr int MN = T::MN, K = T::K;
    constexpr int LD = CH + K;               // the A operand's reads (rows l % MN, columns k + l / MN) fall on 64 different banks
    constexpr int WR = RB / MN, WK = 4 / WR; // waves down the rows and across a chunk's columns: 2 x 2 at rank 32, 4 x 1 at 16
    constexpr int KSPAN = CH / WK;
    __shared__ float Ms[RB * LD];
    __shared__ float Qs[CH * R_];
    // the identity tensors, a slice of each per workgroup
    for (int d = 0; d < ndense; ++d) {
        const float *src = reinterpret_cast<const float *>(dense_table[3 * d]);
        float *dst = reinterpret_cast<float *>(wire + dense_table[3 * d + 1]);
        const int64_t cnt = dense_table[3 * d + 2];
        for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < cnt; i += (int64_t)gridDim.x * THREADS) dst[i] = src[i];
    }
    const int64_t item = blockIdx.x;
    const int seg = aitem_seg[item];
    const int64_t *rec = seg_table + 8 * (int64_t)seg;
    const int64_t *L = lay + 4 * (int64_t)seg;
    const int64_t n = rec[4], m = rec[1] / n, t = item - L[0];
    const int64_t pieces = (m + WP - 1) / WP;
    const int64_t rb = t / pieces, q = t % pieces;
    const int64_t i0 = rb * RB, c0 = q * WP, c1 = c0 + WP < m ? c0 + WP : m;
    const float *M = reinterpret_cast<const float *>(rec[0]);
    float *e = EF ? reinterpret_cast<float *>(rec[7]) : nullptr;
    const float *Q = reinterpret_cast<const float *>(state[2 * (int64_t)seg]);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int lr = threadIdx.x >> 4, lc = (threadIdx.x & 15) * 4;      // this thread loads rows lr + 16 a, columns lc ... lc + 3 of a chunk
    const bool vec = (m & 3) == 0 && aligned16(M) && (!EF || aligned16(e));
    float x[4][4];
    auto load = [&](int64_t cc) {
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int64_t i = i0 + lr + 16 * a, c = cc + lc, at = i * m + c;
            if (i < n && vec && c < c1) {      // (m and c are multiples of 4 and so is every piece's end: the four are inside)
                const float4 g = *reinterpret_cast<const float4 *>(M + at);
                x[a][0] = g.x, x[a][1] = g.y, x[a][2] = g.z, x[a][3] = g.w;
                if (EF) {
                    const float4 r = *reinterpret_cast<const float4 *>(e + at);
                    const float p0 = ef_scale * r.x, p1 = ef_scale * r.y, p2 = ef_scale * r.z, p3 = ef_scale * r.w;
                    x[a][0] = x[a][0] + p0, x[a][1] = x[a][1] + p1, x[a][2] = x[a][2] + p2, x[a][3] = x[a][3] + p3;
                    *reinterpret_cast<float4 *>(e + at) = make_float4(x[a][0], x[a][1], x[a][2], x[a][3]);
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float v = 0.0f;
                    if (i < n && c + k < c1) {
                        v = M[at + k];
                        if (EF) {
                            const float p = ef_scale * e[at + k];
                            v = v + p;
                            e[at + k] = v;
                        }
                    }
                    x[a][k] = v;
                }
            }
        }
    };
    typename T::acc_t acc = {};
    const int h = wv % WR, kh = wv / WR;
    load(c0);
    for (int64_t cc = c0; cc < c1; cc += CH) {
        __syncthreads();      // the chunk before has been multiplied
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int k = 0; k < 4; ++k) Ms[(lr + 16 * a) * LD + lc + k] = x[a][k];
        for (int y = threadIdx.x; y < CH * R_; y += THREADS) Qs[y] = cc + y / R_ < c1 ? Q[cc * R_ + y] : 0.0f;
        __syncthreads();
        if (cc + CH < c1) load(cc + CH);
#pragma unroll
        for (int s = 0; s < KSPAN / K; ++s) {
            const int k = kh * KSPAN + s * K + lane / MN;
            acc = T::mma(Ms[(MN * h + lane % MN) * LD + k], Qs[k * R_ + lane % MN], acc);
        }
    }
    if (WK == 2) {      // the two column halves of the chunks, the lower one first
        __syncthreads();
        if (kh == 1)
#pragma unroll
            for (int v = 0; v < T::NV; ++v) Ms[(MN * h + T::drow(lane, v)) * LD + lane % MN] = acc[v];
        __syncthreads();
        if (kh == 0)
#pragma unroll
            for (int v = 0; v < T::NV; ++v) acc[v] = acc[v] + Ms[(MN * h + T::drow(lane, v)) * LD + lane % MN];
    }
    if (kh == 0) {
        float *pw = pwork + L[1];
#pragma unroll
        for (int v = 0; v < T::NV; ++v) {
            const int64_t i = i0 + MN * h + T::drow(lane, v);
            if (i < n) pw[(i * pieces + q) * R_ + lane % MN] = acc[v];
        }
    }
}

// one workgroup of 16 waves per tensor
template <int R_>
__global__ __launch_bounds__(ORTH_THREADS) void wide_orth_kernel(const int64_t *__restrict__ seg_table, const int64_t *__restrict__ lay,
                                                                 const float *__restrict__ pwork, uint8_t *wire, int32_t *__restrict__ flags) {
    constexpr int NT = R_ / 16, WAVES = ORTH_THREADS / 64;
    __shared__ double Gs[R_ * R_];      // G, then W = L^-T with the reset columns zero
    __shared__ double Ls[R_ * R_];
    __shared__ double scale_s[R_];
    __shared__ int bad_s[R_];
    const int seg = blockIdx.x;
    const int64_t *rec = seg_table + 8 * (int64_t)seg;
    const int64_t n = rec[4], m = rec[1] / n;
    const int64_t pieces = (m + WP - 1) / WP;
    const float *pw = pwork + lay[4 * (int64_t)seg + 1];
    uint32_t *head = reinterpret_cast<uint32_t *>(wire + rec[3]);
    float *ph = reinterpret_cast<float *>(wire + rec[3] + GQ_PSGD_HEADER_BYTES);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (threadIdx.x == 0) {
        head[0] = (uint32_t)n;
        head[1] = (uint32_t)m;
        head[2] = (uint32_t)R_;
        head[3] = 0u;
    }
    for (int y = threadIdx.x; y < R_ * R_; y += ORTH_THREADS) Gs[y] = 0.0;
    // pass 1: a wave folds four rows of P at a time, a lane the value it gives the MFMA as A and as B
    f64x4 g[NT][NT] = {};
    for (int64_t i4 = 4 * wv; i4 < n; i4 += 4 * WAVES) {
        const int64_t i = i4 + (lane >> 4);
        double a[NT];
#pragma unroll
        for (int ta = 0; ta < NT; ++ta) {
            const int j = 16 * ta + (lane & 15);
            float v = 0.0f;
            if (i < n) {
                v = pw[i * pieces * R_ + j];
                for (int64_t p = 1; p < pieces; ++p) v = v + pw[(i * pieces + p) * R_ + j];
                ph[i * R_ + j] = v;
            }
            a[ta] = (double)v;
        }
#pragma unroll
        for (int ta = 0; ta < NT; ++ta)
#pragma unroll
            for (int tb = 0; tb < NT; ++tb) g[ta][tb] = mma64(a[ta], a[tb], g[ta][tb]);
    }
    __syncthreads();
    for (int w = 0; w < WAVES; ++w) {      // the waves' sums in wave order
        if (wv == w) {
#pragma unroll
            for (int ta = 0; ta < NT; ++ta)
#pragma unroll
                for (int tb = 0; tb < NT; ++tb)
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        double *at = &Gs[(16 * ta + 4 * v + (lane >> 4)) * R_ + 16 * tb + (lane & 15)];
                        *at = *at + g[ta][tb][v];
                    }
        }
        __syncthreads();
    }
    // Cholesky, lane t with row t of G in registers: column j's pivot is nrm[j].  A column resets where its pivot's square is not
    // above 2^-40 of the column's own square (the float64 rounding dust of a dependent column, or exactly nothing) or is not
    // finite: L's column and W's column are zero then.  The elimination divides by the pivot itself, so that what is taken out of
    // the later columns is the whole of their part along column j; the contract's nrm[j] + 1e-8f scales column j of W.
    if (wv == 0) {
        const int t = lane & (R_ - 1);
        double gr[R_];
#pragma unroll
        for (int c = 0; c < R_; ++c) gr[c] = Gs[t * R_ + c];
        const double g0 = Gs[t * R_ + t];
#pragma unroll
        for (int j = 0; j < R_; ++j) {
            const double d = lane_value(gr[j], j), d0 = lane_value(g0, j);
            const double piv = d > d0 * 0x1p-40 ? sqrt(d) : 0.0;
            const float nrm = (float)piv;
            const bool bad = !(nrm > 0.0f) || !(nrm < INFINITY);
            const double lt = bad ? 0.0 : gr[j] / piv;      // L[t][j] where t > j
            if (lane < R_) Ls[t * R_ + j] = t > j ? lt : (t == j ? (bad ? 1.0 : piv) : 0.0);
            if (lane == 0) {
                scale_s[j] = bad ? 0.0 : piv / (double)(nrm + 1e-8f);
                bad_s[j] = bad ? 1 : 0;
                flags[R_ * seg + j] = bad ? 1 : 0;
            }
#pragma unroll
            for (int c = j + 1; c < R_; ++c) gr[c] = fma(-lt, lane_value(lt, c), gr[c]);
        }
    }
    __syncthreads();
    // X = L^-1 by forward substitution, lane t its column t; W[t][i] = X[i][t] * nrm[i] / (nrm[i] + 1e-8f)
    if (wv == 0) {
        const int t = lane & (R_ - 1);
        double xs[R_];
#pragma unroll
        for (int i = 0; i < R_; ++i) {
            double s = i == t ? 1.0 : 0.0;
#pragma unroll
            for (int k = 0; k < i; ++k) s = fma(-Ls[i * R_ + k], xs[k], s);
            xs[i] = s / Ls[i * R_ + i];
        }
        if (lane < R_)
#pragma unroll
            for (int i = 0; i < R_; ++i) Gs[t * R_ + i] = bad_s[i] ? 0.0 : xs[i] * scale_s[i];
    }
    __syncthreads();
    // pass 2: Ph = P W, a wave 16 rows at a time, in place (a wave reads all of its rows before it writes them).  The MFMA's k index
    // l / 16 of step s stands for P's column 16 gk + 4 * (l / 16) + s on both sides, so a lane reads four neighbouring values.
    for (int64_t r0 = 16 * wv; r0 < n; r0 += 16 * WAVES) {
        f64x4 d[NT] = {};
        const int64_t i = r0 + (lane & 15);
#pragma unroll
        for (int gk = 0; gk < NT; ++gk) {
            float p[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) p[s] = i < n ? ph[i * R_ + 16 * gk + 4 * (lane >> 4) + s] : 0.0f;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int kk = 16 * gk + 4 * (lane >> 4) + s;
#pragma unroll
                for (int tj = 0; tj < NT; ++tj) d[tj] = mma64((double)p[s], Gs[kk * R_ + 16 * tj + (lane & 15)], d[tj]);
            }
        }
#pragma unroll
        for (int tj = 0; tj < NT; ++tj)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int64_t row = r0 + 4 * v + (lane >> 4);
                const int j = 16 * tj + (lane & 15);
                if (row < n) ph[row * R_ + j] = bad_s[j] ? 0.0f : (float)d[tj][v];
            }
    }
}

template <int R_, bool EF>
__global__ __launch_bounds__(THREADS) void wide_back_kernel(const int64_t *__restrict__ seg_table, const int64_t *__restrict__ lay,
                                                            const int32_t *__restrict__ item_seg, const uint8_t *__restrict__ wire,
                                                            float *__restrict__ cpart) {
    typedef Tile<R_> T;
    constexpr int MN = T::MN, K = T::K, CT = 64 / MN;      // a wave's 64 columns as CT tiles of the MFMA's M side
    __shared__ float phl[RB * R_];
    const int64_t item = blockIdx.x;
    const int seg = item_seg[item];
    const int64_t *rec = seg_table + 8 * (int64_t)seg;
    const int64_t n = rec[4], m = rec[1] / n, t = item - rec[2];
    const int64_t ctiles = (m + TC - 1) / TC;
    const int64_t rb = t / ctiles, ct = t % ctiles;
    const int64_t i0 = rb * RB;
    const int rows = (int)(i0 + RB < n ? RB : n - i0);
    const float *src = reinterpret_cast<const float *>(EF ? rec[7] : rec[0]);
    const float *ph = reinterpret_cast<const float *>(wire + rec[3] + GQ_PSGD_HEADER_BYTES);
    for (int y = threadIdx.x; y < RB * R_; y += THREADS) phl[y] = y < rows * R_ ? ph[i0 * R_ + y] : 0.0f;
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t cw = ct * TC + 64 * wv;
    if (cw >= m) return;
    const int cl = lane % MN, kl = lane / MN;
    typename T::acc_t acc[CT] = {};
#pragma unroll 4
    for (int k0 = 0; k0 < RB; k0 += K) {
        const int rr = k0 + kl;
        const float b = phl[rr * R_ + cl];
#pragma unroll
        for (int u = 0; u < CT; ++u) {
            const int64_t c = cw + MN * u + cl;
            const float a = (rr < rows && c < m) ? src[(i0 + rr) * m + c] : 0.0f;
            acc[u] = T::mma(a, b, acc[u]);
        }
    }
    float *cp = cpart + lay[4 * (int64_t)seg + 2] + rb * m * R_;
#pragma unroll
    for (int u = 0; u < CT; ++u)
#pragma unroll
        for (int v = 0; v < T::NV; ++v) {
            const int64_t c = cw + MN * u + T::drow(lane, v);
            if (c < m) cp[c * R_ + cl] = acc[u][v];
        }
}

// the workgroup of tile (rb, ct) folds share rb of column tile ct's values of Q'
template <int R_>
__global__ __launch_bounds__(THREADS) void wide_fold_kernel(const int64_t *__restrict__ seg_table, const int64_t *__restrict__ lay,
                                                            const int32_t *__restrict__ item_seg, const int64_t *__restrict__ state,
                                                            const float *__restrict__ cpart, const int32_t *__restrict__ flags,
                                                            uint8_t *__restrict__ wire, uint64_t seed) {
    const int64_t item = blockIdx.x;
    const int seg = item_seg[item];
    const int64_t *rec = seg_table + 8 * (int64_t)seg;
    const int64_t n = rec[4], m = rec[1] / n, t = item - rec[2];
    const int64_t ctiles = (m + TC - 1) / TC, nb = (n + RB - 1) / RB;
    const int64_t rb = t / ctiles, ct = t % ctiles;
    uint32_t *sec = reinterpret_cast<uint32_t *>(wire + rec[3]);
    if (t == 0) {
        const int64_t words = 4 + (int64_t)R_ * (n + m), pad = GQ_PSGD_SECTION_BYTES(n, m, R_) / 4 - words;      // 0 ... 3
        if (threadIdx.x < pad) sec[words + threadIdx.x] = 0u;
    }
    const int64_t total = (ct * TC + TC < m ? TC : m - ct * TC) * R_;
    const int64_t share = (total + nb - 1) / nb;
    const int64_t lo = rb * share, hi = lo + share < total ? lo + share : total;
    const float *cp = cpart + lay[4 * (int64_t)seg + 2];
    float *qw = reinterpret_cast<float *>(sec + 4 + n * R_);
    float *Q = reinterpret_cast<float *>(state[2 * (int64_t)seg]);
    const uint64_t key = (uint64_t)(lay[4 * (int64_t)seg + 3] | state[2 * (int64_t)seg + 1]) << 32;
    for (int64_t y = lo + threadIdx.x; y < hi; y += THREADS) {
        const int64_t at = ct * TC * R_ + y;      // c * r + j
        float v = cp[at];
        for (int64_t b = 1; b < nb; ++b) v = v + cp[b * m * R_ + at];
        qw[at] = v;
        const float u = gq::uniform01(seed, key | (uint64_t)at);
        Q[at] = flags[R_ * seg + (int)(at % R_)] ? 2.0f * u - 1.0f : v;
    }
}

// RESID: launch (D) -- one payload, the wire just written; e = M' - D where e is given (it holds M'), D into out where given.
// Otherwise the decode-mean of R payloads.
template <int R_, bool RESID>
__global__ __launch_bounds__(THREADS) void wide_decode_kernel(const int64_t *__restrict__ seg_table, const int32_t *__restrict__ item_seg,
                                                              const uint8_t *__restrict__ gathered, int64_t stride, int R,
                                                              float *__restrict__ out, int with_err) {
    constexpr int LD = R_ + 1;      // rows l % 32 of a factor slice on different banks
    __shared__ float Ps[RB * LD];
    __shared__ float Qs[TC * LD];
    const int64_t item = blockIdx.x;
    const int seg = item_seg[item];
    const int64_t *rec = seg_table + 8 * (int64_t)seg;
    const int64_t n = rec[4], m = rec[1] / n, t = item - rec[2];
    const int64_t ctiles = (m + TC - 1) / TC;
    const int64_t rb = t / ctiles, ct = t % ctiles;
    const int64_t i0 = rb * RB, c0 = ct * TC;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    f32x16 acc[2][2] = {};      // [column half of the wave's 64][row half of the 64]
    for (int rho = 0; rho < R; ++rho) {
        const float *ph = reinterpret_cast<const float *>(gathered + (int64_t)rho * stride + rec[3] + GQ_PSGD_HEADER_BYTES);
        const float *q = ph + n * R_;
        __syncthreads();      // the payload before has been multiplied
        for (int y = threadIdx.x; y < RB * R_; y += THREADS) Ps[(y / R_) * LD + y % R_] = i0 + y / R_ < n ? ph[i0 * R_ + y] : 0.0f;
        for (int y = threadIdx.x; y < TC * R_; y += THREADS) Qs[(y / R_) * LD + y % R_] = c0 + y / R_ < m ? q[c0 * R_ + y] : 0.0f;
        __syncthreads();
#pragma unroll 4
        for (int k0 = 0; k0 < R_; k0 += 2) {
            const int k = k0 + (lane >> 5);
            const float a0 = Qs[(64 * wv + (lane & 31)) * LD + k], a1 = Qs[(64 * wv + 32 + (lane & 31)) * LD + k];
            const float b0 = Ps[(lane & 31) * LD + k], b1 = Ps[(32 + (lane & 31)) * LD + k];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
    const float fR = (float)R;
    float *o = out ? out + rec[5] : nullptr;
    float *e = (RESID && with_err) ? reinterpret_cast<float *>(rec[7]) : nullptr;
#pragma unroll
    for (int rh = 0; rh < 2; ++rh) {
        const int64_t i = i0 + 32 * rh + (lane & 31);
        if (i >= n) continue;
#pragma unroll
        for (int ch = 0; ch < 2; ++ch)
#pragma unroll
            for (int g = 0; g < 4; ++g) {      // registers 4 g ... 4 g + 3: four neighbouring columns
                const int64_t cb = c0 + 64 * wv + 32 * ch + 8 * g + 4 * (lane >> 5);
                if (cb >= m) continue;
                const int64_t at = i * m + cb;
                float v[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = RESID ? acc[ch][rh][4 * g + k] : acc[ch][rh][4 * g + k] / fR;
                if (e) {
                    if (cb + 3 < m && aligned16(e + at)) {
                        const float4 x = *reinterpret_cast<const float4 *>(e + at);
                        *reinterpret_cast<float4 *>(e + at) = make_float4(x.x - v[0], x.y - v[1], x.z - v[2], x.w - v[3]);
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (cb + k < m) e[at + k] = e[at + k] - v[k];
                    }
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
}

#define GQPW_LAUNCHED(name)            \
    do {                               \
        hipError_t e__ = hipGetLastError(); \
        if (e__ != hipSuccess) {       \
            *what = name;              \
            return e__;                \
        }                              \
    } while (0)

template <int R_, bool EF>
static hipError_t compress(const gq_psgd_batch *b, uint8_t *wire, float ef_scale, float *out, hipStream_t st, const char **what) {
    const dim3 items((unsigned)b->naitems), tiles((unsigned)b->nitems), segs((unsigned)b->nseg), block(THREADS);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(wide_project_kernel<R_, EF>), items, block, 0, st, b->seg_table, b->lay, b->aitem_seg, b->state,
                       b->pwork, wire, ef_scale, b->dense_table, b->ndense);
    GQPW_LAUNCHED("project");
    hipLaunchKernelGGL(HIP_KERNEL_NAME(wide_orth_kernel<R_>), segs, dim3(ORTH_THREADS), 0, st, b->seg_table, b->lay, b->pwork, wire, b->flags);
    GQPW_LAUNCHED("orthogonalise");
    hipLaunchKernelGGL(HIP_KERNEL_NAME(wide_back_kernel<R_, EF>), tiles, block, 0, st, b->seg_table, b->lay, b->item_seg, wire, b->cpart);
    GQPW_LAUNCHED("back-project");
    hipLaunchKernelGGL(HIP_KERNEL_NAME(wide_fold_kernel<R_>), tiles, block, 0, st, b->seg_table, b->lay, b->item_seg, b->state, b->cpart,
                       b->flags, wire, b->seed);
    GQPW_LAUNCHED("fold");
    if (EF || out) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(wide_decode_kernel<R_, true>), tiles, block, 0, st, b->seg_table, b->item_seg, wire, (int64_t)0, 1,
                           out, EF ? 1 : 0);
        GQPW_LAUNCHED("residual");
    }
    return hipSuccess;
}

template <int R_>
static hipError_t decode(const gq_psgd_batch *b, const uint8_t *gathered, int64_t stride, int R, float *out, hipStream_t st) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(wide_decode_kernel<R_, false>), dim3((unsigned)b->nitems), dim3(THREADS), 0, st, b->seg_table,
                       b->item_seg, gathered, stride, R, out, 0);
    return hipGetLastError();
}

}  // namespace gqpw

hipError_t gq_psgd_wide_compress(const gq_psgd_batch *b, uint8_t *wire, bool ef, float ef_scale, float *out, hipStream_t st,
                                 const char **what) {
    using namespace gqpw;
    if (b->rank == 16) return ef ? compress<16, true>(b, wire, ef_scale, out, st, what) : compress<16, false>(b, wire, 0.0f, out, st, what);
    return ef ? compress<32, true>(b, wire, ef_scale, out, st, what) : compress<32, false>(b, wire, 0.0f, out, st, what);
}

hipError_t gq_psgd_wide_decode(const gq_psgd_batch *b, const uint8_t *gathered, int64_t stride, int R, float *out, hipStream_t st) {
    using namespace gqpw;
    return b->rank == 16 ? decode<16>(b, gathered, stride, R, out, st) : decode<32>(b, gathered, stride, R, out, st);
}
