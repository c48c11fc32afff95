// The one-sweep + lane-local-walk encode of a 64-subvector tile of the ProbabilisticVectorCompressor, as device code that
// both translation units include: pvq.hip (gq_pvq_encode, one tensor per launch; libgq_hsq.so) and pvq_batched.hip
// (gq_pvq_encode_batched, every tensor of a model per launch; libgq_pvq.so).  One body, so the two give the same bits.
// The scheme is described where it was written: pvq.hip, in front of pvq_encode_walk_kernel.
#pragma once
#include "hsq_encode_common.hpp"

namespace gq {

typedef float pv_f32x2 __attribute__((ext_vector_type(2)));

// The double T with  (float)x >= thr  <=>  x >= T  for every double x (round to nearest even): the midpoint between
// thr and the float below it when the tie goes to thr (even mantissa), the next double above the midpoint otherwise.
__device__ __forceinline__ double rounds_up_to_threshold(float thr) {
    const uint32_t tb = __float_as_uint(thr);
    if ((tb & 0x7F800000u) == 0x7F800000u) return (double)thr;   // +-inf, NaN: the comparison is the same in double
    const float below = thr > 0.0f ? __uint_as_float(tb - 1u)
                                   : (thr < 0.0f ? __uint_as_float(tb + 1u) : __uint_as_float(0x80000001u));
    const double mid = 0.5 * ((double)thr + (double)below);
    if ((tb & 1u) == 0) return mid;
    const int64_t mb = __double_as_longlong(mid);
    return __longlong_as_double(mid > 0.0 ? mb + 1 : mb - 1);
}

#ifndef PVQ_DIAG
#define PVQ_DIAG 0   // tools/pvq_variants.py (answers wrong; never shipped): 1 = no walk, 2 = no boundary sums, 4 = no l1 chain, 8 = no swaps,
                     // 16 = clock stamps, 32 = no MFMA, 64 = no run selection / division, 128 = no draw, 256 = no projection of the code, 512 = no staging
#endif
template <int D>
struct PwShape {
    static constexpr int HALF = D / 2;
    static constexpr int RS = D + 4;          // floats between staged rows (both operands): 16 consecutive rows cover the banks
    static constexpr int SI = 16 * RS + 4;    // floats between in-run indices i: codeword 16 hb + i at i * SI + hb * RS
    static constexpr int NQ = D / 4;          // float4s per row
    static constexpr int KQ = HALF / 4;       // float4s per half row
    static constexpr int CB_FLOATS = 16 * SI;
    static constexpr int TILE_FLOATS = 64 * RS;
    static constexpr size_t LDS_BYTES = (size_t)(CB_FLOATS + ENC_WAVES * TILE_FLOATS) * sizeof(float);
};

// $GQ_PVQ_EPS (tests): a wide window sends most lanes through the wave walk (negative: ... through the term-by-term walk)
inline double pw_eps_from_env() {
    const char *e = getenv("GQ_PVQ_EPS");
    const double v = e ? atof(e) : 0.0;
    return fabs(v) > 0x1.1p-22 ? v : 0x1.1p-22;
}

// codebook (c_dagger [K, D]) into LDS: codeword 16 hb + i as [even elements | odd elements] at i * SI + hb * RS
template <int D>
__device__ __forceinline__ void pw_stage_codebook(const float *__restrict__ cdag, int K, float *s_cb) {
    using S = PwShape<D>;
    for (int idx = threadIdx.x; idx < K * S::NQ; idx += ENC_THREADS) {
        const int row = idx / S::NQ, p = idx - row * S::NQ;
        const f32x4 c = *reinterpret_cast<const f32x4 *>(cdag + (int64_t)row * D + 4 * p);
        float *dst = s_cb + (row & 15) * S::SI + (row >> 4) * S::RS + 2 * p;
        *reinterpret_cast<pv_f32x2 *>(dst) = pv_f32x2{c[0], c[2]};
        *reinterpret_cast<pv_f32x2 *>(dst + S::HALF) = pv_f32x2{c[1], c[3]};
    }
}

// one float4 of a tile (quarter-row e0 of row rr) into the wave's staged tile, even / odd elements apart
template <int D>
__device__ __forceinline__ void pw_stage_quad(float *s_v, int rr, int e0, const f32x4 &val) {
    using S = PwShape<D>;
    float *row = s_v + rr * S::RS + (e0 >> 1);
    *reinterpret_cast<pv_f32x2 *>(row) = pv_f32x2{val[0], val[2]};
    *reinterpret_cast<pv_f32x2 *>(row + S::HALF) = pv_f32x2{val[1], val[3]};
}

// the lane's own subvector against one staged codeword row: the fmaf chain over ascending elements
template <int D>
__device__ __forceinline__ float pw_project(const float *crow, const f32x4 (&ve)[PwShape<D>::KQ], const f32x4 (&vo)[PwShape<D>::KQ]) {
    using S = PwShape<D>;
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < S::KQ; ++k) {
        const f32x4 ce = *reinterpret_cast<const f32x4 *>(crow + 4 * k);
        const f32x4 co = *reinterpret_cast<const f32x4 *>(crow + S::HALF + 4 * k);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            acc = __fmaf_rn(ce[q], ve[k][q], acc);
            acc = __fmaf_rn(co[q], vo[k][q], acc);
        }
    }
    return acc;
}

// The encode of the tile staged in s_v (the wave's 64 subvectors, lane L owns subvector L; `mine`: it exists): sweep 1, the
// draw -- draw(l1) is called once per lane, after the sweep --, the run selection, the lane-local walk and the two walks
// behind it.  -> code (< K) and val = sign(p_code) * l1 of the lane's subvector (left as they are when !mine).
template <int D, class Draw>
__device__ __forceinline__ void pw_encode_tile(const float *s_cb, const float *s_v, int K, bool mine, Draw draw, double eps,
                                               bool force_slow, int &code_out, float &val_out) {
    using S = PwShape<D>;
    constexpr int HALF = S::HALF, RS = S::RS, SI = S::SI, KQ = S::KQ;
    const int lane = threadIdx.x & 63;
    const int j = lane & 31, h = lane >> 5;
    const int nb = K >> 5;
    // ---- sweep 1: l1 (sequential f32, the reference's sum) and the block boundaries' running sums in double
    float l1 = 0.0f;
    double P[16];
    float S8[16];   // the first eight terms of every run of 16, as they entered the running sum
    {
        f32x4 xb0[KQ], xb1[KQ];
        const float *b0 = s_v + j * RS + h * HALF;
        const float *b1 = s_v + (32 + j) * RS + h * HALF;
#pragma unroll
        for (int k = 0; k < KQ; ++k) {
            xb0[k] = *reinterpret_cast<const f32x4 *>(b0 + 4 * k);
            xb1[k] = *reinterpret_cast<const f32x4 *>(b1 + 4 * k);
        }
        double run = 0.0;
#pragma unroll
        for (int rb = 0; rb < 8; ++rb) {
            P[2 * rb] = P[2 * rb + 1] = INFINITY;
            S8[2 * rb] = S8[2 * rb + 1] = 0.0f;
            if (rb < nb) {
                const float *arow = s_cb + (j & 15) * SI + (2 * rb + (j >> 4)) * RS + h * HALF;
                f32x16 acc0 = {0}, acc1 = {0};
#pragma unroll
                for (int k = 0; k < KQ; ++k) {
                    const f32x4 a = *reinterpret_cast<const f32x4 *>(arow + 4 * k);
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        if (PVQ_DIAG & 32) {
                            acc0[4 * k + q] = a[q] * xb0[k][q];
                            acc1[4 * k + q] = a[q] * xb1[k][q];
                            continue;
                        }
                        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q], xb0[k][q], acc0, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q], xb1[k][q], acc1, 0, 0, 0);
                    }
                }
                // lane L <- the 32 scores of subvector L: x[4g..] = codewords 8g..8g+3 of the block, yv[4g..] = 8g+4..8g+7
                float x[16], yv[16];
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    x[q] = acc0[q];
                    yv[q] = acc1[q];
                    if (!(PVQ_DIAG & 8)) swap32(x[q], yv[q]);
                }
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    if (PVQ_DIAG & 4) {
                        l1 = l1 + fabsf(x[4 * g]) + fabsf(yv[4 * g + 3]);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) l1 = l1 + fabsf(x[4 * g + e]);
#pragma unroll
                        for (int e = 0; e < 4; ++e) l1 = l1 + fabsf(yv[4 * g + e]);
                    }
                    if (PVQ_DIAG & 2) {
                        if (g & 1) P[2 * rb + (g >> 1)] = (double)l1;
                        continue;
                    }
                    const float s8 = ((fabsf(x[4 * g]) + fabsf(x[4 * g + 1])) + (fabsf(x[4 * g + 2]) + fabsf(x[4 * g + 3]))) +
                                     ((fabsf(yv[4 * g]) + fabsf(yv[4 * g + 1])) + (fabsf(yv[4 * g + 2]) + fabsf(yv[4 * g + 3])));
                    run = run + (double)s8;
                    if (g & 1) P[2 * rb + (g >> 1)] = run;
                    else S8[2 * rb + (g >> 1)] = s8;
                }
            }
        }
    }
    const float rr = (PVQ_DIAG & 128) ? 0.5f : draw(l1);
    const float thr = rr - 1e-5f;
    const double T = (PVQ_DIAG & 128) ? 0.5 : rounds_up_to_threshold(thr);   // (float)x >= thr  <=>  x >= T
    // ---- the block whose boundaries bracket the threshold, and the walk's value at its start
    const double U = T * (double)l1;
    double startP = 0.0;
    float mid = S8[0];
    int bstar = 0;
#pragma unroll
    for (int b = 0; b < ((PVQ_DIAG & 64) ? 1 : 15); ++b) {
        const bool below = (b < 2 * nb - 1) && (P[b] < U);
        startP = below ? P[b] : startP;
        mid = below ? S8[b + 1] : mid;
        bstar = below ? b + 1 : bstar;
    }
    // ... and the half of that run: the running sum after its first eight terms is startP + mid, as sweep 1 formed it
    {
        const double midP = startP + (double)mid;
        const bool second = midP < U;
        startP = second ? midP : startP;
        bstar = 2 * bstar + (second ? 1 : 0);   // from here on: a run of EIGHT codewords
    }
    f32x4 ve[KQ], vo[KQ];
    {
        const float *v = s_v + lane * RS;
#pragma unroll
        for (int k = 0; k < KQ; ++k) {
            ve[k] = *reinterpret_cast<const f32x4 *>(v + 4 * k);
            vo[k] = *reinterpret_cast<const f32x4 *>(v + HALF + 4 * k);
        }
    }
    const double Tlo = T - eps, Thi = T + eps;
    double cum = (PVQ_DIAG & 64) ? startP * (double)l1 : startP / (double)l1;
    const bool start_ok = cum < Tlo;
    const float y = 1.0f / l1;
    int cnt_lo = 0, cnt_hi = 0;
    float amin = INFINITY;
    {
        // the run's 8 codeword rows, each fetched one projection ahead of its use
        const float *crow = s_cb + (bstar >> 1) * RS + (bstar & 1) * 8 * SI;
        f32x4 ce[2][KQ], co[2][KQ];
        auto fetch_row = [&](int i, int buf) {
#pragma unroll
            for (int k = 0; k < KQ; ++k) {
                ce[buf][k] = *reinterpret_cast<const f32x4 *>(crow + i * SI + 4 * k);
                co[buf][k] = *reinterpret_cast<const f32x4 *>(crow + i * SI + HALF + 4 * k);
            }
        };
        fetch_row(0, 0);
#pragma unroll
        for (int i = 0; i < ((PVQ_DIAG & 1) ? 1 : 8); ++i) {
            if (i + 1 < 8) fetch_row(i + 1, (i + 1) & 1);
            float acc = 0.0f;
#pragma unroll
            for (int k = 0; k < KQ; ++k) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    acc = __fmaf_rn(ce[i & 1][k][q], ve[k][q], acc);
                    acc = __fmaf_rn(co[i & 1][k][q], vo[k][q], acc);
                }
            }
            const float a = fabsf(acc);
            amin = fminf(amin, a);
            cum = cum + (double)shared_quotient(a, l1, y);
            cnt_lo += (cum < Tlo) ? 1 : 0;
            cnt_hi += (cum < Thi) ? 1 : 0;
        }
    }
    int count = bstar * 8 + cnt_lo;
    bool settled = l1 >= 0x1p-80f && l1 <= 0x1p20f && amin >= 0x1p-102f && start_ok && cnt_lo == cnt_hi &&
                   (cnt_lo < 8 || bstar == 4 * nb - 1);
    if (l1 == 0.0f) {   // an all-zero subvector: every term is 0 / 0, every comparison with NaN fails, all K terms count
        count = K;
        settled = true;
    }
    // ---- the unsettled lanes (one in ~2^-13), one at a time by the whole wave: lane L takes codewords 4L .. 4L+3 of
    // the lane's subvector, divides as the reference does, and the running sums come from a wave-wide prefix sum in
    // double.  That equals the sequential sum bit for bit when every non-zero quotient is at least 2^-29: all terms
    // and all partial sums are then multiples of 2^-52 below 2, every double addition is exact in any order.
    // Otherwise (and for a non-finite l1) the lane walks its K terms alone, one after the other.
    uint64_t todo = (PVQ_DIAG & ~16) ? 0 : __builtin_amdgcn_ballot_w64(mine && !settled);
    while (todo) {
        const int src = (int)__builtin_ctzll(todo);
        todo &= todo - 1;
        const float l1s = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(l1), src));
        const float thrs = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(thr), src));
        f32x4 se[KQ], so[KQ];
#pragma unroll
        for (int k = 0; k < KQ; ++k) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float e_own = ve[k][q], o_own = vo[k][q];   // (scalars first: a bit_cast of the vector element
                se[k][q] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(e_own), src));   // read element 0 four times)
                so[k][q] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(o_own), src));
            }
        }
        double inc[4];
        double tot = 0.0;
        bool exact = !force_slow;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int k = 4 * lane + c;
            float q = 0.0f;
            if (k < K) q = fabsf(pw_project<D>(s_cb + (k & 15) * SI + (k >> 4) * RS, se, so)) / l1s;
            exact = exact && (q == 0.0f || (q >= 0x1p-29f && q <= 2.0f));
            tot = tot + (double)q;
            inc[c] = tot;
        }
        double before = tot;   // inclusive prefix over the lanes, then made exclusive
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const double up = __shfl_up(before, off, 64);
            if (lane >= off) before = before + up;
        }
        before = before - tot;   // exact: both are multiples of 2^-52 below 2
        int n = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) n += (4 * lane + c < K && !((float)(before + inc[c]) >= thrs)) ? 1 : 0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
        if (__builtin_amdgcn_ballot_w64(!exact) == 0) {
            if (lane == src) count = n;
        } else if (lane == src) {
            // term by term over all K codewords, the reference's own arithmetic (as pvq_encode_kernel)
            double c2 = 0.0;
            int n2 = 0;
            for (int k = 0; k < K; ++k) {
                const float a = fabsf(pw_project<D>(s_cb + (k & 15) * SI + (k >> 4) * RS, ve, vo));
                c2 = c2 + (double)(a / l1);
                n2 += ((float)c2 >= thr) ? 0 : 1;
            }
            count = n2;
        }
    }
    if (!mine) return;
    const int code = count < K - 1 ? count : K - 1;
    const float sel = (PVQ_DIAG & 256) ? ve[0][0] : pw_project<D>(s_cb + (code & 15) * SI + (code >> 4) * RS, ve, vo);
    const float sg = (sel > 0.0f) ? 1.0f : ((sel < 0.0f) ? -1.0f : 0.0f);
    code_out = code;
    val_out = sg * l1;
}

}  // namespace gq
