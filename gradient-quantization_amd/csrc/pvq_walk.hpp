// The ProbabilisticVectorCompressor's encode as device code, written once for its three users:
//   pvq.hip          gq_pvq_encode: one tensor per launch, tiles one grid apart, partials in the workspace (libgq_hsq.so)
//   pvq_batched.hip  gq_pvq_encode_batched: every tensor of a model per launch, tiles of the gradient (libgq_pvq.so)
//   rq_batched.hip   gq_rq_encode2_batched: the same over  v - decode(stage 1)  (libgq_rq.so)
// pw_encode_tile is the one-sweep + lane-local-walk encode of a 64-subvector tile (the scheme is described where it was
// written: pvq.hip, in front of pvq_encode_walk_kernel): one body, so all three give the same bits.  pw_encode_run is the whole
// kernel of the two multi-tensor launches -- a wave's RUN of consecutive tiles over the segment tables -- around a tile source
// that each file defines; pvq.hip keeps a loop of its own and shares the LDS carve-up, the row fetch and stage 1's residual.
#pragma once
#include "hsq_pf_common.hpp"      // order_map; hsq_encode_common.hpp

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

// ---- what the kernels around the tile encode share -------------------------------------------------------------------------

// the draws of the sampler and the level quantiser's stochastic rounding come from different streams of one seed: the
// multi-tensor launches of both libraries salt theirs with this (tests/rq_contract.py and tests/test_gpu_pvq.py hold copies)
constexpr uint64_t PW_SAMPLER_SALT = 0xA0761D6478BD642Full;

// Pointers out of the segment table are cast to GLOBAL pointers (address space 1): as plain pointers they would be flat,
// and the wait for a flat access sits behind the previous tile's stores (hsq_encode_pf.hip); members of a by-value argument
// struct are flat pointers otherwise, too.  The tables themselves do not change while the kernel runs: read through the
// constant address space they are scalar loads.
typedef const f32x4 __attribute__((address_space(1))) *pw_gcv_ptr;
typedef f32x4 __attribute__((address_space(1))) *pw_gv_ptr;
typedef uint8_t __attribute__((address_space(1))) *pw_gcode_ptr;
typedef float __attribute__((address_space(1))) *pw_gf_ptr;
typedef const float __attribute__((address_space(1))) *pw_gcf_ptr;
typedef unsigned __attribute__((address_space(1))) *pw_gu_ptr;
typedef const int64_t __attribute__((address_space(4))) *pw_crec_ptr;
typedef const int32_t __attribute__((address_space(4))) *pw_cseg_ptr;

// the workgroup's dynamic LDS (PwShape<D>::LDS_BYTES): the staged codebook, then one tile per wave
struct PwLds {
    float *cb, *v;
};
template <int D>
__device__ __forceinline__ PwLds pw_carve_lds(int wave) {
    extern __shared__ __attribute__((aligned(16))) float pw_lds[];
    return PwLds{pw_lds, pw_lds + PwShape<D>::CB_FLOATS + wave * PwShape<D>::TILE_FLOATS};
}

// the wave's ordering point between its reads of a staged tile and the stores of the next one (and back)
__device__ __forceinline__ void pw_wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// The float4s of a tile's rows below `left` into pre[] (zeros above): float4 q = i * 64 + lane of the tile is row q / NQ,
// elements 4 (q mod NQ) ..., 16 q bytes behind `base`, the tile's first float.
template <int D>
__device__ __forceinline__ void pw_fetch_rows(f32x4 (&pre)[PwShape<D>::NQ], uintptr_t base, int left) {
    constexpr int NQ = PwShape<D>::NQ;
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        const int q = i * 64 + lane;
        pre[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        if (q / NQ < left) pre[i] = *(pw_gcv_ptr)(base + (unsigned)q * 16u);
    }
}

// one float4 of  v - codebook1[code1] * norm1 : gq_pvq_encode's stage1 form and the residual compressor's second stage
__device__ __forceinline__ void pw_residual_quad(f32x4 &val, const f32x4 c, float n1) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float dec = c[e] * n1;   // stage 1's decoded element (product rounded)
        val[e] = val[e] - dec;         // residuals -= decompressed (residual_compressor.py:22)
    }
}

// What both multi-tensor launches are given: gq_hsq_batch's tables (tile_seg names the tensor of every 64-subvector tile,
// seg_table its pointers, sizes and wire offsets), the sampler's codebook and draws, and where the results go.
struct PwRunArgs {
    const int64_t *seg_table;
    const int32_t *tile_seg;
    int64_t ntiles;
    const float *cdag;
    uint8_t *wire;
    float *u_flat;
    unsigned *seg_minmax;
    const float *r_flat;
    uint64_t seed;
    double eps;
    int K, random_mode;
    int tiles_per_wave, waves_with_one_more;      // a wave's RUN of consecutive tiles: ntiles = waves * tiles_per_wave + waves_with_one_more
};

// What the walker reads of a tile; wave-uniform, in scalar registers.  A source's Tile derives from it.
struct PwTile {
    uintptr_t grad;         // the tile's first float
    pw_gcode_ptr codes;     // where the tile's first code goes (the source sets it)
    int64_t local0;         // the tile's first subvector within its tensor
    int left;               // subvectors of the tensor from the tile's start on, capped at 64
    int seg;
};
// seg, local0, left and grad of tile t from the tables -> the tensor's record (scalar loads)
template <int D>
__device__ __forceinline__ pw_crec_ptr pw_tile_common(const PwRunArgs &a, int64_t t, PwTile &ti) {
    ti.seg = ((pw_cseg_ptr)(uintptr_t)a.tile_seg)[t];
    const pw_crec_ptr rec = (pw_crec_ptr)(uintptr_t)(a.seg_table + 8 * (int64_t)ti.seg);
    ti.local0 = (t - rec[2]) * 64;
    const int64_t left = rec[1] - ti.local0;
    ti.left = left < 64 ? (int)left : 64;
    ti.grad = (uintptr_t)rec[0] + (uintptr_t)ti.local0 * (D * sizeof(float));
    return rec;
}

// The body of a multi-tensor encode kernel (ENC_THREADS lanes, PwShape<D>::LDS_BYTES of dynamic LDS).  A wave owns a tile at
// a time; per tile the encode is pw_encode_tile, so a tensor's codes and projections are gq_pvq_encode's bit for bit.  What
// differs between the launches is the Source:
//   struct Tile : PwTile { ... };                  the tile's record
//   Tile tile(const PwRunArgs &, int64_t t)        ... from the tables (pw_tile_common + its own fields, `codes` among them)
//   void fetch(const Tile &)                       the tile's global loads into the source's registers
//   void commit(const Tile &, float *s_v)          ... into the wave's staged tile (pw_stage_quad), as the values to encode
// A tile's record is loaded one tile ahead of the tile's fetch, the fetch one tile ahead of its encode.  When the tensor
// changes, the wave's running (min, max) of u is folded into the tensor's order-mapped words, which the level launch of
// libgq_hsq.so unmaps into (lb, ub).  Like the flat kernel's fminf / fmaxf fold, the words never see a NaN projection.
template <int D, class Source>
__device__ __forceinline__ void pw_encode_run(const PwRunArgs &a, Source &src) {
    using Tile = typename Source::Tile;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const PwLds lds = pw_carve_lds<D>(wave);
    const bool force_slow = a.eps < 0.0;   // tests: every unsettled lane walks term by term
    const double eps = fabs(a.eps);
    int random_mode = a.random_mode;
    uint64_t seed = a.seed;
    resolve_seed(random_mode, seed);       // GQ_RANDOM_DEVICE_COUNTER: { seed, step } words -> this launch's seed
    seed ^= PW_SAMPLER_SALT;
    pw_stage_codebook<D>(a.cdag, a.K, lds.cb);
    __syncthreads();
    const pw_gf_ptr u_flat = (pw_gf_ptr)(uintptr_t)a.u_flat;
    const pw_gcf_ptr r_flat = (pw_gcf_ptr)(uintptr_t)a.r_flat;
    const pw_gu_ptr seg_minmax = (pw_gu_ptr)(uintptr_t)a.seg_minmax;
    float lmin = INFINITY, lmax = -INFINITY;
    int cur_seg = -1;
    // the wave's running (min, max) into its tensor's words.  Look before the atomic: the words only move towards the
    // extremes, so a value that is already as good as ours -- however stale -- makes ours redundant (hsq_encode_pf.hip)
    auto flush_minmax = [&]() {
        const float lo = wave_min(lmin), hi = wave_max(lmax);
        if (lane == 0 && cur_seg >= 0) {
            const pw_gu_ptr mm = seg_minmax + 2 * cur_seg;
            const unsigned mlo = order_map(lo), mhi = order_map(hi);
            if (mlo < __hip_atomic_load(mm, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) (void)__hip_atomic_fetch_min(mm, mlo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (mhi > __hip_atomic_load(mm + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) (void)__hip_atomic_fetch_max(mm + 1, mhi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        lmin = INFINITY;
        lmax = -INFINITY;
    };
    // A wave takes a RUN of consecutive tiles (the flat kernel strides by the grid): consecutive tiles mostly belong to one
    // tensor, so the wave folds into a tensor's (min, max) words once per run instead of once per tile.  With the grid's
    // stride every wave changed tensor at nearly every tile of a list of mid-sized tensors, and the ~23,000 look-ups and
    // atomics of a ResNet-50 step on a handful of cache lines serialised in L2: 76 equal tensors took 344 us against 144 us for
    // the same elements as one tensor (profiles/pvq_encode_grid_stride.jsonl; now 162 us: profiles/pvq_step_time.jsonl).  Same tiles per wave either way; same results.
    const int wid = (int)blockIdx.x * ENC_WAVES + wave;
    int64_t t = (int64_t)wid * a.tiles_per_wave + (wid < a.waves_with_one_more ? wid : a.waves_with_one_more);
    const int64_t t_end = t + a.tiles_per_wave + (wid < a.waves_with_one_more ? 1 : 0);
    Tile cur = {}, nxt = {};
    if (t < t_end) {
        cur = src.tile(a, t);
        src.fetch(cur);
    }
    for (; t < t_end; ++t) {
        const bool more = t + 1 < t_end;
        if (more) nxt = src.tile(a, t + 1);
        pw_wave_fence();   // the previous tile's reads are done
        src.commit(cur, lds.v);
        if (more) src.fetch(nxt);
        pw_wave_fence();   // the tile is staged
        if (cur.seg != cur_seg) {      // wave-uniform
            flush_minmax();
            cur_seg = cur.seg;
        }
        const bool mine = lane < cur.left;
        const uint64_t idx = (uint64_t)t * 64 + (uint64_t)lane;      // the subvector's slot in the padded space (u_flat, r_flat)
        int code = 0;
        float val = 0.0f;
        pw_encode_tile<D>(lds.cb, lds.v, a.K, mine,
                          [&](float l1) {
                              if (!mine) return 0.0f;
                              if (random_mode == GQ_RANDOM_GIVEN) return r_flat[idx];
                              return uniform01(random_mode == GQ_RANDOM_DEVICE_KEYED ? keyed_seed(seed, l1, l1) : seed, idx);
                          },
                          eps, force_slow, code, val);
        if (mine) {
            cur.codes[lane] = (uint8_t)code;
            u_flat[idx] = val;
            lmin = fminf(lmin, val);
            lmax = fmaxf(lmax, val);
        }
        cur = nxt;
    }
    flush_minmax();
}

}  // namespace gq
