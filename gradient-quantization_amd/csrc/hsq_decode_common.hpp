// What the d = 16 / K = 256 decode kernels of hsq_decode.hip (one tensor) and hsq_batched.hip (a segment table) share: the
// payload step on the four-copy codebook image, that image's two stagings, and the padded-row image of the other kernels.
#pragma once
#include "gq_common.hpp"

namespace gq {

// LDS row stride (floats) of a staged codebook.  Rows of d floats laid end to end start on very few
// bank positions (d = 16: 64 B rows, the 128 B bank window has TWO), and a gather of 16 random rows
// per ds_read_b128 then serialises ~8 ways (PMC: 16 conflict cycles per LDS instruction, LDS stalled 61 %
// of an R = 8 decode).  An odd number of 16-byte units per row spreads the row starts over all positions.
__host__ __device__ constexpr int cb_row_stride(int d) { return ((d >> 2) & 1) ? d : d + 4; }

// The padded-row image: K rows of D floats, cb_row_stride(D) floats apart, by a workgroup of THREADS (K <= 256 rows; codes
// stay below K).  The caller's barrier follows.
template <int D, int THREADS>
__device__ __forceinline__ void stage_cb_rows(float *s_cb, const float *cb, int K) {
    constexpr int UPS = D / 4, RS = cb_row_stride(D);
    for (int i = threadIdx.x; i < K * UPS; i += THREADS)
        *reinterpret_cast<f32x4 *>(s_cb + (i / UPS) * RS + 4 * (i % UPS)) = reinterpret_cast<const f32x4 *>(cb)[i];
}

// The four-copy image of a d = 16 codebook: [K][4 copies][16], row r copy c at byte r*256 + c*64.  A ds_read_b128 is served
// in four fixed groups of 16 lanes (MI355X_MICROARCH.md, LDS): the four 4-lane teams of a group (one subvector each, 64
// contiguous bytes) read copies 0..3, so every group covers the 64 banks exactly once whatever the codes are:
// conflict-free, 256 B/clk.  Staged directly ...
template <int THREADS>
__device__ __forceinline__ void stage_cb4(float *s_cb, const float *cb, int K) {
    for (int i = threadIdx.x; i < K * 16; i += THREADS) {   // (row, copy, quarter)
        const int row = i >> 4, c = (i >> 2) & 3, q = i & 3;
        *reinterpret_cast<f32x4 *>(s_cb + row * 64 + c * 16 + 4 * q) = *reinterpret_cast<const f32x4 *>(cb + row * 16 + 4 * q);
    }
}

// ... or through registers, by the kernels that request their first payload words before load() so that those round trips
// run under the staging: load() the rows, do what else the prologue has, store() the image.
template <int THREADS>
struct Cb4Stage {
    static constexpr int N = (256 * 16 + THREADS - 1) / THREADS;   // K <= 256 rows of four copies of four 16-byte quarters
    f32x4 v[N];
    __device__ __forceinline__ void load(const float *cb, int K) {
#pragma unroll
        for (int n = 0; n < N; ++n) {
            const int e = threadIdx.x + n * THREADS;   // (row, copy, quarter)
            if (e < K * 16) v[n] = *reinterpret_cast<const f32x4 *>(cb + (e >> 4) * 16 + 4 * (e & 3));
        }
    }
    __device__ __forceinline__ void store(float *s_cb, int K) const {
#pragma unroll
        for (int n = 0; n < N; ++n) {
            const int e = threadIdx.x + n * THREADS;
            const int row = e >> 4, c = (e >> 2) & 3, qq = e & 3;
            if (e < K * 16) *reinterpret_cast<f32x4 *>(s_cb + row * 64 + c * 16 + 4 * qq) = v[n];
        }
    }
};

// LDS byte address of a codebook row for this lane: code * 256 + (copy * 64 + quarter * 16), built by ONE v_perm_b32
// from byte k of the packed codes and the lane's constant (< 256): [0, 0, code_k, lane_const].
template <int K4>
__device__ __forceinline__ unsigned row_addr(unsigned c4, unsigned lane_const) {
    return __builtin_amdgcn_perm(c4, lane_const, 0x0c0c0000u | ((4u + K4) << 8));
}

// One payload's contribution to the four subvectors of a team (a thread produces the same quarter of FOUR consecutive
// subvectors; c4 / l4 are their codes and levels): norms by lane q, shared through quad-permute DPP moves;
// probabilistic_scalar_compressor.py:31-32 unfused (level_to_norm), nearest_neighbor_compressor.py:88.
// ABS0: the codebook image starts at LDS address 0 (a kernel whose only LDS is its dynamic array) and the v_perm_b32
// result IS the address; through a pointer the compiler adds the array's link-time base (0) to every row address.
typedef const f32x4 __attribute__((address_space(3))) lds_f32x4;
// FMA (opt-in, GQ_AGGREGATE_FMA in n_bit; payloads after the first): acc = fma(c, n, acc) instead of the reference's
// separately rounded product and sum -- half the operations per payload, within 1e-6 relative L2 of the exact mean
// (north_star grants 1e-5 on the decoded aggregate); never used for a plain decompress, R = 1 or error-feedback round trips.
template <bool FIRST, bool PACKED6, bool ABS0 = false, bool FMA = false>
__device__ __forceinline__ void dec16_payload(f32x4 (&acc)[4], unsigned c4, unsigned l4, float lb, float range, float inv_s,
                                              int q, const char *cb_bytes, unsigned lane_const) {
    const float n_own = level_to_norm<unsigned>(PACKED6 ? ((l4 >> (6 * q)) & 63u) : ((l4 >> (8 * q)) & 255u), lb, range, inv_s);
    const int n_bits = __builtin_bit_cast(int, n_own);
    const float n_team[4] = {   // quad_perm [k,k,k,k]: lane k of the team broadcasts
        __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(n_bits, 0x00, 0xF, 0xF, true)),
        __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(n_bits, 0x55, 0xF, 0xF, true)),
        __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(n_bits, 0xAA, 0xF, 0xF, true)),
        __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(n_bits, 0xFF, 0xF, 0xF, true))};
    const unsigned a[4] = {row_addr<0>(c4, lane_const), row_addr<1>(c4, lane_const), row_addr<2>(c4, lane_const),
                           row_addr<3>(c4, lane_const)};
    if constexpr (FMA && !FIRST) {      // one v_fmac_f32_dpp per element: the team's norms are read across the quad by the multiply-add itself
        const float n_rdy = quad_norm_ready(n_own);
        const f32x4 c0 = ABS0 ? *reinterpret_cast<lds_f32x4 *>((uintptr_t)a[0]) : *reinterpret_cast<const f32x4 *>(cb_bytes + a[0]);
        const f32x4 c1 = ABS0 ? *reinterpret_cast<lds_f32x4 *>((uintptr_t)a[1]) : *reinterpret_cast<const f32x4 *>(cb_bytes + a[1]);
        const f32x4 c2 = ABS0 ? *reinterpret_cast<lds_f32x4 *>((uintptr_t)a[2]) : *reinterpret_cast<const f32x4 *>(cb_bytes + a[2]);
        const f32x4 c3 = ABS0 ? *reinterpret_cast<lds_f32x4 *>((uintptr_t)a[3]) : *reinterpret_cast<const f32x4 *>(cb_bytes + a[3]);
        acc[0] = fmac_quad4<0>(acc[0], n_rdy, c0);
        acc[1] = fmac_quad4<1>(acc[1], n_rdy, c1);
        acc[2] = fmac_quad4<2>(acc[2], n_rdy, c2);
        acc[3] = fmac_quad4<3>(acc[3], n_rdy, c3);
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float n = n_team[k];
        const f32x4 c = ABS0 ? *reinterpret_cast<lds_f32x4 *>((uintptr_t)a[k])
                             : *reinterpret_cast<const f32x4 *>(cb_bytes + a[k]);
        const f32x4 n4 = {n, n, n, n};
        const f32x4 dec = c * n4;
        if constexpr (FIRST) {
            acc[k] = dec;
        } else {
            acc[k] = acc[k] + dec;
        }
    }
}

}  // namespace gq
