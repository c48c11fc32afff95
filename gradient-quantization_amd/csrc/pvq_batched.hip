// ProbabilisticVectorCompressor encode, multi-tensor (segment table) form -- libgq_pvq.so (include/gq_pvq.h).
//
// One launch encodes every tensor of a model that shares a codebook into one user's wire, over the tables the multi-tensor
// HSQ launches use (gq_hsq_batch).  The kernel is pw_encode_run (pvq_walk.hpp: a wave owns a run of consecutive tiles, the
// tile encode is pvq_encode_walk_kernel's, so a tensor's codes and projections are gq_pvq_encode's bit for bit) over the
// gradient source below: a tile of the gradient, or of  grad + ef_scale * error  written back over the gradient.
#include <math.h>
#include <stdlib.h>

#include "gq_pvq.h"
#include "pvq_walk_host.hpp"

#define GQP_API extern "C" __attribute__((visibility("default")))

namespace gqp {

using namespace gq;

static_assert(sizeof(gq_pvq_batch) == 24, "gq_pvq_batch: the layout the ctypes binding declares (gq_amd/native.py)");

using gql::err_buf;
using gql::fail;

struct PvbArgs {
    PwRunArgs run;
    float ef_scale;
};

// A tile of the gradient.  EF: with the tensor's error tile in flight beside it (NQ more float4s).
template <int D, bool EF>
struct GradSource {
    static constexpr int NQ = PwShape<D>::NQ;
    struct Tile : PwTile {
        uintptr_t err;      // EF: the tile's first float of the tensor's error buffer, 0 = none
    };
    const float ef_scale;
    f32x4 pre[NQ], pre_e[EF ? NQ : 1];

    __device__ __forceinline__ explicit GradSource(float scale) : ef_scale(scale) {}

    __device__ __forceinline__ Tile tile(const PwRunArgs &a, int64_t t) const {
        Tile ti;
        const pw_crec_ptr rec = pw_tile_common<D>(a, t, ti);
        ti.err = (EF && rec[7]) ? (uintptr_t)rec[7] + (uintptr_t)ti.local0 * (D * sizeof(float)) : 0;
        ti.codes = (pw_gcode_ptr)((uintptr_t)a.wire + (uintptr_t)(rec[3] + ti.local0));
        return ti;
    }
    __device__ __forceinline__ void fetch(const Tile &ti) {
        pw_fetch_rows<D>(pre, ti.grad, ti.left);
        if constexpr (EF) {
            if (ti.err) pw_fetch_rows<D>(pre_e, ti.err, ti.left);
        }
    }
    __device__ __forceinline__ void commit(const Tile &ti, float *s_v) {
        const int lane = threadIdx.x & 63;
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            const int q = i * 64 + lane;
            const int rr = q / NQ;
            const int e0 = (q - rr * NQ) * 4;
            f32x4 val = pre[i];
            if (EF && ti.err && rr < ti.left) {      // v = grad + ef_scale * error (ps_quantizer.py:35), back over grad
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float prod = ef_scale * pre_e[i][e];
                    val[e] = val[e] + prod;
                }
                *(pw_gv_ptr)(ti.grad + (unsigned)q * 16u) = val;
            }
            pw_stage_quad<D>(s_v, rr, e0, val);
        }
    }
};

// Registers (-Rpass-analysis=kernel-resource-usage, profiles/pvq_run_ab.txt; no scratch, no AGPRs): d = 8 runs three waves per
// SIMD with and without error feedback, d = 16 three without it.  With the error tile beside the gradient tile d = 16 does
// not fit three waves' 168 registers without spilling and is built for two, which the flat kernel measured as ~2 % (pvq.hip);
// d = 32 needs its 200+ and runs two.
template <int D, bool EF>
__global__ __launch_bounds__(ENC_THREADS) __attribute__((amdgpu_waves_per_eu(D <= 16 ? ((EF && D == 16) ? 2 : 3) : 1))) void pvq_encode_walk_batched_kernel(const PvbArgs a) {
    GradSource<D, EF> src(a.ef_scale);
    pw_encode_run<D>(a.run, src);
}

template <int D, bool EF>
static int launch(const PvbArgs &a, hipStream_t st) {
    return pw_launch_run<D, pvq_encode_walk_batched_kernel<D, EF>>(a, st, "gq_pvq_encode_batched");
}

}  // namespace gqp

GQP_API int gq_pvq_abi_version(void) { return GQ_PVQ_ABI_VERSION; }

GQP_API const char *gq_pvq_last_error(void) { return gqp::err_buf; }

GQP_API int gq_pvq_batched_serves(int d, int K, int code_bytes) { return gq::pw_run_serves(d, K, code_bytes) ? 1 : 0; }

GQP_API int gq_pvq_encode_batched(const gq_pvq_batch *b, uint8_t *wire, int random_mode, uint64_t seed, const float *r_flat,
                                  float ef_scale, void *stream) {
    using gqp::fail;
    if (!b || b->struct_bytes != sizeof(gq_pvq_batch)) return fail(GQ_ERR_INVALID_ARG, "gq_pvq_encode_batched: gq_pvq_batch of another layout");
    const gq_hsq_batch *h = b->hsq;
    if (!h || h->struct_bytes != sizeof(gq_hsq_batch)) return fail(GQ_ERR_INVALID_ARG, "gq_pvq_encode_batched: gq_hsq_batch of another layout");
    if (!gq_pvq_batched_serves(h->d, h->K, h->code_bytes))
        return fail(GQ_ERR_UNSUPPORTED, "gq_pvq_encode_batched: d = %d, K = %d, %d-byte codes (served: d in {8, 16, 32}, K = 32 ... 256 in "
                                        "whole blocks of 32, byte codes)", h->d, h->K, h->code_bytes);
    if (h->nseg < 1 || h->ntiles < 1) return fail(GQ_ERR_INVALID_ARG, "gq_pvq_encode_batched: bad sizes");
    if (!h->seg_table || !h->tile_seg || !h->u_flat || !h->seg_minmax || !b->c_dagger || !wire)
        return fail(GQ_ERR_INVALID_ARG, "gq_pvq_encode_batched: null pointer");
    if (reinterpret_cast<uintptr_t>(b->c_dagger) & 15) return fail(GQ_ERR_INVALID_ARG, "gq_pvq_encode_batched: c_dagger must be 16-byte aligned");
    const int rc = gq::pw_check_draws(random_mode, seed, r_flat, "gq_pvq_encode_batched");
    if (rc != GQ_OK) return rc;
    static const double eps = gq::pw_eps_from_env();   // $GQ_PVQ_EPS (tests)
    gqp::PvbArgs a;
    a.run.seg_table = h->seg_table;
    a.run.tile_seg = h->tile_seg;
    a.run.ntiles = h->ntiles;
    a.run.cdag = b->c_dagger;
    a.run.wire = wire;
    a.run.u_flat = h->u_flat;
    a.run.seg_minmax = h->seg_minmax;
    a.run.r_flat = r_flat;
    a.run.seed = seed;
    a.run.eps = eps;
    a.run.K = h->K;
    a.run.random_mode = random_mode;
    a.ef_scale = ef_scale;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const bool ef = ef_scale == ef_scale;
    switch (h->d) {
        case 8: return ef ? gqp::launch<8, true>(a, st) : gqp::launch<8, false>(a, st);
        case 16: return ef ? gqp::launch<16, true>(a, st) : gqp::launch<16, false>(a, st);
        default: return ef ? gqp::launch<32, true>(a, st) : gqp::launch<32, false>(a, st);
    }
}
