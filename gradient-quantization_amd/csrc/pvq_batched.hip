// ProbabilisticVectorCompressor encode, multi-tensor (segment table) form -- libgq_pvq.so (include/gq_pvq.h).
//
// One launch encodes every tensor of a model that shares a codebook into one user's wire, over the tables the multi-tensor
// HSQ launches use (gq_hsq_batch: tile_seg names the tensor of every 64-subvector tile, seg_table its pointers, sizes and
// wire offsets).  A wave owns a tile at a time, as in pvq_encode_walk_kernel (pvq.hip); the tile encode IS that kernel's
// (pw_encode_tile, pvq_walk.hpp: one f32 MFMA sweep over c_dagger, boundary sums in double, the eps-guarded lane-local walk,
// the wave walk and the term-by-term walk behind it), so a tensor's codes and projections are gq_pvq_encode's bit for bit.
// What is added per tile is wave-uniform and lives in scalar registers: the tile's tensor (tile_seg, scalar load), its
// record (scalar loads, one tile ahead of the tile's fetch; a wave owns a run of CONSECUTIVE tiles), and -- when the tensor changes -- the fold of the wave's running
// (min, max) of u into the tensor's order-mapped words, which the level launch of libgq_hsq.so unmaps into (lb, ub).
// Like the flat kernel's fminf / fmaxf fold, the words never see a NaN projection (a subvector with a NaN element).
#include <math.h>
#include <stdlib.h>

#include "gq_lib_prelude.hpp"
#include "gq_pvq.h"
#include "hsq_pf_common.hpp"
#include "pvq_walk.hpp"

#define GQP_API extern "C" __attribute__((visibility("default")))

namespace gqp {

using namespace gq;

static_assert(sizeof(gq_pvq_batch) == 24, "gq_pvq_batch: the layout the ctypes binding declares (gq_amd/native.py)");

using gql::err_buf;
using gql::fail;

static int cu_count_here() {
    static int cus = [] {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1)
            n = 256;
        return n;
    }();
    return cus;
}

// the draws of the sampler and the level quantiser's stochastic rounding come from different streams of one seed
constexpr uint64_t PVQ_STREAM_SALT = 0xA0761D6478BD642Full;

struct PvbArgs {
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
    float ef_scale;
    int tiles_per_wave, waves_with_one_more;      // a wave's RUN of consecutive tiles: ntiles = waves * tiles_per_wave + waves_with_one_more
};

// Registers: as pvq_encode_walk_kernel -- d <= 16 at three waves per SIMD (132 / 161 VGPRs, no scratch), d = 32 with its 200+.
// With error feedback the error tile is in flight beside the gradient tile (NQ more float4s): d = 16 then spills at three
// waves (168 VGPRs + 20 bytes of scratch) and is built for two, which the flat kernel measured as ~2 % (pvq.hip).
template <int D, bool EF>
__global__ __launch_bounds__(ENC_THREADS) __attribute__((amdgpu_waves_per_eu(D <= 16 ? ((EF && D == 16) ? 2 : 3) : 1))) void pvq_encode_walk_batched_kernel(const PvbArgs a) {
    using S = PwShape<D>;
    constexpr int NQ = S::NQ;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    float *const s_cb = lds;
    float *const s_v = lds + S::CB_FLOATS + wave * S::TILE_FLOATS;
    const bool force_slow = a.eps < 0.0;   // tests: every unsettled lane walks term by term
    const double eps = fabs(a.eps);
    int random_mode = a.random_mode;
    uint64_t seed = a.seed;
    resolve_seed(random_mode, seed);       // GQ_RANDOM_DEVICE_COUNTER: { seed, step } words -> this launch's seed
    seed ^= PVQ_STREAM_SALT;
    pw_stage_codebook<D>(a.cdag, a.K, s_cb);
    __syncthreads();

    // Pointers out of the segment table are cast to GLOBAL pointers (address space 1): as plain pointers they would be flat,
    // and the wait for a flat access sits behind the previous tile's stores (hsq_encode_pf.hip).  The tables themselves do
    // not change while the kernel runs: read through the constant address space they are scalar loads.
    typedef const f32x4 __attribute__((address_space(1))) *gcv_ptr;
    typedef f32x4 __attribute__((address_space(1))) *gv_ptr;
    typedef uint8_t __attribute__((address_space(1))) *gcode_ptr;
    typedef float __attribute__((address_space(1))) *gf_ptr;
    typedef const float __attribute__((address_space(1))) *gcf_ptr;
    typedef unsigned __attribute__((address_space(1))) *gu_ptr;
    const gf_ptr u_flat = (gf_ptr)(uintptr_t)a.u_flat;      // (members of a by-value argument struct are flat pointers otherwise)
    const gcf_ptr r_flat = (gcf_ptr)(uintptr_t)a.r_flat;
    const gu_ptr seg_minmax = (gu_ptr)(uintptr_t)a.seg_minmax;
    typedef const int64_t __attribute__((address_space(4))) *crec_ptr;
    typedef const int32_t __attribute__((address_space(4))) *cseg_ptr;
    struct Tile {
        uintptr_t grad;     // the tile's first float
        uintptr_t err;      // EF: ... of the tensor's error buffer, 0 = none
        gcode_ptr codes;    // the tile's first code in the wire
        int left;           // subvectors of the tensor from the tile's start on, capped at 64
        int seg;
    };
    auto tile_info = [&](int64_t t) {
        Tile ti;
        ti.seg = ((cseg_ptr)(uintptr_t)a.tile_seg)[t];
        const crec_ptr rec = (crec_ptr)(uintptr_t)(a.seg_table + 8 * (int64_t)ti.seg);
        const int64_t local0 = (t - rec[2]) * 64;
        const int64_t left = rec[1] - local0;
        ti.left = left < 64 ? (int)left : 64;
        ti.grad = (uintptr_t)rec[0] + (uintptr_t)local0 * (D * sizeof(float));
        ti.err = (EF && rec[7]) ? (uintptr_t)rec[7] + (uintptr_t)local0 * (D * sizeof(float)) : 0;
        ti.codes = (gcode_ptr)((uintptr_t)a.wire + (uintptr_t)(rec[3] + local0));
        return ti;
    };
    f32x4 pre[NQ], pre_e[EF ? NQ : 1];
    auto fetch_tile = [&](const Tile &ti) {
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            const int q = i * 64 + lane;
            const int rr = q / NQ;
            const unsigned off = (unsigned)q * 16u;      // float4 q of the tile: row q / NQ, elements 4 (q mod NQ) ...
            pre[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if (rr < ti.left) {
                pre[i] = *(gcv_ptr)(ti.grad + off);
                if (EF && ti.err) pre_e[i] = *(gcv_ptr)(ti.err + off);
            }
        }
    };
    auto commit_tile = [&](const Tile &ti) {
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            const int q = i * 64 + lane;
            const int rr = q / NQ;
            const int e0 = (q - rr * NQ) * 4;
            f32x4 val = pre[i];
            if (EF && ti.err && rr < ti.left) {      // v = grad + ef_scale * error (ps_quantizer.py:35), back over grad
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float prod = a.ef_scale * pre_e[i][e];
                    val[e] = val[e] + prod;
                }
                *(gv_ptr)(ti.grad + (unsigned)q * 16u) = val;
            }
            pw_stage_quad<D>(s_v, rr, e0, val);
        }
    };
    float lmin = INFINITY, lmax = -INFINITY;
    int cur_seg = -1;
    // the wave's running (min, max) into its tensor's words.  Look before the atomic: the words only move towards the
    // extremes, so a value that is already as good as ours -- however stale -- makes ours redundant (hsq_encode_pf.hip)
    auto flush_minmax = [&]() {
        const float lo = wave_min(lmin), hi = wave_max(lmax);
        if (lane == 0 && cur_seg >= 0) {
            const gu_ptr mm = seg_minmax + 2 * cur_seg;
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
        cur = tile_info(t);
        fetch_tile(cur);
    }
    for (; t < t_end; ++t) {
        const bool more = t + 1 < t_end;
        if (more) nxt = tile_info(t + 1);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // the previous tile's reads are done
        __builtin_amdgcn_wave_barrier();
        commit_tile(cur);
        if (more) fetch_tile(nxt);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (cur.seg != cur_seg) {      // wave-uniform
            flush_minmax();
            cur_seg = cur.seg;
        }
        const bool mine = lane < cur.left;
        const uint64_t idx = (uint64_t)t * 64 + (uint64_t)lane;      // the subvector's slot in the padded space (u_flat, r_flat)
        int code = 0;
        float val = 0.0f;
        pw_encode_tile<D>(s_cb, s_v, a.K, mine,
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

template <int D, bool EF>
static int launch(const PvbArgs &a, hipStream_t st) {
    constexpr size_t lds_bytes = PwShape<D>::LDS_BYTES;
    static const int bpc = [] {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(pvq_encode_walk_batched_kernel<D, EF>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
        (void)hipGetLastError();
        return resident_blocks_per_cu(pvq_encode_walk_batched_kernel<D, EF>, ENC_THREADS, lds_bytes);
    }();
    int64_t blocks = (a.ntiles + ENC_WAVES - 1) / ENC_WAVES;
    const int64_t cap = (int64_t)cu_count_here() * bpc;      // one resident wave of workgroups: none queues behind another
    if (blocks > cap) blocks = cap;
    PvbArgs b = a;
    const int64_t waves = blocks * ENC_WAVES;
    b.tiles_per_wave = (int)(a.ntiles / waves);
    b.waves_with_one_more = (int)(a.ntiles - (int64_t)b.tiles_per_wave * waves);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(pvq_encode_walk_batched_kernel<D, EF>), dim3((unsigned)blocks), dim3(ENC_THREADS), lds_bytes, st, b);
    GQL_CHECK_LAUNCH("gq_pvq_encode_batched");
    return GQ_OK;
}

}  // namespace gqp

GQP_API int gq_pvq_abi_version(void) { return GQ_PVQ_ABI_VERSION; }

GQP_API const char *gq_pvq_last_error(void) { return gqp::err_buf; }

GQP_API int gq_pvq_batched_serves(int d, int K, int code_bytes) {
    return ((d == 8 || d == 16 || d == 32) && K >= 32 && K <= 256 && (K & 31) == 0 && code_bytes == 1) ? 1 : 0;
}

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
    if (random_mode != GQ_RANDOM_GIVEN && random_mode != GQ_RANDOM_DEVICE && random_mode != GQ_RANDOM_DEVICE_KEYED &&
        random_mode != GQ_RANDOM_DEVICE_COUNTER)
        return fail(GQ_ERR_INVALID_ARG, "gq_pvq_encode_batched: random_mode must be GIVEN, DEVICE, DEVICE_KEYED or DEVICE_COUNTER (the sampler needs draws)");
    if (random_mode == GQ_RANDOM_GIVEN && !r_flat) return fail(GQ_ERR_INVALID_ARG, "gq_pvq_encode_batched: r_flat is null");
    if (random_mode == GQ_RANDOM_DEVICE_COUNTER && !seed) return fail(GQ_ERR_INVALID_ARG, "gq_pvq_encode_batched: DEVICE_COUNTER needs the address of the { seed, step } words");
    static const double eps = gq::pw_eps_from_env();   // $GQ_PVQ_EPS (tests)
    gqp::PvbArgs a;
    a.seg_table = h->seg_table;
    a.tile_seg = h->tile_seg;
    a.ntiles = h->ntiles;
    a.cdag = b->c_dagger;
    a.wire = wire;
    a.u_flat = h->u_flat;
    a.seg_minmax = h->seg_minmax;
    a.r_flat = r_flat;
    a.seed = seed;
    a.eps = eps;
    a.K = h->K;
    a.random_mode = random_mode;
    a.ef_scale = ef_scale;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const bool ef = ef_scale == ef_scale;
    switch (h->d) {
        case 8: return ef ? gqp::launch<8, true>(a, st) : gqp::launch<8, false>(a, st);
        case 16: return ef ? gqp::launch<16, true>(a, st) : gqp::launch<16, false>(a, st);
        default: return ef ? gqp::launch<32, true>(a, st) : gqp::launch<32, false>(a, st);
    }
}
