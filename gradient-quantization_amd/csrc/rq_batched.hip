// ResidualCompressor (residual_compressor.py:7-32), multi-tensor (segment table) form -- libgq_rq.so (include/gq_rq.h).
//
// A residual tensor travels as two HSQ sections back to back: stage 1's (NearestNeighbor on the gradient) and stage 2's (the
// probabilistic vector compressor on  v - decode(stage 1)).  Stage 1's encode and both level launches are libgq_hsq.so's over
// two descriptors of one tile space.  Here:
//  * rq_encode2_batched_kernel: pvq_encode_walk_batched_kernel's walk (pvq_batched.hip: a wave owns a RUN of consecutive
//    tiles, the tile encode is pw_encode_tile of pvq_walk.hpp) whose tile staging is gq_pvq_encode's stage1 form -- the tile is
//    v - codebook1[code1] * norm1, product rounded, then the difference -- with code1 and norm1's level read from stage 1's
//    sections of the SAME wire and norm1 de-quantised in the kernel (level_to_norm, gq_common.hpp: the expression the decode
//    kernels evaluate).  Lane L fetches the code and the level of row L of the tile (two coalesced loads, two registers in
//    flight across the tile encode); the lanes that stage a quarter of row r take them from lane r by a wave shuffle.
//  * rq_decode_sum_kernel: acc = x_0, acc += x_r with x_r = (0 + d1_r) + d2_r rounded first -- torch.stack([d1, d2]).sum(0)
//    per user, then stack(users).mean(0).  Feeding 2R payloads to the HSQ decode would give ((d1_0 + d2_0) + d1_1) + d2_1.
#include <math.h>
#include <stdlib.h>

#include "gq_lib_prelude.hpp"
#include "gq_rq.h"
#include "hsq_pf_common.hpp"
#include "pvq_walk.hpp"

#define GQR_API extern "C" __attribute__((visibility("default")))

namespace gqr {

using namespace gq;

static_assert(sizeof(gq_rq_batch) == 40, "gq_rq_batch: the layout the ctypes binding declares (gq_amd/native.py)");

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

// Three consumers draw per record: stage 1's level launch (the seed as it is), this encode's sampler (RQ_CODE_SALT) and stage
// 2's level launch (RQ_LEVEL2_SALT, through level2_words in counter mode, by the caller's own salting otherwise).
constexpr uint64_t RQ_CODE_SALT = 0xA0761D6478BD642Full;      // (the sampler's salt of libgq_pvq.so)
constexpr uint64_t RQ_LEVEL2_SALT = 0xE7037ED1A0B428DBull;

typedef const uint8_t __attribute__((address_space(1))) *g_u8;
typedef const uint16_t __attribute__((address_space(1))) *g_u16;
typedef const uint32_t __attribute__((address_space(1))) *g_u32;
typedef const float __attribute__((address_space(1))) *g_f32;

// the raw level word of subvector `local` of a level section at byte address `sec` (level_bytes: 0 = f32 bits, 1, 2, 4)
__device__ __forceinline__ uint32_t rq_raw_level(uintptr_t sec, int level_bytes, int64_t local) {
    switch (level_bytes) {
        case 1: return ((g_u8)sec)[local];
        case 2: return ((g_u16)sec)[local];
        default: return ((g_u32)sec)[local];      // int32 levels, or the f32 projection's bits
    }
}
// ... and its norm: probabilistic_scalar_compressor.py:31-32 through level_to_norm
__device__ __forceinline__ float rq_norm(uint32_t raw, int level_bytes, float lb, float range, float inv_s) {
    if (level_bytes == 0) return level_to_norm<float>(__uint_as_float(raw), lb, range, inv_s);
    return level_to_norm<unsigned>(raw, lb, range, inv_s);
}

struct RqEncArgs {
    const int64_t *seg_table;       // stage 1's: gradient pointers, sizes, stage 1's wire offsets
    const int64_t *seg_table2;      // stage 2's: column 3 = its codes section
    const int32_t *tile_seg;
    int64_t ntiles;
    const float *cdag;
    const float *cb1;
    uint8_t *wire;
    float *u_flat;
    unsigned *seg_minmax;
    const float *r_flat;
    uint64_t *level2_words;
    uint64_t seed;
    double eps;
    int K, random_mode, level_bytes;
    float inv_s;
    int tiles_per_wave, waves_with_one_more;      // a wave's RUN of consecutive tiles (pvq_batched.hip)
};

// Registers (-Rpass-analysis=kernel-resource-usage): d = 8 at three waves per SIMD and d = 32 with its 200+, as
// pvq_encode_walk_batched_kernel.  d = 16 carries stage 1's row (code, level, lb, ub) beside the gradient tile and spills at
// three waves (168 VGPRs + 84 bytes of scratch): it is built for two, as that kernel's error-feedback form is.  No scratch.
template <int D>
__global__ __launch_bounds__(ENC_THREADS) __attribute__((amdgpu_waves_per_eu(D < 16 ? 3 : (D == 16 ? 2 : 1)))) void rq_encode2_batched_kernel(const RqEncArgs a) {
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
    const bool counter = random_mode == GQ_RANDOM_DEVICE_COUNTER;
    resolve_seed(random_mode, seed);       // GQ_RANDOM_DEVICE_COUNTER: { seed, step } words -> this launch's seed
    if (counter && a.level2_words && blockIdx.x == 0 && threadIdx.x == 0) {      // stage 2's level launch: its own stream of this step
        a.level2_words[0] = seed ^ RQ_LEVEL2_SALT;
        a.level2_words[1] = 0;
    }
    seed ^= RQ_CODE_SALT;
    pw_stage_codebook<D>(a.cdag, a.K, s_cb);
    __syncthreads();

    // (global pointers and scalar table loads: see pvq_batched.hip)
    typedef const f32x4 __attribute__((address_space(1))) *gcv_ptr;
    typedef uint8_t __attribute__((address_space(1))) *gcode_ptr;
    typedef float __attribute__((address_space(1))) *gf_ptr;
    typedef unsigned __attribute__((address_space(1))) *gu_ptr;
    const gf_ptr u_flat = (gf_ptr)(uintptr_t)a.u_flat;
    const g_f32 r_flat = (g_f32)(uintptr_t)a.r_flat;
    const gu_ptr seg_minmax = (gu_ptr)(uintptr_t)a.seg_minmax;
    const uintptr_t cb1 = (uintptr_t)a.cb1;
    typedef const int64_t __attribute__((address_space(4))) *crec_ptr;
    typedef const int32_t __attribute__((address_space(4))) *cseg_ptr;
    struct Tile {
        uintptr_t grad;     // the tile's first float
        uintptr_t codes1;   // stage 1: the tile's first code ...
        uintptr_t levels1;  // ... its level section (the whole section: the level is addressed by `local0 + lane`)
        uintptr_t lbub1;    // ... its (lb, ub)
        gcode_ptr codes2;   // stage 2: the tile's first code in the wire
        int64_t local0;     // the tile's first subvector within its tensor
        int left;           // subvectors of the tensor from the tile's start on, capped at 64
        int seg;
    };
    auto tile_info = [&](int64_t t) {
        Tile ti;
        ti.seg = ((cseg_ptr)(uintptr_t)a.tile_seg)[t];
        const crec_ptr rec = (crec_ptr)(uintptr_t)(a.seg_table + 8 * (int64_t)ti.seg);
        const crec_ptr rec2 = (crec_ptr)(uintptr_t)(a.seg_table2 + 8 * (int64_t)ti.seg);
        const int64_t local0 = (t - rec[2]) * 64;
        const int64_t left = rec[1] - local0;
        ti.local0 = local0;
        ti.left = left < 64 ? (int)left : 64;
        ti.grad = (uintptr_t)rec[0] + (uintptr_t)local0 * (D * sizeof(float));
        ti.codes1 = (uintptr_t)a.wire + (uintptr_t)(rec[3] + local0);
        ti.levels1 = (uintptr_t)a.wire + (uintptr_t)rec[4];
        ti.lbub1 = (uintptr_t)a.wire + (uintptr_t)rec[5];
        ti.codes2 = (gcode_ptr)((uintptr_t)a.wire + (uintptr_t)(rec2[3] + local0));
        return ti;
    };
    f32x4 pre[NQ];
    uint32_t pre_c1 = 0, pre_lv = 0;      // row `lane` of the tile: stage 1's code and raw level
    float pre_lb = 0.0f, pre_ub = 0.0f;
    auto fetch_tile = [&](const Tile &ti) {
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            const int q = i * 64 + lane;
            const int rr = q / NQ;
            const unsigned off = (unsigned)q * 16u;      // float4 q of the tile: row q / NQ, elements 4 (q mod NQ) ...
            pre[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if (rr < ti.left) pre[i] = *(gcv_ptr)(ti.grad + off);
        }
        pre_c1 = 0;
        pre_lv = 0;
        if (lane < ti.left) {
            pre_c1 = ((g_u8)ti.codes1)[lane];
            pre_lv = rq_raw_level(ti.levels1, a.level_bytes, ti.local0 + lane);
        }
        if (a.level_bytes != 0) {
            pre_lb = ((g_f32)ti.lbub1)[0];
            pre_ub = ((g_f32)ti.lbub1)[1];
        }
    };
    auto commit_tile = [&](const Tile &ti) {
        const float range = pre_ub - pre_lb;
        const float n_own = lane < ti.left ? rq_norm(pre_lv, a.level_bytes, pre_lb, range, a.inv_s) : 0.0f;
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            const int q = i * 64 + lane;
            const int rr = q / NQ;
            const int e0 = (q - rr * NQ) * 4;
            const unsigned c1 = (unsigned)__shfl((int)pre_c1, rr, 64);      // (every lane takes part: rr < 64 always)
            const float n1 = __shfl(n_own, rr, 64);
            f32x4 val = pre[i];
            if (rr < ti.left) {
                const f32x4 c = *(gcv_ptr)(cb1 + ((uintptr_t)c1 * D + (unsigned)e0) * sizeof(float));
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float dec = c[e] * n1;   // stage 1's decoded element (product rounded)
                    val[e] = val[e] - dec;         // residuals -= decompressed (residual_compressor.py:22)
                }
            }
            pw_stage_quad<D>(s_v, rr, e0, val);
        }
    };
    float lmin = INFINITY, lmax = -INFINITY;
    int cur_seg = -1;
    // the wave's running (min, max) into its tensor's words (look before the atomic: pvq_batched.hip)
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
    // A wave takes a RUN of consecutive tiles, not tiles one grid apart: see pvq_batched.hip (1.31x, profiles/pvq_encode_grid_stride.jsonl)
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
            cur.codes2[lane] = (uint8_t)code;
            u_flat[idx] = val;
            lmin = fminf(lmin, val);
            lmax = fmaxf(lmax, val);
        }
        cur = nxt;
    }
    flush_minmax();
}

template <int D>
static int launch_encode2(const RqEncArgs &a, hipStream_t st) {
    constexpr size_t lds_bytes = PwShape<D>::LDS_BYTES;
    static const int bpc = [] {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(rq_encode2_batched_kernel<D>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
        (void)hipGetLastError();
        return resident_blocks_per_cu(rq_encode2_batched_kernel<D>, ENC_THREADS, lds_bytes);
    }();
    int64_t blocks = (a.ntiles + ENC_WAVES - 1) / ENC_WAVES;
    const int64_t cap = (int64_t)cu_count_here() * bpc;      // one resident wave of workgroups: none queues behind another
    if (blocks > cap) blocks = cap;
    RqEncArgs b = a;
    const int64_t waves = blocks * ENC_WAVES;
    b.tiles_per_wave = (int)(a.ntiles / waves);
    b.waves_with_one_more = (int)(a.ntiles - (int64_t)b.tiles_per_wave * waves);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(rq_encode2_batched_kernel<D>), dim3((unsigned)blocks), dim3(ENC_THREADS), lds_bytes, st, b);
    GQL_CHECK_LAUNCH("gq_rq_encode2_batched");
    return GQ_OK;
}

// ---- decode-mean ---------------------------------------------------------------------------------------------------------
constexpr int DEC_THREADS = 256;

// LDS row stride (floats) of a staged codebook: an odd number of 16-byte units per row (hsq_decode.hip: cb_row_stride)
__host__ __device__ constexpr int rq_row_stride(int d) { return ((d >> 2) & 1) ? d : d + 4; }

struct RqDecArgs {
    const int64_t *seg_table;       // stage 1's (columns 0 / 7: gradient / error buffer for ERR; 6: float offset in `out`)
    const int64_t *seg_table2;
    const int32_t *tile_seg;
    int64_t ntiles;
    const uint8_t *gathered;
    int64_t user_stride;
    const float *cb1, *cb2;         // cb2 == cb1: one image serves both stages
    float *out;
    int R, K, level_bytes, plain;
    float inv_s;
};

// A thread owns four consecutive floats of one subvector; a workgroup walks chunks of DEC_THREADS / (D / 4) padded subvector
// slots.  Per payload: the two stages' codes and norms, two codebook rows out of LDS, x = (0 + d1) + d2.
template <int D, bool ERR>
__global__ __launch_bounds__(DEC_THREADS) void rq_decode_sum_kernel(const RqDecArgs a) {
    constexpr int UPS = D / 4, SLOTS = DEC_THREADS / UPS, RS = rq_row_stride(D);
    extern __shared__ __attribute__((aligned(16))) float s_cb[];
    const bool shared_cb = a.cb1 == a.cb2;
    for (int i = threadIdx.x; i < a.K * UPS; i += DEC_THREADS) {
        const int row = i / UPS, p = i - row * UPS;
        *reinterpret_cast<f32x4 *>(s_cb + row * RS + 4 * p) = *reinterpret_cast<const f32x4 *>(a.cb1 + (int64_t)row * D + 4 * p);
        if (!shared_cb)
            *reinterpret_cast<f32x4 *>(s_cb + (a.K + row) * RS + 4 * p) = *reinterpret_cast<const f32x4 *>(a.cb2 + (int64_t)row * D + 4 * p);
    }
    __syncthreads();
    const float *const s_cb2 = shared_cb ? s_cb : s_cb + a.K * RS;
    const MeanDiv md = mean_div_of(a.R, !ERR && !a.plain);
    const int sub = threadIdx.x / UPS, q = threadIdx.x - sub * UPS;
    const int64_t nslots = a.ntiles * 64;
    for (int64_t slot = (int64_t)blockIdx.x * SLOTS + sub; slot < nslots; slot += (int64_t)gridDim.x * SLOTS) {
        const int64_t tile = slot >> 6;
        const int seg = a.tile_seg[tile];
        const int64_t *rec = a.seg_table + 8 * (int64_t)seg;
        const int64_t *rec2 = a.seg_table2 + 8 * (int64_t)seg;
        const int64_t local = (tile - rec[2]) * 64 + (slot & 63);
        if (local >= rec[1]) continue;
        float *dst = ERR ? reinterpret_cast<float *>(rec[7]) : a.out + rec[6];
        if (ERR && !dst) continue;
        f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int r = 0; r < a.R; ++r) {
            const uintptr_t p = (uintptr_t)a.gathered + (uintptr_t)((int64_t)r * a.user_stride);
            float lb1 = 0.0f, rg1 = 0.0f, lb2 = 0.0f, rg2 = 0.0f;
            if (a.level_bytes != 0) {
                const g_f32 b1 = (g_f32)(p + rec[5]), b2 = (g_f32)(p + rec2[5]);
                lb1 = b1[0];
                rg1 = b1[1] - lb1;
                lb2 = b2[0];
                rg2 = b2[1] - lb2;
            }
            const float n1 = rq_norm(rq_raw_level(p + rec[4], a.level_bytes, local), a.level_bytes, lb1, rg1, a.inv_s);
            const float n2 = rq_norm(rq_raw_level(p + rec2[4], a.level_bytes, local), a.level_bytes, lb2, rg2, a.inv_s);
            const unsigned c1 = ((g_u8)(p + rec[3]))[local], c2 = ((g_u8)(p + rec2[3]))[local];
            const f32x4 r1 = *reinterpret_cast<const f32x4 *>(s_cb + c1 * RS + 4 * q);
            const f32x4 r2 = *reinterpret_cast<const f32x4 *>(s_cb2 + c2 * RS + 4 * q);
            f32x4 x;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d1 = r1[e] * n1, d2 = r2[e] * n2;      // each stage's decode: gather x norm, the product rounded
                x[e] = (0.0f + d1) + d2;                           // torch.stack([d1, d2]).sum(0): from +0, so -0 + -0 is +0
            }
            if (r == 0) {
                acc = x;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] = acc[e] + x[e];
            }
        }
        if (md.apply) acc = mean_div(acc, md);
        const int64_t at = local * D + 4 * q;
        if (ERR) {
            const f32x4 v = *reinterpret_cast<const f32x4 *>(reinterpret_cast<const float *>(rec[0]) + at);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = v[e] - acc[e];      // error = v - decoded (ps_quantizer.py:39)
        }
        *reinterpret_cast<f32x4 *>(dst + at) = acc;
    }
}

template <int D, bool ERR>
static int launch_decode(const RqDecArgs &a, hipStream_t st) {
    constexpr int SLOTS = DEC_THREADS / (D / 4);
    const size_t lds_bytes = (size_t)(a.cb1 == a.cb2 ? 1 : 2) * a.K * rq_row_stride(D) * sizeof(float);
    static const bool attr = [] {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(rq_decode_sum_kernel<D, ERR>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
        (void)hipGetLastError();
        return true;
    }();
    (void)attr;
    int64_t blocks = (a.ntiles * 64 + SLOTS - 1) / SLOTS;
    const int64_t cap = (int64_t)cu_count_here() * 8;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(rq_decode_sum_kernel<D, ERR>), dim3((unsigned)blocks), dim3(DEC_THREADS), lds_bytes, st, a);
    GQL_CHECK_LAUNCH("gq_rq_decode_sum_batched");
    return GQ_OK;
}

// what both entry points require of the descriptor pair
static int check(const gq_rq_batch *b, const char *what) {
    if (!b || b->struct_bytes != sizeof(gq_rq_batch)) return fail(GQ_ERR_INVALID_ARG, "%s: gq_rq_batch of another layout", what);
    const gq_hsq_batch *h1 = b->stage1, *h2 = b->stage2;
    if (!h1 || !h2 || h1->struct_bytes != sizeof(gq_hsq_batch) || h2->struct_bytes != sizeof(gq_hsq_batch))
        return fail(GQ_ERR_INVALID_ARG, "%s: gq_hsq_batch of another layout", what);
    if (h1->d != h2->d || h1->K != h2->K || h1->code_bytes != h2->code_bytes || h1->level_bytes != h2->level_bytes ||
        (h1->n_bit & 0xFF) != (h2->n_bit & 0xFF) || h1->nseg != h2->nseg || h1->ntiles != h2->ntiles || h1->tile_seg != h2->tile_seg)
        return fail(GQ_ERR_INVALID_ARG, "%s: the two stages must share shape, widths and tile space", what);
    if (!gq_rq_batched_serves(h1->d, h1->K, h1->code_bytes))
        return fail(GQ_ERR_UNSUPPORTED, "%s: d = %d, K = %d, %d-byte codes (served: d in {8, 16, 32}, K = 32 ... 256 in whole blocks of 32, "
                                        "byte codes)", what, h1->d, h1->K, h1->code_bytes);
    const int lb = h1->level_bytes, nb = h1->n_bit & 0xFF;
    if (lb != 0 && lb != 1 && lb != 2 && lb != 4)
        return fail(GQ_ERR_UNSUPPORTED, "%s: level_bytes must be 0 (f32 projections), 1, 2 or 4 (packed levels are not read here)", what);
    if (lb != 0 && (nb < 1 || nb > 30)) return fail(GQ_ERR_INVALID_ARG, "%s: n_bit = %d", what, nb);
    if (h1->nseg < 1 || h1->ntiles < 1) return fail(GQ_ERR_INVALID_ARG, "%s: bad sizes", what);
    if (!h1->seg_table || !h2->seg_table || !h1->tile_seg || !h1->codebook || !h2->codebook)
        return fail(GQ_ERR_INVALID_ARG, "%s: null pointer in a descriptor", what);
    if ((reinterpret_cast<uintptr_t>(h1->codebook) | reinterpret_cast<uintptr_t>(h2->codebook)) & 15)
        return fail(GQ_ERR_INVALID_ARG, "%s: the codebooks must be 16-byte aligned", what);
    return GQ_OK;
}

static float inv_s_of(const gq_hsq_batch *h) { return h->level_bytes == 0 ? 1.0f : 1.0f / (float)(1u << (h->n_bit & 31)); }

}  // namespace gqr

GQR_API int gq_rq_abi_version(void) { return GQ_RQ_ABI_VERSION; }

GQR_API const char *gq_rq_last_error(void) { return gqr::err_buf; }

GQR_API int gq_rq_batched_serves(int d, int K, int code_bytes) {
    return ((d == 8 || d == 16 || d == 32) && K >= 32 && K <= 256 && (K & 31) == 0 && code_bytes == 1) ? 1 : 0;
}

GQR_API int gq_rq_encode2_batched(const gq_rq_batch *b, uint8_t *wire, int random_mode, uint64_t seed, const float *r_flat, void *stream) {
    using gqr::fail;
    const int rc = gqr::check(b, "gq_rq_encode2_batched");
    if (rc != GQ_OK) return rc;
    const gq_hsq_batch *h1 = b->stage1, *h2 = b->stage2;
    if (!h2->u_flat || !h2->seg_minmax || !b->c_dagger || !wire) return fail(GQ_ERR_INVALID_ARG, "gq_rq_encode2_batched: null pointer");
    if (reinterpret_cast<uintptr_t>(b->c_dagger) & 15) return fail(GQ_ERR_INVALID_ARG, "gq_rq_encode2_batched: c_dagger must be 16-byte aligned");
    if (random_mode != GQ_RANDOM_GIVEN && random_mode != GQ_RANDOM_DEVICE && random_mode != GQ_RANDOM_DEVICE_KEYED &&
        random_mode != GQ_RANDOM_DEVICE_COUNTER)
        return fail(GQ_ERR_INVALID_ARG, "gq_rq_encode2_batched: random_mode must be GIVEN, DEVICE, DEVICE_KEYED or DEVICE_COUNTER (the sampler needs draws)");
    if (random_mode == GQ_RANDOM_GIVEN && !r_flat) return fail(GQ_ERR_INVALID_ARG, "gq_rq_encode2_batched: r_flat is null");
    if (random_mode == GQ_RANDOM_DEVICE_COUNTER && (!seed || (seed & 7)))
        return fail(GQ_ERR_INVALID_ARG, "gq_rq_encode2_batched: DEVICE_COUNTER needs the address of the { seed, step } words");
    static const double eps = gq::pw_eps_from_env();   // $GQ_PVQ_EPS (tests)
    gqr::RqEncArgs a;
    a.seg_table = h1->seg_table;
    a.seg_table2 = h2->seg_table;
    a.tile_seg = h1->tile_seg;
    a.ntiles = h1->ntiles;
    a.cdag = b->c_dagger;
    a.cb1 = h1->codebook;
    a.wire = wire;
    a.u_flat = h2->u_flat;
    a.seg_minmax = h2->seg_minmax;
    a.r_flat = r_flat;
    a.level2_words = b->level2_words;
    a.seed = seed;
    a.eps = eps;
    a.K = h1->K;
    a.random_mode = random_mode;
    a.level_bytes = h1->level_bytes;
    a.inv_s = gqr::inv_s_of(h1);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    switch (h1->d) {
        case 8: return gqr::launch_encode2<8>(a, st);
        case 16: return gqr::launch_encode2<16>(a, st);
        default: return gqr::launch_encode2<32>(a, st);
    }
}

GQR_API int gq_rq_decode_sum_batched(const gq_rq_batch *b, const uint8_t *gathered, int64_t user_stride_bytes, int R, float *out,
                                     int mode, void *stream) {
    using gqr::fail;
    const int rc = gqr::check(b, "gq_rq_decode_sum_batched");
    if (rc != GQ_OK) return rc;
    if (mode != GQ_RQ_MEAN && mode != GQ_RQ_PLAIN && mode != GQ_RQ_ERROR) return fail(GQ_ERR_INVALID_ARG, "gq_rq_decode_sum_batched: mode %d", mode);
    if (R < 1 || (mode != GQ_RQ_MEAN && R != 1)) return fail(GQ_ERR_INVALID_ARG, "gq_rq_decode_sum_batched: R = %d (PLAIN and ERROR decode one payload)", R);
    if (!gathered || (mode != GQ_RQ_ERROR && !out)) return fail(GQ_ERR_INVALID_ARG, "gq_rq_decode_sum_batched: null pointer");
    const gq_hsq_batch *h1 = b->stage1, *h2 = b->stage2;
    gqr::RqDecArgs a;
    a.seg_table = h1->seg_table;
    a.seg_table2 = h2->seg_table;
    a.tile_seg = h1->tile_seg;
    a.ntiles = h1->ntiles;
    a.gathered = gathered;
    a.user_stride = user_stride_bytes;
    a.cb1 = h1->codebook;
    a.cb2 = h2->codebook;
    a.out = out;
    a.R = R;
    a.K = h1->K;
    a.level_bytes = h1->level_bytes;
    a.plain = mode == GQ_RQ_PLAIN ? 1 : 0;
    a.inv_s = gqr::inv_s_of(h1);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const bool err = mode == GQ_RQ_ERROR;
    switch (h1->d) {
        case 8: return err ? gqr::launch_decode<8, true>(a, st) : gqr::launch_decode<8, false>(a, st);
        case 16: return err ? gqr::launch_decode<16, true>(a, st) : gqr::launch_decode<16, false>(a, st);
        default: return err ? gqr::launch_decode<32, true>(a, st) : gqr::launch_decode<32, false>(a, st);
    }
}
