// ResidualCompressor (residual_compressor.py:7-32), multi-tensor (segment table) form -- libgq_rq.so (include/gq_rq.h).
//
// A residual tensor travels as two HSQ sections back to back: stage 1's (NearestNeighbor on the gradient) and stage 2's (the
// probabilistic vector compressor on  v - decode(stage 1)).  Stage 1's encode and both level launches are libgq_hsq.so's over
// two descriptors of one tile space.  Here:
//  * rq_encode2_batched_kernel: pw_encode_run (pvq_walk.hpp: a wave owns a RUN of consecutive tiles, the tile encode is
//    pw_encode_tile; libgq_pvq.so's kernel is the same walker over the gradient) over ResidualSource, whose tile is gq_pvq_encode's
//    stage1 form -- v - codebook1[code1] * norm1, product rounded, then the difference -- with code1 and norm1's level read from
//    stage 1's sections of the SAME wire and norm1 de-quantised in the kernel (level_to_norm, gq_common.hpp: the expression the
//    decode kernels evaluate).
//  * rq_decode_sum_kernel: acc = x_0, acc += x_r with x_r = (0 + d1_r) + d2_r rounded first -- torch.stack([d1, d2]).sum(0)
//    per user, then stack(users).mean(0).  Feeding 2R payloads to the HSQ decode would give ((d1_0 + d2_0) + d1_1) + d2_1.
#include <math.h>
#include <stdlib.h>

#include "gq_rq.h"
#include "pvq_walk_host.hpp"

#define GQR_API extern "C" __attribute__((visibility("default")))

namespace gqr {

using namespace gq;

static_assert(sizeof(gq_rq_batch) == 40, "gq_rq_batch: the layout the ctypes binding declares (gq_amd/native.py)");

using gql::err_buf;
using gql::fail;

// Three consumers draw per record: stage 1's level launch (the seed as it is), this encode's sampler (PW_SAMPLER_SALT,
// pvq_walk.hpp) and stage 2's level launch (RQ_LEVEL2_SALT, through level2_words in counter mode, by the caller's own salting
// otherwise).
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
    PwRunArgs run;                  // seg_table: stage 1's (gradient pointers, sizes, stage 1's wire offsets); u_flat, seg_minmax: stage 2's
    const int64_t *seg_table2;      // stage 2's: column 3 = its codes section
    const float *cb1;
    uint64_t *level2_words;
    int level_bytes;
    float inv_s;
};

// A tile of  v - codebook1[code1] * norm1  (pw_residual_quad: gq_pvq_encode's stage1 form), stage 1 read from its sections of
// the wire.  Lane L fetches the code and the level of row L of the tile (two coalesced loads, two registers in flight across
// the tile encode); the lanes that stage a quarter of row r take them from lane r by a wave shuffle.
template <int D>
struct ResidualSource {
    static constexpr int NQ = PwShape<D>::NQ;
    struct Tile : PwTile {
        uintptr_t codes1;   // stage 1: the tile's first code ...
        uintptr_t levels1;  // ... its level section (the whole section: the level is addressed by `local0 + lane`)
        uintptr_t lbub1;    // ... its (lb, ub)
    };
    const int64_t *const seg_table2;
    const uintptr_t cb1;
    const int level_bytes;
    const float inv_s;
    f32x4 pre[NQ];
    uint32_t pre_c1 = 0, pre_lv = 0;      // row `lane` of the tile: stage 1's code and raw level
    float pre_lb = 0.0f, pre_ub = 0.0f;

    __device__ __forceinline__ explicit ResidualSource(const RqEncArgs &a)
        : seg_table2(a.seg_table2), cb1((uintptr_t)a.cb1), level_bytes(a.level_bytes), inv_s(a.inv_s) {}

    __device__ __forceinline__ Tile tile(const PwRunArgs &a, int64_t t) const {
        Tile ti;
        const pw_crec_ptr rec = pw_tile_common<D>(a, t, ti);
        const pw_crec_ptr rec2 = (pw_crec_ptr)(uintptr_t)(seg_table2 + 8 * (int64_t)ti.seg);
        ti.codes1 = (uintptr_t)a.wire + (uintptr_t)(rec[3] + ti.local0);
        ti.levels1 = (uintptr_t)a.wire + (uintptr_t)rec[4];
        ti.lbub1 = (uintptr_t)a.wire + (uintptr_t)rec[5];
        ti.codes = (pw_gcode_ptr)((uintptr_t)a.wire + (uintptr_t)(rec2[3] + ti.local0));
        return ti;
    }
    __device__ __forceinline__ void fetch(const Tile &ti) {
        const int lane = threadIdx.x & 63;
        pw_fetch_rows<D>(pre, ti.grad, ti.left);
        pre_c1 = 0;
        pre_lv = 0;
        if (lane < ti.left) {
            pre_c1 = ((g_u8)ti.codes1)[lane];
            pre_lv = rq_raw_level(ti.levels1, level_bytes, ti.local0 + lane);
        }
        if (level_bytes != 0) {
            pre_lb = ((g_f32)ti.lbub1)[0];
            pre_ub = ((g_f32)ti.lbub1)[1];
        }
    }
    __device__ __forceinline__ void commit(const Tile &ti, float *s_v) {
        const int lane = threadIdx.x & 63;
        const float range = pre_ub - pre_lb;
        const float n_own = lane < ti.left ? rq_norm(pre_lv, level_bytes, pre_lb, range, inv_s) : 0.0f;
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            const int q = i * 64 + lane;
            const int rr = q / NQ;
            const int e0 = (q - rr * NQ) * 4;
            const unsigned c1 = (unsigned)__shfl((int)pre_c1, rr, 64);      // (every lane takes part: rr < 64 always)
            const float n1 = __shfl(n_own, rr, 64);
            f32x4 val = pre[i];
            if (rr < ti.left) pw_residual_quad(val, *(pw_gcv_ptr)(cb1 + ((uintptr_t)c1 * D + (unsigned)e0) * sizeof(float)), n1);
            pw_stage_quad<D>(s_v, rr, e0, val);
        }
    }
};

// Registers (-Rpass-analysis=kernel-resource-usage, profiles/pvq_run_ab.txt; no scratch, no AGPRs): d = 8 runs three waves per
// SIMD.  d = 16 carries stage 1's row (code, level, lb, ub) beside the gradient tile, does not fit three waves' 168 registers
// without spilling and is built for two, as pvq_encode_walk_batched_kernel's error-feedback form is; d = 32 needs its 200+.
template <int D>
__global__ __launch_bounds__(ENC_THREADS) __attribute__((amdgpu_waves_per_eu(D < 16 ? 3 : (D == 16 ? 2 : 1)))) void rq_encode2_batched_kernel(const RqEncArgs a) {
    if (a.run.random_mode == GQ_RANDOM_DEVICE_COUNTER && a.level2_words && blockIdx.x == 0 && threadIdx.x == 0) {
        int random_mode = a.run.random_mode;      // stage 2's level launch: its own stream of this step
        uint64_t seed = a.run.seed;
        resolve_seed(random_mode, seed);
        a.level2_words[0] = seed ^ RQ_LEVEL2_SALT;
        a.level2_words[1] = 0;
    }
    ResidualSource<D> src(a);
    pw_encode_run<D>(a.run, src);
}

template <int D>
static int launch_encode2(const RqEncArgs &a, hipStream_t st) {
    return pw_launch_run<D, rq_encode2_batched_kernel<D>>(a, st, "gq_rq_encode2_batched");
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
    const int64_t cap = (int64_t)gql::cu_count() * 8;
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

GQR_API int gq_rq_batched_serves(int d, int K, int code_bytes) { return gq::pw_run_serves(d, K, code_bytes) ? 1 : 0; }

GQR_API int gq_rq_encode2_batched(const gq_rq_batch *b, uint8_t *wire, int random_mode, uint64_t seed, const float *r_flat, void *stream) {
    using gqr::fail;
    const int rc = gqr::check(b, "gq_rq_encode2_batched");
    if (rc != GQ_OK) return rc;
    const gq_hsq_batch *h1 = b->stage1, *h2 = b->stage2;
    if (!h2->u_flat || !h2->seg_minmax || !b->c_dagger || !wire) return fail(GQ_ERR_INVALID_ARG, "gq_rq_encode2_batched: null pointer");
    if (reinterpret_cast<uintptr_t>(b->c_dagger) & 15) return fail(GQ_ERR_INVALID_ARG, "gq_rq_encode2_batched: c_dagger must be 16-byte aligned");
    const int rcd = gq::pw_check_draws(random_mode, seed, r_flat, "gq_rq_encode2_batched");
    if (rcd != GQ_OK) return rcd;
    static const double eps = gq::pw_eps_from_env();   // $GQ_PVQ_EPS (tests)
    gqr::RqEncArgs a;
    a.run.seg_table = h1->seg_table;
    a.run.tile_seg = h1->tile_seg;
    a.run.ntiles = h1->ntiles;
    a.run.cdag = b->c_dagger;
    a.run.wire = wire;
    a.run.u_flat = h2->u_flat;
    a.run.seg_minmax = h2->seg_minmax;
    a.run.r_flat = r_flat;
    a.run.seed = seed;
    a.run.eps = eps;
    a.run.K = h1->K;
    a.run.random_mode = random_mode;
    a.seg_table2 = h2->seg_table;
    a.cb1 = h1->codebook;
    a.level2_words = b->level2_words;
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
