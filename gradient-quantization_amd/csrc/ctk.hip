// Chunked top-k, multi-tensor (segment table) form -- libgq_ctk.so (include/gq_ctk.h).  One launch each way, a workgroup per item.
//
// compress   The item's 4,096 values sit in registers, sixteen a lane: register step s of thread t is the float4 at elements
//            1024 s + 4 t, so every load and store of the gradient, the residual and the dense decode is one coalesced 16-byte
//            access.  Element order is therefore (step, thread, slot in the float4), and everything that ranks elements -- the tie
//            rule, the compaction -- scans in that order: four packed wave scans, their totals through LDS, the steps chained.
//   select   a radix select over the 31-bit key, 8 + 8 + 8 + 7 bits from the top, in a 256-bin LDS histogram (integer LDS adds:
//            the counts do not depend on their order).  Wave 0 walks the bins from the top, four a lane, fixes the digit and the
//            remaining rank and clears the bins it read; every lane then counts only keys that match the prefix.  The result is
//            the threshold key T and `need`, the ties to keep.  An element past the item's end enters as key 0 at the highest
//            indices: it can only swell the lowest bin below everything the select looks for, and as a tie it ranks behind every
//            real one, of which there are at least `need`.
//   compact  per lane and step #(key > T) | #(key == T) << 16 (an item has 4,096 elements: neither half overflows), an
//            exclusive scan in element order; a kept element's slot is the kept elements before it.  pos and value are staged
//            in LDS (2,048 entries at cr = 2: 12 KB) and leave as contiguous 16-byte stores; a 16-byte group that two items
//            share is written by element, each item its own.  The tensor's last item writes the pads.
// decode     a tile of 4,096 floats in LDS, +0; the payloads in order with a barrier between them, each lane adding its pairs
//            into tile[pos] (positions inside one payload are distinct); then the division and float4 stores.
// PACKED16   the second value format, further instantiations of the same two kernels: the compress also reduces the item's largest
//            key H (a wave reduction, four partials through LDS behind the compaction's barrier), gives every kept element one of
//            eight levels between T and H (struct Levels) and stages 16-bit words alone; one lane writes the item's { T, H }.  The
//            decode rebuilds every magnitude from the payload's { T, H } of the item.
// Both launches' arguments depend on the layout alone: they replay from a HIP graph.  No global scratch, no global atomics.
#include <math.h>

#include "gq_ctk.h"
#include "gq_lib_prelude.hpp"
#include "sparse_kernels.hpp"

#define GQC_API extern "C" __attribute__((visibility("default")))

namespace gqc {

using gql::aligned16;
using gql::copy_dense;
using gql::err_buf;
using gql::fail;
using gqsp::key_of;
using gqsp::NO_KEY;
using gqsp::THREADS;
using gqsp::WAVES;

constexpr int CHUNK = GQ_CTK_CHUNK;
constexpr int RUN = 4;                              // elements of a lane's float4
constexpr int STEPS = CHUNK / (THREADS * RUN);      // register steps
constexpr int STEP_ELEMS = THREADS * RUN;           // elements the workgroup covers in one step
constexpr int BINS = 256;
constexpr int MAX_KEPT = CHUNK / GQ_CTK_MIN_CR;     // an item's kept elements at the smallest cr
static_assert(CHUNK == 4096 && THREADS == 256 && STEPS == 4 && BINS == THREADS, "an item is four float4 a lane; a bin a thread");
static_assert(BINS == 4 * 64, "wave 0 walks the bins four a lane");
static_assert(sizeof(gq_ctk_batch) == 48, "gq_ctk_batch: the layout the ctypes binding declares (gq_amd/native.py)");

// pass p of the in-workgroup select: the key bits [shift, shift + nb).  Its own digits, four of them for 256 bins -- not the
// 11 / 11 / 9 of sparse_kernels.hpp's pass_shift / pass_bits, hence other names
__device__ constexpr int digit_shift(int p) { return p == 0 ? 23 : (p == 1 ? 15 : (p == 2 ? 7 : 0)); }
__device__ constexpr int digit_bits(int p) { return p == 3 ? 7 : 8; }

__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t x) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    return x;
}

// what every kernel knows about its item
struct Item {
    const int64_t *rec;
    int64_t base;              // the item's first element in its tensor
    uint32_t len, kt, e0, K;   // elements, kept elements, the first of its entries in the section, the tensor's entries
    bool last;
    __device__ __forceinline__ Item(const int64_t *seg_table, const int32_t *item_seg, int cr) {
        const int64_t item = blockIdx.x;
        rec = seg_table + 8 * (int64_t)item_seg[item];
        const int64_t n = rec[1], t = item - rec[2];
        base = t * CHUNK;
        last = base + CHUNK >= n;
        len = (uint32_t)(last ? n - base : CHUNK);
        const uint32_t kf = (uint32_t)(CHUNK / cr);
        kt = len / (uint32_t)cr;
        e0 = (uint32_t)t * kf;
        K = (uint32_t)GQ_CTK_KEPT(n, cr);
    }
    __device__ __forceinline__ int64_t value_offset() const { return rec[3] + ((2 * (int64_t)K + 15) & ~(int64_t)15); }
    // PACKED16: the tensor's items; this item's bounds; the words behind the padded bounds of all of them
    __device__ __forceinline__ int64_t items() const { return (rec[1] + CHUNK - 1) / CHUNK; }
    __device__ __forceinline__ int64_t bounds_offset() const { return rec[3] + 8 * (base / CHUNK); }
    __device__ __forceinline__ int64_t word_offset() const { return rec[3] + ((8 * items() + 15) & ~(int64_t)15); }
};

// PACKED16 (include/gq_ctk.h): the eight magnitudes of an item, evenly spaced in key space between its bounds T and H.  D = H - T
// in uint32 arithmetic, so a decode of foreign bytes with H < T computes something defined.  Both formulas without a division by D
// and without 64-bit products but the compares of `level`.
struct Levels {
    uint32_t T, D, qd, rd;
    __device__ __forceinline__ Levels(uint32_t T_, uint32_t H) : T(T_), D(H - T_), qd((H - T_) / 7u), rd((H - T_) % 7u) {}
    // ((k - T) * 14 + D) / (2 D): the number of j = 1 ... 7 with (2 j - 1) D <= 14 (k - T)  (T <= k <= H: never more than 7)
    __device__ __forceinline__ uint32_t level(uint32_t k) const {
        if (D == 0u) return 0u;
        const uint64_t x = (uint64_t)(k - T) * 14u;
        uint32_t l = 0;
#pragma unroll
        for (uint32_t j = 1; j <= 7; ++j) l += x >= (uint64_t)(2u * j - 1u) * D ? 1u : 0u;
        return l;
    }
    // T + (l D + 3) / 7 with D = 7 qd + rd: l qd + (l rd + 3) / 7, and x / 7 = x * 37 >> 8 for every x <= 45 = 7 * 6 + 3
    __device__ __forceinline__ uint32_t key(uint32_t l) const { return T + l * qd + (((l * rd + 3u) * 37u) >> 8); }
};

// a lane's four elements at e of the item: one 16-byte load where the view is aligned and the run inside the item, else by
// element, +0 past the end
__device__ __forceinline__ void load_run(const float *__restrict__ p, uint32_t e, uint32_t len, bool vec, float (&x)[RUN]) {
    if (vec && e + RUN <= len) {
        const float4 a = *reinterpret_cast<const float4 *>(p + e);
        x[0] = a.x, x[1] = a.y, x[2] = a.z, x[3] = a.w;
    } else {
#pragma unroll
        for (int j = 0; j < RUN; ++j) x[j] = e + j < len ? p[e + j] : 0.0f;
    }
}

__device__ __forceinline__ void store_run(float *__restrict__ p, uint32_t e, uint32_t len, bool vec, const float (&x)[RUN]) {
    if (vec && e + RUN <= len) {
        *reinterpret_cast<float4 *>(p + e) = make_float4(x[0], x[1], x[2], x[3]);
    } else {
#pragma unroll
        for (int j = 0; j < RUN; ++j)
            if (e + j < len) p[e + j] = x[j];
    }
}

// The item's entries e0 ... e0 + cnt - 1 of a section array `g` (16-byte aligned at entry 0), from LDS, and zeros up to `end`
// (the tensor's last item: the pad).  Sixteen bytes a store where the whole group is this item's, by element where it is not.
template <class T>
__device__ __forceinline__ void store_entries(T *__restrict__ g, const T *staged, uint32_t e0, uint32_t cnt, uint32_t end) {
    constexpr uint32_t PER = 16 / sizeof(T);
    for (uint32_t lo = (e0 / PER + threadIdx.x) * PER; lo < end; lo += THREADS * PER) {
        T x[PER];
#pragma unroll
        for (uint32_t j = 0; j < PER; ++j) {
            const uint32_t at = lo + j - e0;      // (wraps below e0: not below cnt)
            x[j] = at < cnt ? staged[at] : (T)0;
        }
        if (lo >= e0 && lo + PER <= end) {
            uint4 q;
            __builtin_memcpy(&q, x, 16);
            *reinterpret_cast<uint4 *>(g + lo) = q;
        } else {
#pragma unroll
            for (uint32_t j = 0; j < PER; ++j)
                if (lo + j >= e0 && lo + j < end) g[lo + j] = x[j];
        }
    }
}

// PACKED: the PACKED16 section -- a 16-bit word  pos | level << 12 | sign << 15  per kept element behind the items' { T, H }
template <bool EF, bool PACKED>
__global__ __launch_bounds__(THREADS) void ctk_compress_kernel(const int64_t *__restrict__ seg_table, const int32_t *__restrict__ item_seg,
                                                               uint8_t *__restrict__ wire, float *__restrict__ out, float ef_scale, int cr,
                                                               const int64_t *__restrict__ dense_table, int ndense) {
    copy_dense<THREADS>(dense_table, ndense, wire);
    __shared__ uint32_t hist[BINS];
    __shared__ uint32_t picked[2];                  // the pass's prefix and remaining rank
    __shared__ uint32_t totals[STEPS][WAVES];
    __shared__ __align__(16) float sval[PACKED ? RUN : MAX_KEPT];      // (PACKED stages words alone: 8 KB less)
    __shared__ __align__(16) uint16_t spos[MAX_KEPT];
    __shared__ uint32_t wave_max[WAVES];            // PACKED: the waves' largest keys
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const Item it(seg_table, item_seg, cr);
    float *v = reinterpret_cast<float *>(it.rec[0]) + it.base;
    float *err = EF && it.rec[7] ? reinterpret_cast<float *>(it.rec[7]) + it.base : nullptr;
    float *o = out ? out + it.rec[5] + it.base : nullptr;
    const bool vec_in = aligned16(v) && aligned16(err), vec_o = aligned16(o);      // (a null err counts as aligned)

    hist[tid] = 0u;
    float w[STEPS][RUN];
    uint32_t key[STEPS][RUN];
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
        const uint32_t e = (uint32_t)(s * STEP_ELEMS + RUN * tid);
        load_run(v, e, it.len, vec_in, w[s]);
        if (EF && err) {
            float r[RUN];
            load_run(err, e, it.len, vec_in, r);
#pragma unroll
            for (int j = 0; j < RUN; ++j) {
                const float p = ef_scale * r[j];      // (-ffp-contract=off: the product rounded, then the sum)
                w[s][j] = w[s][j] + p;
            }
        }
#pragma unroll
        for (int j = 0; j < RUN; ++j) key[s][j] = key_of(w[s][j]);
    }
    __syncthreads();

    // ---- the select: T = the kt-th largest key, need = how many keys == T are kept
    uint32_t T = NO_KEY, need = 0;
    if (it.kt != 0) {      // (the same for the whole workgroup)
        uint32_t prefix = 0, kr = it.kt;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            constexpr uint32_t ALL = 0xffffffffu;
            const int shift = digit_shift(p), hi = shift + digit_bits(p);
            const uint32_t mask = ~(ALL << digit_bits(p));
#pragma unroll
            for (int s = 0; s < STEPS; ++s) {
#pragma unroll
                for (int j = 0; j < RUN; ++j) {
                    const uint32_t k = key[s][j];
                    if ((k >> hi) == (prefix >> hi)) atomicAdd(&hist[(k >> shift) & mask], 1u);
                }
            }
            __syncthreads();
            if (wv == 0) {      // lane l: bins 255 - 4 l downwards, the highest first; it clears what it read
                uint32_t c[4], sum = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int b = BINS - 1 - 4 * lane - j;
                    c[j] = hist[b];
                    hist[b] = 0u;
                    sum += c[j];
                }
                const uint32_t incl = wave_inclusive_scan(sum);
                uint32_t cum = incl - sum;
                if (cum < kr && kr <= incl) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (kr <= cum + c[j]) {
                            picked[0] = prefix | ((uint32_t)(BINS - 1 - 4 * lane - j) << shift);
                            picked[1] = kr - cum;
                            break;
                        }
                        cum += c[j];
                    }
                }
            }
            __syncthreads();      // (the next pass writes `picked` behind its own first barrier: every read below is done by then)
            prefix = picked[0];
            kr = picked[1];
        }
        T = prefix;
        need = kr;
    }

    // ---- the compaction, in element order
    // (the lane's sixteen verdicts as two bit masks in vector registers: as compare results they would each hold a scalar pair)
    uint32_t gt_mask = 0, eq_mask = 0;
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
#pragma unroll
        for (int j = 0; j < RUN; ++j) {
            gt_mask |= (key[s][j] > T ? 1u : 0u) << (s * RUN + j);
            eq_mask |= (key[s][j] == T ? 1u : 0u) << (s * RUN + j);
        }
    }
    uint32_t cnt[STEPS], incl[STEPS];
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
        cnt[s] = (uint32_t)__popc((gt_mask >> (s * RUN)) & 0xfu) + ((uint32_t)__popc((eq_mask >> (s * RUN)) & 0xfu) << 16);
        incl[s] = wave_inclusive_scan(cnt[s]);
        if (lane == 63) totals[s][wv] = incl[s];
    }
    if constexpr (PACKED) {      // H, the item's largest key, through the same barrier (an element past the end holds key 0: below or equal to every real one)
        uint32_t h = 0;
#pragma unroll
        for (int s = 0; s < STEPS; ++s) {
#pragma unroll
            for (int j = 0; j < RUN; ++j) h = key[s][j] > h ? key[s][j] : h;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const uint32_t y = __shfl_xor(h, d, 64);
            h = y > h ? y : h;
        }
        if (lane == 0) wave_max[wv] = h;
    }
    __syncthreads();
    uint32_t H = 0;
    if constexpr (PACKED) {
#pragma unroll
        for (int j = 0; j < WAVES; ++j) H = wave_max[j] > H ? wave_max[j] : H;
    }
    // (both the same in every lane, read from LDS: as scalars, so that the level thresholds are; k_t == 0: T = NO_KEY, nothing is kept and nothing asks)
    const Levels lv(PACKED ? __builtin_amdgcn_readfirstlane(T) : T, PACKED ? __builtin_amdgcn_readfirstlane(H) : H);
    uint32_t carry = 0;
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
        uint32_t before = carry;
#pragma unroll
        for (int j = 0; j < WAVES; ++j) {
            const uint32_t x = totals[s][j];
            if (j < wv) before += x;
            carry += x;
        }
        before += incl[s] - cnt[s];
        uint32_t g = before & 0xffffu, q = before >> 16;      // keys > T, keys == T before the element
        const uint32_t e = (uint32_t)(s * STEP_ELEMS + RUN * tid);
        float dec[RUN], res[RUN];
#pragma unroll
        for (int j = 0; j < RUN; ++j) {
            const bool is_gt = (gt_mask >> (s * RUN + j)) & 1u, is_eq = (eq_mask >> (s * RUN + j)) & 1u;
            const bool kept = is_gt || (is_eq && q < need);
            const uint32_t slot = g + (q < need ? q : need);
            if constexpr (PACKED) {
                dec[j] = w[s][j] * 0.0f;
                if (kept) {
                    // (the key anew from w: the sixteen key registers end with the masks above)
                    const uint32_t l = lv.level(key_of(w[s][j])), sign = __float_as_uint(w[s][j]) >> 31;
                    dec[j] = __uint_as_float(lv.key(l) | (sign << 31));
                    if (slot < (uint32_t)MAX_KEPT) spos[slot] = (uint16_t)((e + j) | (l << 12) | (sign << 15));
                }
            } else {
                if (kept && slot < (uint32_t)MAX_KEPT) {
                    spos[slot] = (uint16_t)(e + j);
                    sval[slot] = w[s][j];
                }
                dec[j] = w[s][j] * (kept ? 1.0f : 0.0f);
            }
            res[j] = w[s][j] - dec[j];
            g += is_gt ? 1u : 0u;
            q += is_eq ? 1u : 0u;
        }
        if (o) store_run(o, e, it.len, vec_o, dec);
        if (EF && err) {
            store_run(v, e, it.len, vec_in, w[s]);
            store_run(err, e, it.len, vec_in, res);
        }
    }
    __syncthreads();

    // ---- the item's run of the section; the tensor's last item also writes the pads
    const uint32_t stop = it.e0 + it.kt;
    if constexpr (PACKED) {
        if (tid == 0) {      // the item's bounds, 8-byte aligned; behind an odd number of them 8 zero bytes
            uint2 *b = reinterpret_cast<uint2 *>(wire + it.bounds_offset());
            b[0] = it.kt != 0 ? make_uint2(T, H) : make_uint2(0u, 0u);
            if (it.last && (it.items() & 1)) b[1] = make_uint2(0u, 0u);
        }
        store_entries<uint16_t>(reinterpret_cast<uint16_t *>(wire + it.word_offset()), spos, it.e0, it.kt, it.last ? (it.K + 7u) & ~7u : stop);
    } else {
        uint16_t *pos = reinterpret_cast<uint16_t *>(wire + it.rec[3]);
        float *val = reinterpret_cast<float *>(wire + it.value_offset());
        store_entries<uint16_t>(pos, spos, it.e0, it.kt, it.last ? (it.K + 7u) & ~7u : stop);
        store_entries<float>(val, sval, it.e0, it.kt, it.last ? (it.K + 3u) & ~3u : stop);
    }
}

// two or four bytes of a payload at any alignment: the widest loads the address allows
__device__ __forceinline__ uint32_t load_u16(const uint8_t *p) {
    if ((reinterpret_cast<uintptr_t>(p) & 1) == 0) return *reinterpret_cast<const uint16_t *>(p);
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8);
}

__device__ __forceinline__ uint32_t load_u32(const uint8_t *p) {
    if ((reinterpret_cast<uintptr_t>(p) & 3) == 0) return *reinterpret_cast<const uint32_t *>(p);
    return load_u16(p) | (load_u16(p + 2) << 16);
}

__device__ __forceinline__ void tile_add(float *tile, uint32_t pos, uint32_t bits, uint32_t len, bool direct) {
    const float x = __uint_as_float(bits);
    if (pos < len) tile[pos] = direct ? x : tile[pos] + x;
}

__device__ __forceinline__ void tile_add_word(float *tile, uint32_t word, const Levels &lv, uint32_t len, bool direct) {
    tile_add(tile, word & 0xfffu, lv.key((word >> 12) & 7u) | ((word & 0x8000u) << 16), len, direct);
}

// PACKED: per payload the item's { T, H } (any alignment), then four words a lane as one 8-byte load where the address allows, each
// magnitude rebuilt in the lane; the tile, the barriers and the order of additions are the same in both formats
template <bool PACKED>
__global__ __launch_bounds__(THREADS) void ctk_decode_kernel(const int64_t *__restrict__ seg_table, const int32_t *__restrict__ item_seg,
                                                             const uint8_t *__restrict__ gathered, int64_t stride, int R,
                                                             float *__restrict__ out, int plain, int cr) {
    __shared__ __align__(16) float tile[CHUNK];
    const int tid = threadIdx.x;
    const Item it(seg_table, item_seg, cr);
    float *o = out + it.rec[5] + it.base;
#pragma unroll
    for (int s = 0; s < STEPS; ++s) reinterpret_cast<float4 *>(tile)[s * THREADS + tid] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    __syncthreads();
    const bool direct = plain && R == 1;
    const int64_t pos_at = (PACKED ? it.word_offset() : it.rec[3]) + 2 * (int64_t)it.e0;
    const int64_t val_at = PACKED ? it.bounds_offset() : it.value_offset() + 4 * (int64_t)it.e0;      // (PACKED: the item's bounds)
    for (int r = 0; r < R; ++r) {
        const uint8_t *pp = gathered + (int64_t)r * stride + pos_at, *pv = gathered + (int64_t)r * stride + val_at;
        uint32_t done = 0;
        if constexpr (PACKED) {
            const Levels lv(load_u32(pv), load_u32(pv + 4));
            if ((reinterpret_cast<uintptr_t>(pp) & 7) == 0) {
                const uint32_t groups = it.kt / 4;
                for (uint32_t g = tid; g < groups; g += THREADS) {
                    const uint2 ws = *reinterpret_cast<const uint2 *>(pp + 8 * g);
                    tile_add_word(tile, ws.x & 0xffffu, lv, it.len, direct);
                    tile_add_word(tile, ws.x >> 16, lv, it.len, direct);
                    tile_add_word(tile, ws.y & 0xffffu, lv, it.len, direct);
                    tile_add_word(tile, ws.y >> 16, lv, it.len, direct);
                }
                done = 4 * groups;
            }
            for (uint32_t j = done + tid; j < it.kt; j += THREADS) tile_add_word(tile, load_u16(pp + 2 * j), lv, it.len, direct);
        } else {
            if ((reinterpret_cast<uintptr_t>(pp) & 7) == 0 && aligned16(pv)) {      // four pairs a lane: 8 bytes of pos, 16 of values
                const uint32_t groups = it.kt / 4;
                for (uint32_t g = tid; g < groups; g += THREADS) {
                    const uint2 ps = *reinterpret_cast<const uint2 *>(pp + 8 * g);
                    const uint4 vs = *reinterpret_cast<const uint4 *>(pv + 16 * g);
                    tile_add(tile, ps.x & 0xffffu, vs.x, it.len, direct);
                    tile_add(tile, ps.x >> 16, vs.y, it.len, direct);
                    tile_add(tile, ps.y & 0xffffu, vs.z, it.len, direct);
                    tile_add(tile, ps.y >> 16, vs.w, it.len, direct);
                }
                done = 4 * groups;
            }
            for (uint32_t j = done + tid; j < it.kt; j += THREADS) tile_add(tile, load_u16(pp + 2 * j), load_u32(pv + 4 * j), it.len, direct);
        }
        __syncthreads();      // payloads in order: r + 1 adds to what r left
    }
    const float fR = (float)R;
    const bool vec_o = aligned16(o);
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
        const uint32_t e = (uint32_t)(s * STEP_ELEMS + RUN * tid);
        const float4 a = reinterpret_cast<const float4 *>(tile)[s * THREADS + tid];
        float x[RUN] = {a.x, a.y, a.z, a.w};
        if (!direct) {
#pragma unroll
            for (int j = 0; j < RUN; ++j) x[j] = x[j] / fR;
        }
        store_run(o, e, it.len, vec_o, x);
    }
}

static int check_batch(const gq_ctk_batch *b, const char *what) {
    const int rc = gqsp::check_batch_common(b, what);
    if (rc != GQ_OK) return rc;
    if (b->cr < GQ_CTK_MIN_CR || b->cr > GQ_CTK_MAX_CR)
        return fail(GQ_ERR_INVALID_ARG, "%s: cr = %d (%d ... %d)", what, b->cr, GQ_CTK_MIN_CR, GQ_CTK_MAX_CR);
    if (b->ndense > 0 && !b->dense_table) return fail(GQ_ERR_INVALID_ARG, "%s: null dense table", what);
    return GQ_OK;
}

// the two launches in either value format: the checks and the arguments are the same
template <bool PACKED>
static int compress(const gq_ctk_batch *b, uint8_t *wire, float ef_scale, float *out, void *stream, const char *what) {
    const int rc = check_batch(b, what);
    if (rc != GQ_OK) return rc;
    if (!wire || (reinterpret_cast<uintptr_t>(wire) & 15) != 0) return fail(GQ_ERR_INVALID_ARG, "%s: the wire must be a 16-byte aligned device address", what);
    if ((reinterpret_cast<uintptr_t>(out) & 3) != 0) return fail(GQ_ERR_INVALID_ARG, "%s: out must be 4-byte aligned", what);
    const dim3 items((unsigned)b->nitems), block(THREADS);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (!isnan(ef_scale))
        hipLaunchKernelGGL(HIP_KERNEL_NAME(ctk_compress_kernel<true, PACKED>), items, block, 0, st, b->seg_table, b->item_seg, wire, out, ef_scale,
                           b->cr, b->dense_table, b->ndense);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(ctk_compress_kernel<false, PACKED>), items, block, 0, st, b->seg_table, b->item_seg, wire, out, 0.0f,
                           b->cr, b->dense_table, b->ndense);
    GQL_CHECK_LAUNCH(what);
    return GQ_OK;
}

template <bool PACKED>
static int decode_sum(const gq_ctk_batch *b, const uint8_t *gathered, int64_t user_stride_bytes, int R, float *out, int plain, void *stream,
                      const char *what) {
    const int rc = check_batch(b, what);
    if (rc != GQ_OK) return rc;
    if (!gathered || !out) return fail(GQ_ERR_INVALID_ARG, "%s: null pointer", what);
    if ((reinterpret_cast<uintptr_t>(out) & 3) != 0) return fail(GQ_ERR_INVALID_ARG, "%s: out must be 4-byte aligned", what);
    if (R < 1 || (R > 1 && user_stride_bytes < 0)) return fail(GQ_ERR_INVALID_ARG, "%s: R = %d, user stride %lld", what, R, (long long)user_stride_bytes);
    if (plain && R != 1) return fail(GQ_ERR_INVALID_ARG, "%s: plain takes one payload, R = %d", what, R);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(ctk_decode_kernel<PACKED>), dim3((unsigned)b->nitems), dim3(THREADS), 0,
                       reinterpret_cast<hipStream_t>(stream), b->seg_table, b->item_seg, gathered, user_stride_bytes, R, out, plain ? 1 : 0, b->cr);
    GQL_CHECK_LAUNCH(what);
    return GQ_OK;
}

}  // namespace gqc

GQC_API int gq_ctk_abi_version(void) { return GQ_CTK_ABI_VERSION; }

GQC_API const char *gq_ctk_last_error(void) { return gqc::err_buf; }

GQC_API int gq_ctk_compress_batched(const gq_ctk_batch *b, uint8_t *wire, float ef_scale, float *out, void *stream) {
    return gqc::compress<false>(b, wire, ef_scale, out, stream, "gq_ctk_compress_batched");
}

GQC_API int gq_ctk_compress_packed_batched(const gq_ctk_batch *b, uint8_t *wire, float ef_scale, float *out, void *stream) {
    return gqc::compress<true>(b, wire, ef_scale, out, stream, "gq_ctk_compress_packed_batched");
}

GQC_API int gq_ctk_decode_sum_batched(const gq_ctk_batch *b, const uint8_t *gathered, int64_t user_stride_bytes, int R, float *out,
                                      int plain, void *stream) {
    return gqc::decode_sum<false>(b, gathered, user_stride_bytes, R, out, plain, stream, "gq_ctk_decode_sum_batched");
}

GQC_API int gq_ctk_decode_sum_packed_batched(const gq_ctk_batch *b, const uint8_t *gathered, int64_t user_stride_bytes, int R, float *out,
                                             int plain, void *stream) {
    return gqc::decode_sum<true>(b, gathered, user_stride_bytes, R, out, plain, stream, "gq_ctk_decode_sum_packed_batched");
}
