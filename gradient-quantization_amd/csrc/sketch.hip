// A count-sketch compressor whose wire adds across users, multi-tensor (segment table) form -- libgq_sketch.so
// (include/gq_sketch.h, which defines every value here to the bit).
//
//   sketch   a workgroup per UNIT = one chunk (up to 8 items) of one window's list.  The unit owns its 4,096 cells: no atomics.  An
//            item is staged into LDS coalesced (16 KB, 16-byte loads, the sign bits flipped on the way in: the 64 sign words of every
//            item of the unit are computed once, one finaliser per 64 elements, and kept in 4 KB of LDS); the next item's loads are in
//            flight while this one is consumed, two buffers in turn, one barrier per item.  A thread owns the 16 cells
//            tid + 256 q in registers and gathers the element that maps to each, t = A^-1 (cell - off) & 4095: the lanes of a wave
//            read at an odd stride, so distinct banks.  The chunk's partial sums go to scratch, 256 bytes per wave and store.
//   fold     a workgroup per window: the chunks' partials in order from +0 -> the wire section (mode 0: + the header, + the dense
//            copies) or, for the error accumulation, E = T - that (mode 1).
//   sum      a workgroup per window: T = (the R payloads' cells in order from +0) / R, + E.
//   estimate a workgroup per item: a row's window of T (which fits the L2) staged into LDS and gathered from there, the signs from a
//            wave-uniform word (a wave's 64 elements share it, the lane is the bit), the median network -> est.
//   select   top-k's radix select, count, scan (csrc/sparse_kernels.hpp) on est; store: est where kept, +0 elsewhere.
//   recover  (the chunked recovery, in place of estimate, select and store) a workgroup per item: the estimates stay in registers, the
//            item's own select runs in a 256-bin LDS histogram, the dense output is written once -- see recover_kernel.
// Every launch's arguments depend on the layout and the seed alone.
#include <math.h>

#include "gq_lib_prelude.hpp"
#include "gq_sketch.h"
#include "hadamard.hpp"
#include "sketch_host.hpp"
#include "sparse_kernels.hpp"

#define GQK_API extern "C" __attribute__((visibility("default")))

namespace gqk {

using gql::copy_dense;
using gql::err_buf;
using gql::fail;
using gqsp::block_exclusive_scan;
using gqsp::key_of;
using gqsp::NO_KEY;
using gqsp::THREADS;
using gqsp::WAVES;

struct Sizes {      // what the select's kernels (csrc/sparse_kernels.hpp) are instantiated over
    static constexpr int CHUNK = GQ_SKETCH_CHUNK, BINS = GQ_SKETCH_HIST_BINS;
};
constexpr int CHUNK = GQ_SKETCH_CHUNK;
constexpr int MASK = CHUNK - 1;
constexpr int PER_THREAD = CHUNK / THREADS;      // 16 cells in registers
constexpr int UNIT = GQ_SKETCH_CHUNK_ITEMS;
constexpr int HDR = GQ_SKETCH_HEADER_BYTES;
constexpr int MAX_ROWS = GQ_SKETCH_MAX_ROWS;
constexpr uint64_t G = gqk_host::G, M = gqk_host::M;
static_assert(CHUNK == 4096 && CHUNK == 16 * THREADS, "a staging thread moves four float4; 12-bit cells");
static_assert(sizeof(gq_sketch_batch) == 176, "gq_sketch_batch: the layout the ctypes binding declares (gq_amd/native.py)");
static_assert(offsetof(gq_sketch_batch, recover) == GQ_SKETCH_BATCH_BYTES_V1, "{ recover, cr } follow the whole version-1 descriptor");

// what the hash needs of every row, by value in the launch: K_j, A_j and A_j^-1 mod 4096
struct Rows {
    uint64_t key[MAX_ROWS];
    uint32_t mul[MAX_ROWS], inv[MAX_ROWS];
};

__device__ __forceinline__ uint64_t sign_word(uint64_t key, uint32_t a, uint32_t g) {
    return gqx::splitmix_fin(key + ((((uint64_t)a) << 6) + g + 1) * M);
}

__device__ __forceinline__ float flip(float w, uint32_t bit) { return __uint_as_float(__float_as_uint(w) ^ (bit << 31)); }

// the four float4 of item a that thread tid stages: positions 4 (tid + 256 p) .. + 3, +0 past the tensor's end
__device__ __forceinline__ void load_item(const float *__restrict__ src, int64_t n, uint32_t a, bool vec, float4 (&x)[4]) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int64_t i = (int64_t)a * CHUNK + 4 * (threadIdx.x + THREADS * p);
        if (vec && i + 3 < n) {
            x[p] = *reinterpret_cast<const float4 *>(src + i);
        } else {
            x[p].x = i < n ? src[i] : 0.0f;
            x[p].y = i + 1 < n ? src[i + 1] : 0.0f;
            x[p].z = i + 2 < n ? src[i + 2] : 0.0f;
            x[p].w = i + 3 < n ? src[i + 3] : 0.0f;
        }
    }
}

// ... into the buffer, signed: the float4 at position t lies in sign word t >> 6 = (tid >> 4) + 16 p, at bits 4 (tid & 15) .. + 3
__device__ __forceinline__ void stage_item(float *__restrict__ buf, const uint64_t *__restrict__ words, const float4 (&x)[4]) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const uint32_t nib = (uint32_t)(words[(threadIdx.x >> 4) + 16 * p] >> (4 * (threadIdx.x & 15))) & 15u;
        float4 y;
        y.x = flip(x[p].x, nib & 1u), y.y = flip(x[p].y, (nib >> 1) & 1u), y.z = flip(x[p].z, (nib >> 2) & 1u), y.w = flip(x[p].w, nib >> 3);
        *reinterpret_cast<float4 *>(buf + 4 * (threadIdx.x + THREADS * p)) = y;
    }
}

// src_base != NULL: the tensors are read at src_base + out offset (the decoded tensors, for the error accumulation)
__global__ __launch_bounds__(THREADS) void sketch_kernel(const int64_t *__restrict__ seg_table, const int64_t *__restrict__ lay,
                                                         const int32_t *__restrict__ win_tab, const int32_t *__restrict__ unit_tab,
                                                         const uint32_t *__restrict__ list, float *__restrict__ part,
                                                         const float *__restrict__ src_base, Rows rows) {
    __shared__ __attribute__((aligned(16))) float buf[2][CHUNK];
    __shared__ uint64_t words[UNIT][64];
    const int64_t u = blockIdx.x;
    const int32_t *ut = unit_tab + 4 * u;
    const int64_t W = ut[0];
    const int cnt = ut[2] < UNIT ? ut[2] : UNIT;
    const uint32_t *ent = list + ut[1];
    const int seg = win_tab[4 * W];
    const int64_t *rec = seg_table + 8 * (int64_t)seg;
    const int64_t n = rec[1], nwin = rec[6];
    const int j = (int)((W - lay[seg]) / nwin);
    const float *src = src_base ? src_base + rec[5] : reinterpret_cast<const float *>(rec[0]);
    const bool vec = gql::aligned16(src);
    uint64_t key = rows.key[0];      // (selects: no indexed kernel argument)
    uint32_t inv = rows.inv[0];
#pragma unroll
    for (int x = 1; x < MAX_ROWS; ++x) {
        key = j == x ? rows.key[x] : key;
        inv = j == x ? rows.inv[x] : inv;
    }
    for (int x = threadIdx.x; x < cnt * 64; x += THREADS) words[x >> 6][x & 63] = sign_word(key, ent[x >> 6] & 0x7ffffu, (uint32_t)x & 63u);
    float acc[PER_THREAD];
#pragma unroll
    for (int q = 0; q < PER_THREAD; ++q) acc[q] = 0.0f;
    float4 x[4];
    load_item(src, n, ent[0] & 0x7ffffu, vec, x);
    __syncthreads();      // (the sign words)
    stage_item(buf[0], words[0], x);
    __syncthreads();
    const uint32_t step = (inv * (uint32_t)THREADS) & MASK;
#pragma unroll 1
    for (int i = 0; i < cnt; ++i) {
        const bool more = i + 1 < cnt;
        if (more) load_item(src, n, ent[i + 1] & 0x7ffffu, vec, x);
        const uint32_t off = ent[i] >> 19;
        uint32_t t = (inv * ((threadIdx.x - off) & MASK)) & MASK;
        const float *b = buf[i & 1];
#pragma unroll
        for (int q = 0; q < PER_THREAD; ++q) {
            acc[q] = acc[q] + b[t];
            t = (t + step) & MASK;
        }
        if (more) stage_item(buf[(i + 1) & 1], words[i + 1], x);      // (its last readers passed the barrier of item i - 1)
        __syncthreads();
    }
    float *o = part + u * CHUNK;
#pragma unroll
    for (int q = 0; q < PER_THREAD; ++q) o[threadIdx.x + THREADS * q] = acc[q];
}

// mode 0: the window's cells into the wire; mode 1: E = T - the window's cells
__global__ __launch_bounds__(THREADS) void fold_kernel(const int64_t *__restrict__ seg_table, const int64_t *__restrict__ lay,
                                                       const int32_t *__restrict__ win_tab, const float *__restrict__ part,
                                                       uint8_t *__restrict__ wire, const float *__restrict__ table,
                                                       const int64_t *__restrict__ etab, int rows, int mode,
                                                       const int64_t *__restrict__ dense_table, int ndense) {
    if (mode == 0) copy_dense<THREADS>(dense_table, ndense, wire);
    const int64_t W = blockIdx.x;
    const int32_t *wt = win_tab + 4 * W;
    const int seg = wt[0];
    const int64_t u0 = wt[1];
    const int chunks = wt[2];
    const int64_t *rec = seg_table + 8 * (int64_t)seg;
    const int64_t lw = W - lay[seg];
    float acc[PER_THREAD];
#pragma unroll
    for (int q = 0; q < PER_THREAD; ++q) acc[q] = 0.0f;
    for (int c = 0; c < chunks; ++c) {
        const float *p = part + (u0 + c) * CHUNK;
#pragma unroll
        for (int q = 0; q < PER_THREAD; ++q) acc[q] = acc[q] + p[threadIdx.x + THREADS * q];
    }
    if (mode == 0) {
        uint32_t *hdr = reinterpret_cast<uint32_t *>(wire + rec[3]);
        if (lw == 0 && threadIdx.x < 4)
            hdr[threadIdx.x] = threadIdx.x == 0 ? (uint32_t)rec[1] : (threadIdx.x == 1 ? (uint32_t)rows : (threadIdx.x == 2 ? (uint32_t)rec[6] : 0u));
        float *o = reinterpret_cast<float *>(wire + rec[3] + HDR) + lw * CHUNK;
#pragma unroll
        for (int q = 0; q < PER_THREAD; ++q) o[threadIdx.x + THREADS * q] = acc[q];
    } else {
        float *e = reinterpret_cast<float *>(etab[seg]) + lw * CHUNK;
        const float *t = table + W * CHUNK;
#pragma unroll
        for (int q = 0; q < PER_THREAD; ++q) e[threadIdx.x + THREADS * q] = t[threadIdx.x + THREADS * q] - acc[q];
    }
}

__global__ __launch_bounds__(THREADS) void sum_kernel(const int64_t *__restrict__ seg_table, const int64_t *__restrict__ lay,
                                                      const int32_t *__restrict__ win_tab, const uint8_t *__restrict__ gathered,
                                                      int64_t stride, int R, float *__restrict__ table, const int64_t *__restrict__ etab) {
    const int64_t W = blockIdx.x;
    const int seg = win_tab[4 * W];
    const int64_t *rec = seg_table + 8 * (int64_t)seg;
    const int64_t lw = W - lay[seg];
    const float fR = (float)R;
    const float *e = etab ? reinterpret_cast<const float *>(etab[seg]) + lw * CHUNK : nullptr;
    float acc[PER_THREAD];
#pragma unroll
    for (int q = 0; q < PER_THREAD; ++q) acc[q] = 0.0f;
    for (int r = 0; r < R; ++r) {
        const float *p = reinterpret_cast<const float *>(gathered + (int64_t)r * stride + rec[3] + HDR) + lw * CHUNK;
#pragma unroll
        for (int q = 0; q < PER_THREAD; ++q) acc[q] = acc[q] + p[threadIdx.x + THREADS * q];
    }
#pragma unroll
    for (int q = 0; q < PER_THREAD; ++q) {
        float t = acc[q] / fR;
        if (e) t = t + e[threadIdx.x + THREADS * q];
        table[W * CHUNK + threadIdx.x + THREADS * q] = t;
    }
}

__device__ __forceinline__ void cx(float &x, float &y) {
    const bool swap = y < x;
    const float lo = swap ? y : x, hi = swap ? x : y;
    x = lo, y = hi;
}

template <int R>
__device__ __forceinline__ float median(float (&p)[R]) {
    if (R == 3) {
        cx(p[0], p[1]), cx(p[1], p[2]), cx(p[0], p[1]);
        return p[1];
    }
    if (R == 5) {
        cx(p[0], p[1]), cx(p[3], p[4]), cx(p[0], p[3]), cx(p[1], p[4]), cx(p[1], p[2]), cx(p[2], p[3]), cx(p[1], p[2]);
        return p[2];
    }
    return p[0];
}

// A row's window of T is staged into LDS coalesced (16 KB, 16-byte loads) and gathered from there at the odd stride A_j -- distinct
// banks across a wave; gathered from global memory, a wave's 64 reads touched 64 cache lines.
template <int R>
__global__ __launch_bounds__(THREADS) void estimate_kernel(const int64_t *__restrict__ seg_table, const int32_t *__restrict__ item_seg,
                                                           const int64_t *__restrict__ lay, const float *__restrict__ table,
                                                           float *__restrict__ est, Rows rows) {
    __shared__ __attribute__((aligned(16))) float win[CHUNK];
    const int64_t item = blockIdx.x;
    const int seg = item_seg[item];
    const int64_t *rec = seg_table + 8 * (int64_t)seg;
    const int64_t n = rec[1], nwin = rec[6], li = item - rec[2];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));      // (uniform: the sign words are the wave's)
    float val[R][PER_THREAD];
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const uint64_t h = gqx::splitmix_fin(rows.key[j] + (uint64_t)(li + 1) * G);
        const int64_t v = (int64_t)(((h >> 32) * (uint64_t)nwin) >> 32);
        const float *T = table + (lay[seg] + j * nwin + v) * CHUNK;
        if (j) __syncthreads();      // (the last row's readers)
#pragma unroll
        for (int p = 0; p < 4; ++p)
            *reinterpret_cast<float4 *>(win + 4 * (threadIdx.x + THREADS * p)) = *reinterpret_cast<const float4 *>(T + 4 * (threadIdx.x + THREADS * p));
        __syncthreads();
        uint32_t c = (rows.mul[j] * threadIdx.x + ((uint32_t)h & (uint32_t)MASK)) & MASK;
        const uint32_t step = (rows.mul[j] * (uint32_t)THREADS) & MASK;
#pragma unroll
        for (int q = 0; q < PER_THREAD; ++q) {      // element t = tid + 256 q: its sign word, t >> 6 = wv + 4 q, is the wave's
            const uint64_t w = sign_word(rows.key[j], (uint32_t)li, wv + 4u * q);
            val[j][q] = flip(win[c], (uint32_t)(w >> lane) & 1u);
            c = (c + step) & MASK;
        }
    }
    float *o = est + rec[5] + li * CHUNK;
    const int64_t len = n - li * CHUNK < CHUNK ? n - li * CHUNK : CHUNK;
#pragma unroll
    for (int q = 0; q < PER_THREAD; ++q) {
        float p[R];
#pragma unroll
        for (int j = 0; j < R; ++j) p[j] = val[j][q];
        const float m = median<R>(p);
        if (threadIdx.x + THREADS * q < len) o[threadIdx.x + THREADS * q] = m;
    }
}

// ---- the chunked recovery (include/gq_sketch.h: CHUNKED RECOVERY): estimate, select and store in ONE launch, a workgroup per item ----
// The estimates never leave the workgroup: after the rows' gathers and the median a thread holds those of the elements t = tid + 256 q,
// q = 0 .. 15, in registers, so ELEMENT ORDER is (q, wave, lane) -- not chunked top-k's (step, thread, slot of a float4), whose
// select this one otherwise follows (csrc/ctk.hip):
//   select   the item's kt-th largest key by radix, 8 + 8 + 8 + 7 bits from the top in a 256-bin LDS histogram (integer LDS adds: the
//            counts do not depend on their order); wave 0 walks the bins from the top, four a lane, fixes the digit and the remaining
//            rank and clears what it read.  -> the threshold key T and `need`, the ties to keep.  An element past the item's end
//            enters as key 0 at the highest indices: it can only swell the lowest bin, below everything the select looks for, and as
//            a tie it ranks behind every real one, of which there are at least `need`.
//   tie rank the output is dense, so nothing is compacted and only the TIES are ranked: per q the wave's lanes with key == T as a
//            ballot, a lane's rank inside the wave the popcount of the bits below it, the waves' totals of all sixteen q through
//            LDS behind one barrier, q ascending as a running carry.
//   store    estimate or +0, one 4-byte store a lane and q: a wave writes 256 consecutive bytes; the item's tail is guarded by len.
constexpr int SELECT_BINS = 256;
static_assert(SELECT_BINS == THREADS && SELECT_BINS == 4 * 64, "a bin a thread to clear; wave 0 walks the bins four a lane");

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

template <int R>
__global__ __launch_bounds__(THREADS) void recover_kernel(const int64_t *__restrict__ seg_table, const int32_t *__restrict__ item_seg,
                                                          const int64_t *__restrict__ lay, const float *__restrict__ table,
                                                          float *__restrict__ out, Rows rows, int cr) {
    __shared__ __attribute__((aligned(16))) float win[CHUNK];
    __shared__ uint32_t hist[SELECT_BINS];
    __shared__ uint32_t picked[2];                     // the pass's prefix and remaining rank
    __shared__ uint32_t ties[PER_THREAD][WAVES];       // per q and wave: its keys == T
    const int64_t item = blockIdx.x;
    const int seg = item_seg[item];
    const int64_t *rec = seg_table + 8 * (int64_t)seg;
    const int64_t n = rec[1], nwin = rec[6], li = item - rec[2];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const uint32_t len = (uint32_t)(n - li * CHUNK < CHUNK ? n - li * CHUNK : CHUNK);
    const uint32_t kt = len / (uint32_t)cr;
    hist[tid] = 0u;
    float est[PER_THREAD];
    uint32_t key[PER_THREAD];
    {      // estimate_kernel's row loop, statement for statement (that kernel keeps its own text: the global recovery's instructions stay)
        const uint32_t uwv = (uint32_t)__builtin_amdgcn_readfirstlane((int)wv);      // (uniform: the sign words are the wave's)
        float val[R][PER_THREAD];
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const uint64_t h = gqx::splitmix_fin(rows.key[j] + (uint64_t)(li + 1) * G);
            const int64_t v = (int64_t)(((h >> 32) * (uint64_t)nwin) >> 32);
            const float *T = table + (lay[seg] + j * nwin + v) * CHUNK;
            if (j) __syncthreads();      // (the last row's readers)
#pragma unroll
            for (int p = 0; p < 4; ++p)
                *reinterpret_cast<float4 *>(win + 4 * (tid + THREADS * p)) = *reinterpret_cast<const float4 *>(T + 4 * (tid + THREADS * p));
            __syncthreads();
            uint32_t c = (rows.mul[j] * tid + ((uint32_t)h & (uint32_t)MASK)) & MASK;
            const uint32_t step = (rows.mul[j] * (uint32_t)THREADS) & MASK;
#pragma unroll
            for (int q = 0; q < PER_THREAD; ++q) {      // element t = tid + 256 q: its sign word, t >> 6 = wv + 4 q, is the wave's
                const uint64_t w = sign_word(rows.key[j], (uint32_t)li, uwv + 4u * q);
                val[j][q] = flip(win[c], (uint32_t)(w >> lane) & 1u);
                c = (c + step) & MASK;
            }
        }
#pragma unroll
        for (int q = 0; q < PER_THREAD; ++q) {
            float p[R];
#pragma unroll
            for (int j = 0; j < R; ++j) p[j] = val[j][q];
            est[q] = median<R>(p);
            key[q] = tid + THREADS * q < len ? key_of(est[q]) : 0u;
        }
    }
    // (hist was cleared in front of the first row's barrier)

    // ---- the select: T = the kt-th largest key, need = how many keys == T are kept
    uint32_t T = NO_KEY, need = 0;
    if (kt != 0) {      // (the same for the whole workgroup)
        uint32_t prefix = 0, kr = kt;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            constexpr uint32_t ALL = 0xffffffffu;
            const int shift = digit_shift(p), hi = shift + digit_bits(p);
            const uint32_t mask = ~(ALL << digit_bits(p));
#pragma unroll
            for (int q = 0; q < PER_THREAD; ++q) {
                const uint32_t k = key[q];
                if ((k >> hi) == (prefix >> hi)) atomicAdd(&hist[(k >> shift) & mask], 1u);
            }
            __syncthreads();
            if (wv == 0) {      // lane l: bins 255 - 4 l downwards, the highest first; it clears what it read
                uint32_t c[4], sum = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int b = SELECT_BINS - 1 - 4 * (int)lane - j;
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
                            picked[0] = prefix | ((uint32_t)(SELECT_BINS - 1 - 4 * (int)lane - j) << shift);
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

    // ---- the ties in element order: (q, wave, lane)
    const uint64_t below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    uint32_t eq_mask = 0, rank_in_wave[PER_THREAD / 4] = {};      // (a rank is at most 63: four to a register, a byte each)
#pragma unroll
    for (int q = 0; q < PER_THREAD; ++q) {
        const bool is_eq = key[q] == T;
        const uint64_t me = __ballot(is_eq);
        eq_mask |= (is_eq ? 1u : 0u) << q;
        rank_in_wave[q / 4] |= (uint32_t)__popcll(me & below) << (8 * (q & 3));
        if (lane == 0) ties[q][wv] = (uint32_t)__popcll(me);
    }
    __syncthreads();
    float *o = out + rec[5] + li * CHUNK;
    uint32_t carry = 0;      // the ties of the steps before q
#pragma unroll
    for (int q = 0; q < PER_THREAD; ++q) {
        uint32_t before = carry;
#pragma unroll
        for (int j = 0; j < WAVES; ++j) {
            const uint32_t x = ties[q][j];
            if (j < (int)wv) before += x;
            carry += x;
        }
        before += (rank_in_wave[q / 4] >> (8 * (q & 3))) & 0xffu;
        const bool kept = key[q] > T || (((eq_mask >> q) & 1u) && before < need);
        if (tid + THREADS * q < len) o[tid + THREADS * q] = kept ? est[q] : 0.0f;
    }
}

__global__ __launch_bounds__(THREADS) void count_kernel(const int64_t *__restrict__ dec_table, const int32_t *__restrict__ item_seg,
                                                        const int32_t *__restrict__ state, int32_t *__restrict__ counts) {
    __shared__ uint32_t lds[2][WAVES];
    const int64_t item = blockIdx.x;
    const int seg = item_seg[item];
    const int64_t *rec = dec_table + 8 * (int64_t)seg;
    const int64_t n = rec[1];
    const uint32_t T = (uint32_t)state[4 * seg];
    uint32_t gt = 0, eq = 0;
    if (T != NO_KEY) {
        const float *v = reinterpret_cast<const float *>(rec[0]);
        const int64_t base = (item - rec[2]) * CHUNK;
        const int64_t end = base + CHUNK < n ? base + CHUNK : n;
        for (int64_t i = base + threadIdx.x; i < end; i += THREADS) {
            const uint32_t key = key_of(v[i]);
            gt += key > T ? 1u : 0u;
            eq += key == T ? 1u : 0u;
        }
    }
    uint32_t tg, te;
    block_exclusive_scan(gt, lds[0], &tg);
    block_exclusive_scan(eq, lds[1], &te);
    if (threadIdx.x == 0) {
        counts[2 * item] = (int32_t)tg;
        counts[2 * item + 1] = (int32_t)te;
    }
}

__global__ __launch_bounds__(THREADS) void scan_kernel(const int64_t *__restrict__ dec_table, int32_t *__restrict__ counts) {
    const int64_t *rec = dec_table + 8 * (int64_t)blockIdx.x;
    uint32_t total[2];
    gqsp::scan_item_counts<2, 0>(counts, rec[2], (rec[1] + CHUNK - 1) / CHUNK, total);
}

// the dense output: the estimate where kept (top-k's tie rule: csrc/sparse_kernels.hpp), +0 elsewhere
__global__ __launch_bounds__(THREADS) void store_kernel(const int64_t *__restrict__ dec_table, const int32_t *__restrict__ item_seg,
                                                        const int32_t *__restrict__ state, const int32_t *__restrict__ counts,
                                                        float *__restrict__ out) {
    const int64_t item = blockIdx.x;
    const int seg = item_seg[item];
    const int64_t *rec = dec_table + 8 * (int64_t)seg;
    const int64_t n = rec[1];
    const uint32_t T = (uint32_t)state[4 * seg], need = (uint32_t)state[4 * seg + 1];
    uint32_t gt_before = (uint32_t)counts[2 * item], eq_before = (uint32_t)counts[2 * item + 1];
    const float *v = reinterpret_cast<const float *>(rec[0]);
    float *o = out + rec[5];
    const int64_t base = (item - rec[2]) * CHUNK;
    const int64_t end = base + CHUNK < n ? base + CHUNK : n;
#pragma unroll 1
    for (int s = 0; s < PER_THREAD; ++s) {
        const int64_t i = base + (int64_t)s * THREADS + threadIdx.x;
        const bool valid = i < end;
        float w = 0.0f;
        uint32_t key = 0;
        if (valid) {
            w = v[i];
            key = key_of(w);
        }
        const bool is_gt = valid && key > T;
        const bool is_eq = valid && key == T;
        const gqsp::Rank r = gqsp::rank_step<true>(s, is_gt, is_eq, gt_before, eq_before);
        if (valid) o[i] = r.kept(is_gt, is_eq, need) ? w : 0.0f;
        gt_before += r.tg;
        eq_before += r.te;
    }
}

static Rows rows_of(const gq_sketch_batch *b) {
    Rows r = {};
    for (int j = 0; j < b->rows; ++j) {
        r.key[j] = gqk_host::row_key(b->seed, j);
        r.mul[j] = gqk_host::row_mul(r.key[j]);
        r.inv[j] = gqk_host::inverse12(r.mul[j]);
    }
    return r;
}

// a descriptor of the version-1 size has no { recover, cr }: the global recovery
static bool chunked(const gq_sketch_batch *b) {
    return b->struct_bytes == sizeof(gq_sketch_batch) && b->recover == GQ_SKETCH_RECOVER_CHUNKED;
}

// (gqsp::check_batch_common's checks and texts, but for the size: this descriptor has two)
static int check_batch(const gq_sketch_batch *b, const char *what, bool compress, bool decode) {
    if (!b || (b->struct_bytes != sizeof(gq_sketch_batch) && b->struct_bytes != GQ_SKETCH_BATCH_BYTES_V1))
        return fail(GQ_ERR_INVALID_ARG, "%s: descriptor missing or of another size", what);
    if (b->nseg < 1 || b->nitems < 1 || b->nitems > 0x7fffffff || b->ndense < 0)
        return fail(GQ_ERR_INVALID_ARG, "%s: bad sizes (nseg %d, nitems %lld, ndense %d)", what, b->nseg, (long long)b->nitems, b->ndense);
    if (!b->seg_table || !b->item_seg) return fail(GQ_ERR_INVALID_ARG, "%s: null table", what);
    if (b->struct_bytes == sizeof(gq_sketch_batch)) {
        if (b->recover != GQ_SKETCH_RECOVER_GLOBAL && b->recover != GQ_SKETCH_RECOVER_CHUNKED)
            return fail(GQ_ERR_INVALID_ARG, "%s: recover = %d (0: global, 1: chunked)", what, b->recover);
        if (chunked(b) && (b->cr < GQ_SKETCH_MIN_CR || b->cr > GQ_SKETCH_MAX_CR))
            return fail(GQ_ERR_INVALID_ARG, "%s: cr = %d (%d ... %d with the chunked recovery)", what, b->cr, GQ_SKETCH_MIN_CR,
                        GQ_SKETCH_MAX_CR);
    }
    if (b->rows != 1 && b->rows != 3 && b->rows != 5) return fail(GQ_ERR_INVALID_ARG, "%s: rows = %d (1, 3 or 5)", what, b->rows);
    if (b->nwindows < 1 || b->nwindows > 0x7fffffff || b->nunits < 1 || b->nunits > 0x7fffffff)
        return fail(GQ_ERR_INVALID_ARG, "%s: bad sizes (windows %lld, units %lld)", what, (long long)b->nwindows, (long long)b->nunits);
    if (!b->lay || !b->win_tab) return fail(GQ_ERR_INVALID_ARG, "%s: null table", what);
    if (compress && (!b->unit_tab || !b->list || !b->part || (b->ndense > 0 && !b->dense_table)))
        return fail(GQ_ERR_INVALID_ARG, "%s: null table or scratch buffer", what);
    if (decode && (!b->table || (!chunked(b) && (!b->est || !b->dec_table || !b->hist || !b->state || !b->counts))))
        return fail(GQ_ERR_INVALID_ARG, "%s: null scratch buffer", what);
    return GQ_OK;
}

static int sketch_launches(const gq_sketch_batch *b, const float *src_base, uint8_t *wire, int mode, hipStream_t st, const char *what) {
    hipLaunchKernelGGL(sketch_kernel, dim3((unsigned)b->nunits), dim3(THREADS), 0, st, b->seg_table, b->lay, b->win_tab, b->unit_tab,
                       b->list, b->part, src_base, rows_of(b));
    GQL_CHECK_LAUNCH(what);
    hipLaunchKernelGGL(fold_kernel, dim3((unsigned)b->nwindows), dim3(THREADS), 0, st, b->seg_table, b->lay, b->win_tab, b->part, wire,
                       b->table, b->etab, b->rows, mode, b->dense_table, b->ndense);
    GQL_CHECK_LAUNCH(what);
    return GQ_OK;
}

static int decode_launches(const gq_sketch_batch *b, const uint8_t *gathered, int64_t stride, int R, float *out, bool ef, hipStream_t st) {
    const char *what = "gq_sketch_decode_sum_batched";
    const dim3 items((unsigned)b->nitems), segs((unsigned)b->nseg), block(THREADS);
    const Rows rows = rows_of(b);
    hipLaunchKernelGGL(sum_kernel, dim3((unsigned)b->nwindows), block, 0, st, b->seg_table, b->lay, b->win_tab, gathered, stride, R, b->table,
                       ef ? b->etab : nullptr);
    GQL_CHECK_LAUNCH(what);
    if (chunked(b)) {      // the estimate, the select and the store as one launch, the select per item
        if (b->rows == 1) hipLaunchKernelGGL(recover_kernel<1>, items, block, 0, st, b->seg_table, b->item_seg, b->lay, b->table, out, rows, b->cr);
        else if (b->rows == 3) hipLaunchKernelGGL(recover_kernel<3>, items, block, 0, st, b->seg_table, b->item_seg, b->lay, b->table, out, rows, b->cr);
        else hipLaunchKernelGGL(recover_kernel<5>, items, block, 0, st, b->seg_table, b->item_seg, b->lay, b->table, out, rows, b->cr);
        GQL_CHECK_LAUNCH(what);
        if (ef) return sketch_launches(b, out, nullptr, 1, st, what);
        return GQ_OK;
    }
    if (b->rows == 1) hipLaunchKernelGGL(estimate_kernel<1>, items, block, 0, st, b->seg_table, b->item_seg, b->lay, b->table, b->est, rows);
    else if (b->rows == 3) hipLaunchKernelGGL(estimate_kernel<3>, items, block, 0, st, b->seg_table, b->item_seg, b->lay, b->table, b->est, rows);
    else hipLaunchKernelGGL(estimate_kernel<5>, items, block, 0, st, b->seg_table, b->item_seg, b->lay, b->table, b->est, rows);
    GQL_CHECK_LAUNCH(what);
    for (int p = 0; p < 3; ++p) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(gqsp::hist_kernel<Sizes, false>), items, block, 0, st, b->dec_table, b->item_seg, b->state, b->hist, p,
                           0.0f);
        GQL_CHECK_LAUNCH(what);
        hipLaunchKernelGGL(gqsp::pick_kernel<Sizes>, segs, block, 0, st, b->dec_table, b->state, b->hist, p);
        GQL_CHECK_LAUNCH(what);
    }
    hipLaunchKernelGGL(count_kernel, items, block, 0, st, b->dec_table, b->item_seg, b->state, b->counts);
    GQL_CHECK_LAUNCH(what);
    hipLaunchKernelGGL(scan_kernel, segs, block, 0, st, b->dec_table, b->counts);
    GQL_CHECK_LAUNCH(what);
    hipLaunchKernelGGL(store_kernel, items, block, 0, st, b->dec_table, b->item_seg, b->state, b->counts, out);
    GQL_CHECK_LAUNCH(what);
    if (ef) return sketch_launches(b, out, nullptr, 1, st, what);
    return GQ_OK;
}

}  // namespace gqk

GQK_API int gq_sketch_abi_version(void) { return GQ_SKETCH_ABI_VERSION; }

GQK_API const char *gq_sketch_last_error(void) { return gqk::err_buf; }

GQK_API int gq_sketch_build_lists(uint64_t seed, int rows, int64_t items, int64_t nwin, uint32_t *list, int64_t *starts) {
    const int rc = gqk_host::build_lists(seed, rows, items, nwin, list, starts);
    if (rc != 0)
        return gqk::fail(GQ_ERR_INVALID_ARG, "gq_sketch_build_lists: bad argument %d (rows %d, items %lld, windows %lld)", -rc, rows,
                         (long long)items, (long long)nwin);
    return GQ_OK;
}

GQK_API int gq_sketch_compress_batched(const gq_sketch_batch *b, uint8_t *wire, float ef_scale, float *out, void *stream) {
    const char *what = "gq_sketch_compress_batched";
    int rc = gqk::check_batch(b, what, true, out != nullptr);
    if (rc != GQ_OK) return rc;
    if (!wire || (reinterpret_cast<uintptr_t>(wire) & 3) != 0 || (reinterpret_cast<uintptr_t>(out) & 3) != 0)
        return gqk::fail(GQ_ERR_INVALID_ARG, "%s: the wire and `out` must be 4-byte aligned device addresses", what);
    if (!isnan(ef_scale))
        return gqk::fail(GQ_ERR_UNSUPPORTED, "%s: no per-user error feedback (the sketch accumulates its error on the decoding side)", what);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    rc = gqk::sketch_launches(b, nullptr, wire, 0, st, what);
    if (rc != GQ_OK || !out) return rc;
    return gqk::decode_launches(b, wire, 0, 1, out, false, st);
}

GQK_API int gq_sketch_decode_sum_batched(const gq_sketch_batch *b, const uint8_t *gathered, int64_t user_stride_bytes, int R, float *out,
                                         int plain, void *stream) {
    const char *what = "gq_sketch_decode_sum_batched";
    int rc = gqk::check_batch(b, what, b && b->etab && !plain, true);
    if (rc == GQ_OK) rc = gqsp::check_decode(what, gathered, out, user_stride_bytes, R);
    if (rc != GQ_OK) return rc;
    if (plain && R != 1) return gqk::fail(GQ_ERR_INVALID_ARG, "%s: plain takes one payload, got R = %d", what, R);
    if ((reinterpret_cast<uintptr_t>(out) & 3) != 0) return gqk::fail(GQ_ERR_INVALID_ARG, "%s: `out` must be 4-byte aligned", what);
    return gqk::decode_launches(b, gathered, user_stride_bytes, R, out, b->etab && !plain, reinterpret_cast<hipStream_t>(stream));
}
