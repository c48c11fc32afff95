/*
 * libgq_stc.so -- sparse ternary compression (Sattler et al., "Robust and Communication-Efficient Federated Learning from
 * Non-IID Data", 2019) on gfx950: top-k's kept set, ONE magnitude mu for all of it, a 16-bit word per kept element.
 *
 * A library of its own with the conventions of include/gq_topk.h:
 *   - return value: GQ_OK (0) or a negative GQ_ERR_* code (values of include/gq_hsq.h); gq_stc_last_error() gives text;
 *   - every pointer is device memory except the descriptor itself; work goes to `stream` (a hipStream_t, NULL = default);
 *   - nothing is allocated inside: the caller owns every scratch buffer the descriptor names.
 *
 * Per compressed tensor (n elements, 1 <= n < 2^31, k = n // cr, 0 <= k <= n), w the value the compress works on:
 *     key(w)   = bits(w) & 0x7fffffff, every NaN mapped to 0x7fffffff
 *     kept set = the k largest keys; among the elements whose key equals the k-th largest (T), the LOWEST indices -- exactly
 *                include/gq_topk.h's.  gt = #(key > T), need = k - gt = the number of kept ties.
 *     mu       = f32( S / (double)k ), +0 when k = 0; a NaN mu is the ONE pattern 0x7fc00000.  S is a float64 sum of the kept
 *                |w| in a fixed order (an item: GQ_STC_CHUNK consecutive elements, the last one padded; |w| = w with bit 31 cleared):
 *         x[j]     = key(w[j]) > T ? (double)|w[j]| : +0.0     for the 4,096 slots of an item (slots past n: +0.0)
 *         halve(x, m): for h = m / 2, m / 4, ..., 1:  x[j] = x[j] + x[j + h] for every j < h;  the result is x[0]
 *         s[t]     = halve(x of item t, 4096)
 *         S        = halve(s padded with +0.0 to the next power of two P >= the number of items, P)
 *                    + (double)need * (double)float_from_bits(T)         (the product rounded, then the sum; k = 0: S unused)
 *       The kept ties all have the magnitude float_from_bits(T), so S does not depend on which of them are kept.  Every
 *       addition is an IEEE float64 addition; nothing depends on the grid, on scheduling or on atomics.
 *     decoded  = kept ? copysign(mu, w) : +0.0f       (the sign is bit 31 of w: a kept -0 or a kept NaN carries its sign bit)
 *
 * Wire section of one tensor (at a 16-byte aligned offset of ONE user's wire), every byte written by every compress:
 *     uint32 { k, bits(mu), nitems = ceil(n / GQ_STC_CHUNK), 0 }
 *     uint32 start[nitems]     the number of kept elements in the items before this one: item t's words are
 *                              start[t] .. start[t + 1] - 1, the last item's end at k
 *     uint16 word[k]           pos | sign << 15, pos = the element's index inside its item (0 ... 4095; bits 12-14 zero), sign =
 *                              bit 31 of w; ascending by index
 *     zero bytes up to a multiple of 16
 * GQ_STC_SECTION_BYTES(n, k) bytes.  The bytes depend on the input alone.  A compress writes the tensors' sections and the
 * dense copies of dense_table and no other byte of the wire.
 */
#ifndef GQ_STC_H
#define GQ_STC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GQ_STC_ABI_VERSION 1
#define GQ_STC_CHUNK 4096      /* elements per item: every launch walks a tensor in chunks of this many elements */
#define GQ_STC_HIST_BINS 2048  /* uint32 words of histogram per tensor */
#define GQ_STC_HEADER_BYTES 16
#define GQ_STC_NAN 0x7fc00000u /* the pattern of a NaN mu, in `state`, in the header and (with w's sign) in the decoded tensor */
#define GQ_STC_SECTION_BYTES(n, k) \
    ((GQ_STC_HEADER_BYTES + 4 * (((int64_t)(n) + GQ_STC_CHUNK - 1) / GQ_STC_CHUNK) + 2 * (int64_t)(k) + 15) / 16 * 16)

/*
 * The tensors of one group, table-driven like gq_topk_batch: ONE launch per stage serves all of them.
 *   seg_table int64[nseg][8] = { source (float *), n, first item, wire offset (bytes, a multiple of 16), k,
 *                                out offset (floats), -, error buffer (float *, 0 = none) }
 *   item_seg  int32[nitems]: the tensor of every item; the items of tensor s are first .. first + ceil(n / GQ_STC_CHUNK) - 1
 *   hist      uint32[nseg][GQ_STC_HIST_BINS]: ZERO when a compress starts; the compress leaves it zero again (the pick
 *             launches clear what they read), so a replayed graph of the launches needs no reset node
 *   state     int32[nseg][4]: { T, need, bits(mu), - } per tensor; written before they are read
 *   counts    int32[nitems][2]: per-item counts, then their exclusive scans; written before they are read
 *   sums      float64[nitems]: the items' s[t], reduced in place per tensor; written before they are read
 *   dense_table int64[ndense][3] = { source (float *), byte offset in ONE user's wire (a multiple of 4), elements }: the
 *             uncompressed tensors the compress launch copies into the wire as it is (gq_topk_batch.dense_table)
 * A decode needs seg_table and item_seg only.
 */
typedef struct gq_stc_batch {
    uint32_t struct_bytes;     /* sizeof(gq_stc_batch) */
    int32_t nseg;
    int64_t nitems;
    const int64_t *seg_table;
    const int32_t *item_seg;
    uint32_t *hist;
    int32_t *state;
    int32_t *counts;
    double *sums;
    const int64_t *dense_table;
    int32_t ndense;
    int32_t reserved;
} gq_stc_batch;

int gq_stc_abi_version(void);
const char *gq_stc_last_error(void);

/*
 * Select, reduce and compact, in top-k's eight launches (three 11/11/9-bit radix histogram passes with a per-tensor pick behind
 * each, the per-item counts and sums s[t], their scan and mu, the write).  The launch arguments do not depend on the data: the
 * sequence replays from a graph.
 * ef_scale not NaN: error feedback -- every pass reads w = v + ef_scale * err (the product rounded, then the sum), and the
 * write launch stores w back into the source and err = w - decoded.
 * out != NULL: the dense decoded tensors at out + out offset (required with error feedback).
 */
int gq_stc_compress_batched(const gq_stc_batch *b, uint8_t *wire, float ef_scale, float *out, void *stream);

/*
 * Decode-mean of R payloads (payload r at gathered + r * user_stride_bytes) into out + out offset, one launch:
 *     out[i] = (+0 + c_0[i] + ... + c_{R-1}[i]) / R     payloads in order, a true division (gq_topk_decode_sum_batched's arithmetic)
 * where c_r[i] is float_from_bits(header word 1 of payload r) with bit 31 replaced by the sign bit of the word that names i, or
 * +0 if payload r has no such word.
 * plain (R == 1 only): c_0 as it is (a -mu stays -mu, also for mu = 0), +0 elsewhere, no division.
 * A workgroup decodes one item from start[] directly.  k and nitems are the TABLE's: every start is clamped to the table's k
 * and a word whose bits 0-14 are not below the item's length is skipped, so whatever the wire holds no byte outside the
 * sections is read and none outside `out` is written (a wire that names an index twice in one payload gives an unspecified
 * value there).
 */
int gq_stc_decode_sum_batched(const gq_stc_batch *b, const uint8_t *gathered, int64_t user_stride_bytes, int R, float *out,
                              int plain, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GQ_STC_H */
