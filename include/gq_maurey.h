/*
 * libgq_maurey.so -- Maurey sparsification (MaureySparsification, maurey_sparsification.py:4-50) on gfx950.
 *
 * A library of its own next to libgq_hsq.so, with the conventions of libgq_topk.so (include/gq_topk.h):
 *   - return value: GQ_OK (0) or a negative GQ_ERR_* code (values of include/gq_hsq.h); gq_maurey_last_error() gives text;
 *   - every pointer is device memory except the descriptor itself; work goes to `stream` (a hipStream_t, NULL = default);
 *   - nothing is allocated inside: the caller owns every scratch buffer the descriptor names;
 *   - every launch's arguments depend on the layout alone: the sequences replay from a HIP graph.
 *
 * Per compressed tensor (n elements, 1 <= n < 2^31; k >= 1 draws, with replacement, so k > n is allowed):
 *     w_i   = v_i, or v_i + ef_scale * err_i under error feedback (the product rounded, then the sum)
 *     a_i   = |w_i| as a double
 *     C_i   = a_0 + ... + a_i in f64, in the FIXED order below;  T = C_{n-1}
 *     draw j (0 <= j < k): u_j in [0, 1), t_j = (double)u_j * T; it selects the smallest i with t_j < C_i (a strict comparison:
 *             an element of weight zero is never drawn).  A t_j that is not below T (a u >= 1 or NaN handed in) is taken as the
 *             largest double below T: the last i whose a_i still moved the sum.
 *     scale = (float)T / (float)k      (f32: T rounded once, then a true division)
 *     D[i]  = scale * (float)(+-m), m = how often i was drawn, the sign that of w_i;  +0 where i was not drawn
 * The order of additions.  An item is a run of GQ_MAUREY_CHUNK = 4096 elements, 16 consecutive elements to each of 256 threads,
 * 16 consecutive threads to a group.  Everything is added left to right: the 16 elements of a thread (s), the 16 thread totals
 * of a group (B), the 16 group totals of an item (G; the last is the item's sum S).  The items of a tensor go to 256 runs of
 * m = ceil(items / 256) consecutive items: the items of a run left to right (s'), the 256 run totals left to right (B').  Then
 *     C_i = B' + (s' + (G + (B + s)))        every + one f64 rounding, innermost first
 * so every level's pieces tile the level above exactly and C is non-decreasing; it depends on the input alone.
 * Degenerate tensor (T == 0, or T not finite: an inf or NaN element): every draw selects index 0 with a plus sign; scale is
 * computed as above (0, inf or NaN), so D[0] = scale * k and every other D[i] = +0.
 *
 * Wire section of one tensor (at a 16-byte aligned offset of ONE user's wire), 16 + roundup(4k, 16) bytes:
 *     16 bytes   scale (f32), 12 zero bytes
 *     k words    little-endian uint32  index | (w_index < 0) << 31,  ascending by index; an index drawn m times appears m times
 *     padding    zero bytes to a multiple of 16
 * The bytes depend on the input and the draws alone (no dependence on workgroup scheduling; every byte is written).
 */
#ifndef GQ_MAUREY_H
#define GQ_MAUREY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GQ_MAUREY_ABI_VERSION 1
#define GQ_MAUREY_CHUNK 4096      /* elements per item */
#define GQ_MAUREY_HEADER_BYTES 16 /* scale + 12 zero bytes in front of a section's words */

/*
 * The tensors of one group, table-driven like gq_topk_batch: ONE launch per stage serves all of them.
 *   seg_table int64[nseg][8] = { source (float *), n, first item, wire offset (bytes, a multiple of 16), k,
 *                                out offset (floats), first draw, error buffer (float *, 0 = none) }
 *             first draw of tensor s = k_0 + ... + k_{s-1} (ascending, no gaps); ndraws = the sum of all k
 *   item_seg  int32[nitems]: the tensor of every item; the items of tensor s are first .. first + ceil(n / GQ_MAUREY_CHUNK) - 1
 *   sums      double[nitems][4]: per item S, B', s', the item's last C           (written before they are read)
 *   totals    double[nseg]: T                                                     (written before it is read)
 *   counts    int32[nitems][3]: draws of the item, its first output word, a cursor (written before they are read)
 *   draw_item int32[ndraws], bucket float[ndraws]: the item of every draw; the draws' u grouped by item  (likewise)
 *   dense_table int64[ndense][3] = { source (float *), byte offset in ONE user's wire (a multiple of 4), elements }: the
 *             uncompressed tensors the compress copies into the wire as they are (gq_topk_batch.dense_table)
 * NOTHING has to be zero when a compress starts: the launch that scans the item sums clears the draw counts before the draws
 * are counted, and every other word is written before it is read -- a replayed graph of the launches needs no reset node.
 * A decode needs seg_table and item_seg only.
 */
typedef struct gq_maurey_batch {
    uint32_t struct_bytes;     /* sizeof(gq_maurey_batch) */
    int32_t nseg;
    int64_t nitems;
    int64_t ndraws;
    const int64_t *seg_table;
    const int32_t *item_seg;
    double *sums;
    double *totals;
    int32_t *counts;
    int32_t *draw_item;
    float *bucket;
    const int64_t *dense_table;
    int32_t ndense;
    int32_t reserved;
} gq_maurey_batch;

int gq_maurey_abi_version(void);
const char *gq_maurey_last_error(void);

/*
 * Sample and write the sections, in six launches (item sums, their per-tensor scan + the headers, the draws counted per item,
 * the counts' scan, the draws bucketed by item, one workgroup per item that places its draws and writes them in index order).
 * random_mode (GQ_RANDOM_* of include/gq_hsq.h):
 *     GQ_RANDOM_GIVEN           r is f32[ndraws]: draw j of tensor s reads r[first draw + j]
 *     GQ_RANDOM_DEVICE          u_j = the library's counter-based generator at (seed, first draw + j)
 *     GQ_RANDOM_DEVICE_COUNTER  seed is the address of a device { seed, step } pair (uint64[2]): a replay draws afresh once
 *                               the step word has moved (gq_mean_rows / a step tail of libgq_hsq.so moves it)
 * ef_scale not NaN: error feedback (ps_quantizer.py:35-39) -- w = v + ef_scale * err; the last launch stores w back into the
 * source and err = w - D.
 * out != NULL: the dense D at out + out offset (required with error feedback).
 */
int gq_maurey_compress_batched(const gq_maurey_batch *b, uint8_t *wire, int random_mode, const float *r, uint64_t seed,
                               float ef_scale, float *out, void *stream);

/*
 * Decode-mean of R payloads (payload r at gathered + r * user_stride_bytes) into out + out offset, one launch:
 *     out[i] = (+0 + D_0[i] + ... + D_{R-1}[i]) / R     payloads in order, a true division (gq_mean_rows' arithmetic)
 * D_r[i] = scale_r * (float)(+-m) for the m words of payload r that carry i (one rounding), +0 if none does.
 * plain (R == 1 only): D_0 as it is, no division.
 */
int gq_maurey_decode_sum_batched(const gq_maurey_batch *b, const uint8_t *gathered, int64_t user_stride_bytes, int R, float *out,
                                 int plain, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GQ_MAUREY_H */
