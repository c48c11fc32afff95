/*
 * libgq_ctk.so -- chunked (block-wise) top-k sparsification on gfx950: every item of 4,096 consecutive elements keeps its own
 * largest len // cr elements.  The select needs nothing outside one workgroup, so a compress is ONE launch that reads the
 * gradient once, with no global scratch, no global atomics and no scan across items; the kept count of an item is fixed by the
 * layout, so the wire has static offsets, no header and no start[] table.
 *
 * A library of its own with the conventions of include/gq_topk.h:
 *   - return value: GQ_OK (0) or a negative GQ_ERR_* code (values of include/gq_hsq.h); gq_ctk_last_error() gives text;
 *   - every pointer is device memory except the descriptor itself; work goes to `stream` (a hipStream_t, NULL = default);
 *   - nothing is allocated inside; float32 tensors.
 *
 * ITEMS.  Item t of a tensor of n elements (1 <= n < 2^31) is elements 4096 t ... min(n, 4096 (t + 1)) - 1, len_t of them.  It
 * keeps k_t = len_t // cr elements, 2 <= cr <= 4096: a full item keeps kf = 4096 // cr, the last item may keep fewer, or 0.
 * K = the sum of the k_t = (n // 4096) * kf + (n % 4096) // cr.
 *
 * KEY AND TIES (include/gq_topk.h's, word for word), w the value the compress works on:
 *     key(w)   = bits(w) & 0x7fffffff, every NaN mapped to 0x7fffffff
 *     kept set of an item = its k_t largest keys; among the elements whose key equals the k_t-th largest, the LOWEST indices.
 *     decoded  = w * (kept ? 1 : 0)        (a dropped element gives copysign(0, w), or NaN for an infinity or a NaN)
 *
 * WIRE SECTION of one tensor (at a 16-byte aligned offset of ONE user's wire), no header:
 *     uint16 pos[K]      the element's index inside its item (0 ... 4095), ascending inside an item; item t's entries are
 *                        t * kf ... t * kf + k_t - 1
 *     zero bytes up to a multiple of 16
 *     f32 value[K]       in the same order: w as it is, bit for bit
 *     zero bytes up to a multiple of 16
 * GQ_CTK_SECTION_BYTES(n, cr) bytes, 6 per kept element.  Every byte, pads included, is written by every compress, and the bytes
 * depend on the input alone.  A compress writes the tensors' sections and the dense copies of dense_table and no other byte of the
 * wire, and loads none of it.
 *
 * PACKED16, the second value format (gq_ctk_compress_packed_batched / gq_ctk_decode_sum_packed_batched): one 16-bit word per kept
 * element, its magnitude as one of eight levels spaced evenly in KEY space -- roughly geometrically in magnitude: the key is a
 * monotone, piecewise-linear stand-in for log2 |w| -- between two bounds of the item.  The kept set, the key and the tie rule are
 * the ones above.  All of it is integer arithmetic on uint32 / uint64.  For an item with k_t > 0:
 *     T = the k_t-th largest key (the smallest kept key), H = the largest key among the item's len_t elements, D = H - T
 * and for a kept element with key k and value w:
 *     level  l  = D == 0 ? 0 : ((uint64)(k - T) * 14 + D) / (2 * D)        0 ... 7, round half up in key space
 *     dk        = T + (uint32)(((uint64)l * D + 3) / 7)                     T <= dk <= H
 *     decoded   = float_from_bits(dk | (bits(w) & 0x80000000))
 *     word      = pos | l << 12 | (bits(w) >> 31) << 15                     pos = the index inside the item, 0 ... 4095
 * so that 14 * |dk - k| <= D + 6.  A dropped element decodes to w * 0 as above.  The formulas' bits are the contract for
 * non-finite input too: a NaN's key is 0x7fffffff, so an item that holds one has H = 0x7fffffff, the NaN sits on level 7 and
 * decodes to a NaN, and an infinity decodes to whatever level it falls on between T and H.
 * WIRE SECTION of one tensor, items = ceil(n / 4096):
 *     uint32 bounds[items][2]   { T, H } of every item; { 0, 0 } where k_t == 0
 *     zero bytes up to a multiple of 16
 *     uint16 word[K]            item t's entries at t * kf ... t * kf + k_t - 1, positions ascending
 *     zero bytes up to a multiple of 16
 * GQ_CTK_PACKED_SECTION_BYTES(n, cr) bytes, 2 per kept element and 8 per item.  As above: every byte, pads included, is written by
 * every compress, the bytes depend on the input alone, and a compress loads none of the wire.
 * Error feedback is unchanged -- w = v + ef_scale * err, err = w - decoded -- but for a kept element that difference is now the
 * quantisation error, not zero.  Rounding is to the nearest level only.
 * A decode computes D = H - T in uint32 arithmetic, whatever the bounds are.
 */
#ifndef GQ_CTK_H
#define GQ_CTK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GQ_CTK_ABI_VERSION 1
#define GQ_CTK_CHUNK 4096      /* elements per item */
#define GQ_CTK_MIN_CR 2
#define GQ_CTK_MAX_CR 4096
#define GQ_CTK_KEPT(n, cr) (((int64_t)(n) / GQ_CTK_CHUNK) * (GQ_CTK_CHUNK / (cr)) + ((int64_t)(n) % GQ_CTK_CHUNK) / (cr))
#define GQ_CTK_SECTION_BYTES(n, cr) ((2 * GQ_CTK_KEPT(n, cr) + 15) / 16 * 16 + (4 * GQ_CTK_KEPT(n, cr) + 15) / 16 * 16)
#define GQ_CTK_PACKED_SECTION_BYTES(n, cr) ((8 * (((int64_t)(n) + GQ_CTK_CHUNK - 1) / GQ_CTK_CHUNK) + 15) / 16 * 16 + (2 * GQ_CTK_KEPT(n, cr) + 15) / 16 * 16)

/*
 * The tensors of one group, table-driven like gq_topk_batch: ONE launch serves all of them.
 *   seg_table int64[nseg][8] = { source (float *), n, first item, wire offset (bytes, a multiple of 16), kf,
 *                                out offset (floats), -, error buffer (float *, 0 = none) }
 *   item_seg  int32[nitems]: the tensor of every item; the items of tensor s are first .. first + ceil(n / GQ_CTK_CHUNK) - 1
 *   dense_table int64[ndense][3] = { source (float *), byte offset in ONE user's wire (a multiple of 4), elements }: the
 *             uncompressed tensors the compress launch copies into the wire as it is (gq_topk_batch.dense_table)
 *   cr        the compression ratio of every tensor of the group
 * There is no scratch.  A decode needs seg_table, item_seg and cr only.
 */
typedef struct gq_ctk_batch {
    uint32_t struct_bytes;     /* sizeof(gq_ctk_batch) */
    int32_t nseg;
    int64_t nitems;
    const int64_t *seg_table;
    const int32_t *item_seg;
    const int64_t *dense_table;
    int32_t ndense;
    int32_t cr;
} gq_ctk_batch;

int gq_ctk_abi_version(void);
const char *gq_ctk_last_error(void);

/*
 * Select and compact, ONE launch: a workgroup per item holds the item in registers, selects inside LDS and writes its run of
 * the section.  The launch arguments do not depend on the data: it replays from a graph.  `wire` must be 16-byte aligned.
 * out != NULL (4-byte aligned): the dense decoded tensors at out + out offset.
 * ef_scale not NaN: error feedback -- w = v + ef_scale * err (the product rounded, then the sum), w is stored back over the source
 * and err = w - decoded (include/gq_topk.h's, word for word); a tensor whose error buffer is 0 is compressed without.
 */
int gq_ctk_compress_batched(const gq_ctk_batch *b, uint8_t *wire, float ef_scale, float *out, void *stream);

/*
 * Decode-mean of R payloads (payload r at gathered + r * user_stride_bytes, ANY alignment) into out + out offset, one launch:
 *     out[j] = (+0 + the values that payloads 0 ... R-1 hold for j, payloads ascending, one f32 addition each) / (float)R
 * a true division.  plain (R == 1 only): the value as it is, +0 where nothing was kept, no division.
 * A `pos` not below the item's length is skipped; a position named twice in ONE payload gives an unspecified value there and
 * nothing else.  Whatever the wire holds, nothing outside the sections is read and nothing outside `out` is written.
 * Refused: a descriptor of another size, cr out of range, bad sizes, null tables or pointers, a misaligned `out`, R < 1, a
 * negative stride, plain with R != 1.
 */
int gq_ctk_decode_sum_batched(const gq_ctk_batch *b, const uint8_t *gathered, int64_t user_stride_bytes, int R, float *out,
                              int plain, void *stream);

/*
 * The same two launches on the PACKED16 section (above): the same arguments, conventions and refusals.  The compress's `out` and
 * its residual take `decoded`, the quantised value; the decode-mean rebuilds every magnitude from the item's { T, H } of that
 * payload (read at any alignment) and adds in gq_ctk_decode_sum_batched's order.
 */
int gq_ctk_compress_packed_batched(const gq_ctk_batch *b, uint8_t *wire, float ef_scale, float *out, void *stream);
int gq_ctk_decode_sum_packed_batched(const gq_ctk_batch *b, const uint8_t *gathered, int64_t user_stride_bytes, int R, float *out,
                                     int plain, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GQ_CTK_H */
