/*
 * libgq_topk.so -- top-k sparsification (TopKSparsificationCompressor, topk_sparsification_compressor.py:9-26) on gfx950.
 *
 * A library of its own next to libgq_hsq.so: that library's entry-point list is fixed (include/gq_hsq.h), the top-k
 * launches keep the same conventions without widening it.
 *   - return value: GQ_OK (0) or a negative GQ_ERR_* code (values of include/gq_hsq.h); gq_topk_last_error() gives text;
 *   - every pointer is device memory except the descriptor itself; work goes to `stream` (a hipStream_t, NULL = default);
 *   - nothing is allocated inside: the caller owns every scratch buffer the descriptor names.
 *
 * Per compressed tensor (n elements, k = n // cr, 0 <= k <= n):
 *     key(v)   = bits(v) & 0x7fffffff, every NaN mapped to 0x7fffffff   (torch.topk(abs(v)) ranks NaN above +inf)
 *     kept set = the k largest keys; among the elements whose key equals the k-th largest, the LOWEST indices
 *     decoded  = v * (kept ? 1 : 0)                                      (v * 0 = copysign(0, v), or NaN for +-inf / NaN)
 * Wire section of one tensor (at a 16-byte aligned offset of ONE user's wire): k x uint32 index, ascending, then k x f32
 * value -- 8k bytes, no header.  The bytes depend on the input alone (no draws, no dependence on workgroup scheduling).
 * A compress writes the tensors' sections and the dense copies of dense_table and no other byte of the wire.
 */
#ifndef GQ_TOPK_H
#define GQ_TOPK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GQ_TOPK_ABI_VERSION 1
#define GQ_TOPK_CHUNK 4096      /* elements per item: every launch walks a tensor in chunks of this many elements */
#define GQ_TOPK_HIST_BINS 2048  /* uint32 words of histogram per tensor */

/*
 * The tensors of one group, table-driven like gq_qsgd_batch: ONE launch per stage serves all of them.
 *   seg_table int64[nseg][8] = { source (float *), n, first item, wire offset (bytes, a multiple of 16), k,
 *                                out offset (floats), -, error buffer (float *, 0 = none) }
 *   item_seg  int32[nitems]: the tensor of every item; the items of tensor s are first .. first + ceil(n / GQ_TOPK_CHUNK) - 1
 *   hist      uint32[nseg][GQ_TOPK_HIST_BINS]: ZERO when a compress starts; the compress leaves it zero again (the pick
 *             launches clear what they read), so a replayed graph of the launches needs no reset node
 *   state     int32[nseg][4]: per-tensor words of the select (threshold key, ties to keep); written before they are read
 *   counts    int32[nitems][2]: per-item counts, then their exclusive scans; written before they are read
 *   dense_table int64[ndense][3] = { source (float *), byte offset in ONE user's wire (a multiple of 4), elements }: the
 *             uncompressed tensors the compress launch copies into the wire as it is (gq_qsgd_batch.dense_table)
 * A decode needs seg_table and item_seg only.
 */
typedef struct gq_topk_batch {
    uint32_t struct_bytes;     /* sizeof(gq_topk_batch) */
    int32_t nseg;
    int64_t nitems;
    const int64_t *seg_table;
    const int32_t *item_seg;
    uint32_t *hist;
    int32_t *state;
    int32_t *counts;
    const int64_t *dense_table;
    int32_t ndense;
    int32_t reserved;
} gq_topk_batch;

int gq_topk_abi_version(void);
const char *gq_topk_last_error(void);

/*
 * Select and compact, in eight launches (three 11/11/9-bit radix histogram passes with a per-tensor pick behind each, the
 * per-item counts, their scan, the write).  The launch arguments do not depend on the data: the sequence replays from a graph.
 * ef_scale not NaN: error feedback (ps_quantizer.py:35-39) -- every pass reads w = v + ef_scale * err (the product rounded,
 * then the sum), and the write launch stores w back into the source and err = w - decoded.
 * out != NULL: the dense decoded tensors  w * (kept ? 1 : 0)  at out + out offset (required with error feedback).
 */
int gq_topk_compress_batched(const gq_topk_batch *b, uint8_t *wire, float ef_scale, float *out, void *stream);

/*
 * Decode-mean of R payloads (payload r at gathered + r * user_stride_bytes) into out + out offset, one launch:
 *     out[i] = (+0 + c_0[i] + ... + c_{R-1}[i]) / R     payloads in order, a true division (gq_mean_rows' arithmetic)
 * where c_r[i] is the value payload r carries for index i, or +0 if it does not carry i.
 * plain (R == 1 only): the payload's values as they are (a -0 stays -0), +0 elsewhere, no division.
 */
int gq_topk_decode_sum_batched(const gq_topk_batch *b, const uint8_t *gathered, int64_t user_stride_bytes, int R, float *out,
                               int plain, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GQ_TOPK_H */
