/*
 * libgq_dgc.so -- momentum correction and momentum factor masking around the top-k select (Deep Gradient Compression, Lin et
 * al. 2018, section 3.2) on gfx950.  The select, the compaction, the wire and the decode-mean are libgq_topk.so's
 * (include/gq_topk.h), unchanged; this library adds the two elementwise launches around the select.
 *
 * A library of its own next to libgq_topk.so, with the same conventions:
 *   - return value: GQ_OK (0) or a negative GQ_ERR_* code (values of include/gq_hsq.h); gq_dgc_last_error() gives text;
 *   - every pointer is device memory except the descriptor itself; work goes to `stream` (a hipStream_t, NULL = default);
 *   - nothing is allocated inside, and no launch argument depends on the data: the launches replay from a graph.
 *
 * Per compressed tensor (n elements, k = n // cr) and per local user slot: state u and v, two f32 buffers of n elements that
 * start at +0, and a scratch buffer s of n elements (any content).  One record, with g the gradient (read only) and m the
 * momentum; every operation is ONE f32 operation rounded to nearest, never contracted:
 *
 *     t  = m * u_old
 *     u1 = t + g                                   gq_dgc_accumulate_batched: u <- u1, s <- u1
 *     v1 = v_old + u1                              gq_topk_compress_batched(ef_scale = 1) over the state table: source s,
 *     kept set, wire section, decoded =            error buffer v -- its w = s + 1 * v is v1 (f32 addition commutes, and
 *         gq_topk.h's rule applied to v1           1 * v is v); it stores err = w - decoded into v
 *     v_new = v1 - decoded                         (+0 where kept and finite, NaN where kept and not finite)
 *     u_new = kept ? +0 : u1                       gq_dgc_mask_batched: u[index] <- +0 for the k indices of the wire section
 *
 * The wire is top-k's, byte for byte: gq_topk_decode_sum_batched decodes it.  Where an operation above yields a NaN, which NaN
 * (sign, payload) is not part of the contract.
 */
#ifndef GQ_DGC_H
#define GQ_DGC_H

#include <stdint.h>

#include "gq_topk.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GQ_DGC_ABI_VERSION 1

/*
 * The tensors of one group.  Items are GQ_TOPK_CHUNK elements: item_seg and the `first item` column are the ones of the
 * gq_topk_batch that runs the select between the two launches.
 *   grad_table  int64[nseg][8]: column 0 = the gradient (const float *, 4-byte aligned); the other columns are not read.  The
 *               only table that follows the gradients' addresses.
 *   state_table int64[nseg][8] = { s (float *), n, first item, wire offset (bytes, a multiple of 16), k, out offset, u (float *),
 *               v (float *) } -- as it stands the seg_table of the select's gq_topk_batch (column 6 is free there, column 7 its
 *               error buffer).  One per user slot; nothing in it changes from record to record.
 *   item_seg    int32[nitems]: the tensor of every item
 */
typedef struct gq_dgc_batch {
    uint32_t struct_bytes;     /* sizeof(gq_dgc_batch) */
    int32_t nseg;
    int64_t nitems;
    const int64_t *grad_table;
    const int64_t *state_table;
    const int32_t *item_seg;
} gq_dgc_batch;

int gq_dgc_abi_version(void);
const char *gq_dgc_last_error(void);

/* One launch over all items: u1 = m * u + g (two roundings) into u and into s.  m must not be NaN. */
int gq_dgc_accumulate_batched(const gq_dgc_batch *b, float m, void *stream);

/*
 * One launch over all items, behind the select that wrote `wire` (the same user's wire): item j of a tensor reads the indices
 * [j * GQ_TOPK_CHUNK, min(k, (j + 1) * GQ_TOPK_CHUNK)) of the tensor's section and stores +0 into u there.  An index that is
 * not below n (a wire that no select wrote) is skipped.
 */
int gq_dgc_mask_batched(const gq_dgc_batch *b, const uint8_t *wire, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GQ_DGC_H */
