/*
 * libgq_thr.so -- threshold sparsification with a fitted (or a given) threshold on gfx950: a sparse wire with a variable count and
 * no select.  Keeps what exceeds a threshold eta; eta is either the caller's or fitted to the tail of |w| in `stages` O(n) passes
 * (a count-adaptive multi-stage peaks-over-threshold exponential fit, after SIDCo, Abdelmoniem et al., MLSys 2021).
 *
 * Conventions of include/gq_topk.h:
 *   - return value: GQ_OK (0) or a negative GQ_ERR_* code (values of include/gq_hsq.h); gq_thr_last_error() gives text;
 *   - every pointer is device memory except the descriptor itself; work goes to `stream` (a hipStream_t, NULL = default);
 *   - nothing is allocated inside: the caller owns every scratch buffer the descriptor names;
 *   - every launch argument depends on the layout (and the caller's eta) alone: the whole sequence replays from a HIP graph;
 *   - float32 tensors only, no draws, no float or double atomics: the bytes depend on the input alone.
 *
 * PER TENSOR   n elements, 1 <= n < 2^31.  k = n // cr >= 1 (the host computes it; the library refuses k < 1).
 *              cap = min(n, (k * P + 99) // 100) >= 1, P the host's capacity percentage: an integer of the segment table.
 *              m >= 1: the fit stride, from the segment table.
 *              w = v, or with error feedback v + ef_scale * err (the product rounded to f32, then the sum).
 *              key(w) = bits(w) & 0x7fffffff, every NaN mapped to 0x7fffffff (include/gq_topk.h).
 *              An item is GQ_THR_CHUNK = 4,096 consecutive elements; item j of a tensor holds elements [4096 j, min(n, 4096 (j+1))).
 *
 * KEPT SET     Element i is EXCEEDING iff key(w_i) > bits(eta), an integer compare.  eta is an f32 with +0 <= eta <= FLT_MAX, so an
 *              infinity or a NaN always exceeds and +-0 never does.  found = the number of exceeding elements; kept = the first
 *              min(found, cap) exceeding elements in index order.  decoded_i = w_i * (kept ? 1 : 0), as top-k decodes.
 *
 * FIXED MODE   stages == 0: eta is the caller's, one f32 per launch sequence.  Anything not in [+0, FLT_MAX] (a negative value,
 *              -0, an infinity, a NaN) is refused.
 *
 * FITTED MODE  stages == S, 1 ... GQ_THR_MAX_STAGES.  eta_0 = +0.  For s = 1 ... S:
 *     1. Over the FIT ITEMS of the tensor -- the items j with j % m == 0, n_fit elements in total --
 *            c_s     = the number of elements with bits(eta_{s-1}) < key < 0x7f800000   (finite, above eta_{s-1})
 *            Sigma_s = the sum of  (double)|w| - (double)eta_{s-1}  over those elements: ONE f64 subtraction per element.
 *     2. The order of the f64 additions in Sigma_s:
 *          inside an item: a balanced tree in index order over 4,096 slots, slot i = element i's term, or +0.0 where the element
 *            does not count or lies past n.  Level t = 0 ... 11 replaces  v_j <- v_j + v_{j + 2^t}  for j a multiple of 2^(t+1);
 *            the item's sum is v_0 after level 11 (include/gq_drive.h's tree, in f64);
 *          across the fit items, ascending (fit item q is item q * m): the same balanced tree over Q slots, Q the smallest power
 *            of two >= the number of fit items, padded with +0.0.
 *        Counts are integers; their order is free.
 *     3. c^ = ((double)c_s * (double)n) / (double)n_fit          (the product rounded, then ONE division)
 *     4. c_s == 0 or c^ <= (double)k:  eta_s = eta_{s-1}.
 *     5. Otherwise
 *            beta = Sigma_s / (double)c_s                         (ONE division; not a multiplication by 1 / c_s)
 *            L    = gq_ln(c^ / (double)k) / (double)(S - s + 1)   (two divisions)
 *            t    = (double)eta_{s-1} + beta * L                  (the product rounded, then the sum: never fused)
 *            eta_s = t rounded to f32, to nearest even; an eta_s that is not finite (t above FLT_MAX's rounding range, or not
 *            finite) is replaced by 0x7f7fffff (FLT_MAX).
 *     6. eta = eta_S.
 *
 * gq_ln(x)     for a finite f64 x >= 1, a fixed sequence of f64 +, -, *, / with no library call:
 *            e = (bits(x) >> 52) - 1023;  mant = the f64 with x's 52 fraction bits and the exponent field 1023 (1 <= mant < 2);
 *            if bits(mant) > GQ_LN_SQRT2 (0x3FF6A09E667F3BCD):  mant = mant * 0.5, e = e + 1      (sqrt(1/2) < mant <= sqrt(2))
 *            z = (mant - 1.0) / (mant + 1.0);   y = z * z;
 *            p = C[11];  for j = 10 ... 0:  p = p * y, then p = p + C[j]       (Horner, 12 terms, each operation rounded)
 *            gq_ln = (double)e * GQ_LN_LN2  +  (2.0 * z) * p                   ((2.0 * z) first, then * p, then the sum)
 *        C[j] = the f64 nearest 1 / (2j + 1):
 *            C[0]  0x3FF0000000000000   C[1]  0x3FD5555555555555   C[2]  0x3FC999999999999A   C[3]  0x3FC2492492492492
 *            C[4]  0x3FBC71C71C71C71C   C[5]  0x3FB745D1745D1746   C[6]  0x3FB3B13B13B13B14   C[7]  0x3FB1111111111111
 *            C[8]  0x3FAE1E1E1E1E1E1E   C[9]  0x3FAAF286BCA1AF28   C[10] 0x3FA8618618618618   C[11] 0x3FA642C8590B2164
 *        GQ_LN_LN2 = 0x3FE62E42FEFA39EF.  |z| <= 0.1716, so the first dropped term is below 2e-20 of the sum: the relative error
 *        against the true logarithm stays far below 1e-13 (tests/test_thr_contract.py bounds it).
 *        The kernels compute it with these operations (the file is built with -ffp-contract=off).
 *
 * WIRE SECTION of one tensor, at a 16-byte aligned offset of ONE user's wire -- GQ_THR_HEADER_BYTES + 8 cap bytes, then zero bytes
 *              up to a multiple of 16:
 *            16-byte header  { kept u32, found u32, bits(eta) u32, 0 }
 *            cap x u32 index, ascending; cap x f32 value (bits of w)
 *            the slots from `kept` on hold index 0xffffffff and value +0.
 *        EVERY byte of the section is written by a compress; a compress writes the sections, the dense copies of dense_table and no
 *        other byte of the wire.
 */
#ifndef GQ_THR_H
#define GQ_THR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GQ_THR_ABI_VERSION 1
#define GQ_THR_CHUNK 4096        /* elements per item */
#define GQ_THR_HEADER_BYTES 16   /* kept, found, bits(eta), 0 in front of a section's indices */
#define GQ_THR_MAX_STAGES 8
#define GQ_THR_NO_INDEX 0xffffffffu   /* the index of a slot that holds no pair */

/*
 * The tensors of one group, table-driven like gq_topk_batch: ONE launch per stage serves all of them.
 *   seg_table int64[nseg][8] = { source (float *), n, first item, wire offset (bytes, a multiple of 16), k, out offset (floats),
 *                                cap + (m << 32), error buffer (float *, 0 = none) }
 *   item_seg  int32[nitems]: the tensor of every item; the items of tensor s are first .. first + ceil(n / GQ_THR_CHUNK) - 1
 *   sums      double[nitems]: the fit items' Sigma of the current stage
 *   state     int32[nseg][4]: { bits(eta), found, -, - }
 *   counts    int32[nitems][2]: { the fit count of the current stage, the exceeding count and then its exclusive scan }
 *             sums, state and counts are written before they are read: garbage in them changes nothing.
 *   dense_table int64[ndense][3] = { source (float *), byte offset in ONE user's wire (a multiple of 4), elements }: the
 *             uncompressed tensors the write launch copies into the wire as they are (gq_topk_batch.dense_table)
 *   stages    0: fixed mode; 1 ... GQ_THR_MAX_STAGES: fitted mode
 *   min_k, min_cap, min_stride: the smallest k, cap and m of the table, as the host that built it knows them.  The library cannot
 *             read the table, which is device memory, so it refuses on these (each < 1: nothing is launched); the launches take
 *             the table as given.
 * A decode needs seg_table and item_seg only.
 */
typedef struct gq_thr_batch {
    uint32_t struct_bytes;     /* sizeof(gq_thr_batch) */
    int32_t nseg;
    int64_t nitems;
    const int64_t *seg_table;
    const int32_t *item_seg;
    double *sums;
    int32_t *state;
    int32_t *counts;
    const int64_t *dense_table;
    int32_t ndense;
    int32_t stages;
    int32_t min_k;
    int32_t min_cap;
    int32_t min_stride;
    int32_t reserved;
} gq_thr_batch;

int gq_thr_abi_version(void);
const char *gq_thr_last_error(void);

/*
 * Fit and compact: `stages` times { the reduce launch over all tensors' fit items, the pick launch (one workgroup per tensor:
 * eta_s) }, then count, scan, write -- 2 * stages + 3 launches; fixed mode runs the last three only, with the caller's eta.
 * The write launch stores the pairs, the header and the pad slots, the dense-copy tensors, with out != NULL the decoded tensors
 * w * (kept ? 1 : 0) at out + out offset, and with ef_scale not NaN (error feedback; needs out)  v <- w  and  err = w - decoded.
 * wire: 16-byte aligned; out: 4-byte aligned.  eta is read in fixed mode only.
 */
int gq_thr_compress_batched(const gq_thr_batch *b, uint8_t *wire, float eta, float ef_scale, float *out, void *stream);

/*
 * Decode-mean of R payloads (payload r at gathered + r * user_stride_bytes, any 4-byte alignment) into out + out offset, one launch:
 *     out[i] = (+0 + c_0[i] + ... + c_{R-1}[i]) / (float)R     payloads in order, a true division
 * where c_r[i] is the value payload r carries for index i, or +0 if it does not carry i.  Of payload r the first
 * min(kept, cap) slots are read, kept from its header: a corrupt count cannot run past the section.
 * plain (R == 1 only, refused otherwise): the payload's values as they are (a -0 stays -0), +0 elsewhere, no division.
 */
int gq_thr_decode_sum_batched(const gq_thr_batch *b, const uint8_t *gathered, int64_t user_stride_bytes, int R, float *out, int plain,
                              void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GQ_THR_H */
