/*
 * libgq_psgd.so -- low-rank gradient compression (Vogels, Karimireddy, Jaggi, "PowerSGD: Practical Low-Rank Gradient
 * Compression for Distributed Optimization", NeurIPS 2019) on gfx950, rank r = 1, 2 or 4: one power iteration per record
 * from a warm start, modified Gram-Schmidt, error feedback.
 *
 * A library of its own with the conventions of include/gq_topk.h:
 *   - return value: GQ_OK (0) or a negative GQ_ERR_* code (values of include/gq_hsq.h); gq_psgd_last_error() gives text;
 *   - every pointer is device memory except the descriptor itself; work goes to `stream` (a hipStream_t, NULL = default);
 *   - nothing is allocated inside: the caller owns every scratch buffer the descriptor names.
 *
 * A tensor is the row-major matrix M of n rows and m columns (1 <= n, m; n * m < 2^31; r <= min(n, m)).  Its state is the
 * warm start Q, m x r float32, row-major (Q[c * r + j]).  Every operation below is ONE IEEE float32 operation, round to
 * nearest even, subnormals kept; fmaf(a, b, c) is a * b + c with one rounding; nothing else is fused.
 *
 * THE TREE.  tree(x) of 256 values:  for h = 128, 64, 32, 16, 8, 4, 2, 1:  x[t] = x[t] + x[t + h] for every t < h;  the
 * result is x[0].  dot(a, b) over L index values i = 0 ... L - 1:  x[t] = +0.0f, then for i = t, t + 256, t + 512, ... < L in
 * ascending order  x[t] = fmaf(a[i], b[i], x[t]);  dot = tree(x).  (256 accumulators, strided; slots that own no index stay +0.)
 *
 * A RECORD of one tensor, in order:
 *   1. M' = M + s * e   under error feedback (s = ef_scale; the product rounded, then the sum), else M' = M.
 *   2. P[i][j], a row being cut into pieces of GQ_PSGD_PIECE columns (the last one shorter; one piece when m <= GQ_PSGD_PIECE):
 *          piece q of row i:  pp[q] = dot(M'[i][c], Q[c][j]) over the columns c of the piece, ascending from the piece's first
 *          P[i][j] = pp[0], then P[i][j] = P[i][j] + pp[q] for q = 1, 2, ... in order.
 *   3. Modified Gram-Schmidt, columns left to right.  For j = 0 ... r - 1:
 *          for k = 0 ... j - 1 in order:  d = dot(Ph[:, k], P[:, j]) over the rows;  P[i][j] = fmaf(-d, Ph[i][k], P[i][j])
 *          nrm[j] = sqrtf(dot(P[:, j], P[:, j]))          -- a correctly rounded square root
 *          Ph[i][j] = P[i][j] / (nrm[j] + 1e-8f)          -- a correctly rounded division; a zero column stays zero
 *          reset[j] = nrm[j] is exactly 0, infinite or NaN   (nrm[j] is the norm the column is divided by, i.e. of what the
 *                     earlier columns left of it: a column that depends on them linearly and leaves exactly nothing resets too)
 *   4. Q'[c][j], the rows being cut into blocks of GQ_PSGD_ROW_BLOCK rows (the last one shorter):
 *          block b:  part[b] = +0.0f, then for the rows i of the block in ascending order  part[b] = fmaf(M'[i][c], Ph[i][j], part[b])
 *          Q'[c][j] = part[0], then Q'[c][j] = Q'[c][j] + part[b] for b = 1, 2, ... in order.
 *   5. The wire section (below) takes Ph and Q'.
 *   6. The warm start becomes Q', except that column j goes back to Q0[:, j] where reset[j] (a single all-zero gradient would
 *      otherwise pin the column at zero for the rest of the run).  The wire carries Q' as computed.
 *          Q0[c][j] = 2.0f * uniform01(seed, ((uint64)key << 32) | (c * r + j)) - 1.0f     (exact: a multiple of 2^-23 in [-1, 1))
 *      uniform01 is the library family's counter hash (csrc/gq_common.hpp), key = (parameter index << 12) | user, user < 4096.
 *   7. D[i][c] = Ph[i][0] * Q'[c][0], then D[i][c] = fmaf(Ph[i][j], Q'[c][j], D[i][c]) for j = 1 ... r - 1;  e = M' - D.
 *
 * DECODE-MEAN of R payloads:  out[i][c] = (D_0[i][c] + D_1[i][c] + ... + D_{R-1}[i][c]) / (float)R, every D_rho formed as in 7
 * from payload rho's factors, then added in row order (D_0 first, no +0 in front), a true division.
 *
 * NON-FINITE VALUES.  Nothing is special-cased: a NaN or an infinity in M, e or Q travels through the operations above as IEEE
 * arithmetic takes it (NaN out wherever a NaN reaches).  WHICH NaN pattern comes out is not defined: two results are equal when
 * they agree bit for bit on every value that is not a NaN and are both NaN elsewhere.
 *
 * Wire section of one tensor (at a 16-byte aligned offset of ONE user's wire), every byte written by every compress:
 *     uint32 { n, m, r, 0 }
 *     float  Ph[n][r]
 *     float  Q'[m][r]
 *     zero bytes up to a multiple of 16            GQ_PSGD_SECTION_BYTES(n, m, r)
 *
 * No float atomics anywhere: the bytes depend on M, e, Q and the arguments alone, not on the grid or on scheduling.
 */
#ifndef GQ_PSGD_H
#define GQ_PSGD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GQ_PSGD_ABI_VERSION 1
#define GQ_PSGD_PIECE 4096          /* columns per piece of a long row */
#define GQ_PSGD_ROW_BLOCK 64        /* rows per block of the back-projection; also the rows of a tile */
#define GQ_PSGD_TILE_COLS 256       /* columns per tile */
#define GQ_PSGD_HEADER_BYTES 16
#define GQ_PSGD_MAX_USERS 4096      /* user < 4096 in the key of Q0; the two-phase server's warm start is user 4095 */
#define GQ_PSGD_SECTION_BYTES(n, m, r) ((GQ_PSGD_HEADER_BYTES + 4 * (int64_t)(r) * ((int64_t)(n) + (int64_t)(m)) + 15) / 16 * 16)

/*
 * Tables (device memory), s = tensor of the group:
 *   seg_table  int64[nseg][8] = { M (const float *), n * m, first tile, byte offset of the section in ONE user's wire (a multiple
 *              of 16), n, offset in `out` (floats), 0, e (float *; error feedback) }
 *   item_seg   int32[nitems]: the tensor of every TILE.  A tensor has ceil(n / 64) * ceil(m / 256) tiles, row block major:
 *              tile t = row block t / ceil(m / 256), column tile t % ceil(m / 256).  Launches (C), (C'), (D) and the decode run
 *              one workgroup per tile.
 *   lay        int64[nseg][4] = { first item, offset in pwork (floats), offset in cpart (floats), key of Q0 without the user
 *              (parameter index << 12) }
 *   aitem_seg  int32[naitems]: the tensor of every ITEM of launch (A).  m <= 4096: an item is max(1, 4096 / m) whole rows, a
 *              tensor has ceil(n / that) items.  m > 4096: an item is one piece of one row, item = row * pieces + piece.
 *   state      int64[nseg][2] = { Q (float *, 4-byte aligned), user }: ONE user's warm starts
 *   pwork      float: a tensor owns n * pieces * r values (the pieces' partial sums, [row][piece][j])
 *   cpart      float: a tensor owns ceil(n / 64) * m * r values (the row blocks' partial sums, [block][c][j])
 *   flags      int32[nseg][4]: reset[j]
 *   dense_table int64[ndense][3] = { source (float *), byte offset in ONE user's wire (a multiple of 4), elements }: the
 *              uncompressed tensors launch (A) copies into the wire as they are
 * Scratch is written before it is read in every compress: what it held before plays no part.  A decode needs seg_table and
 * item_seg only.
 */
typedef struct gq_psgd_batch {
    uint32_t struct_bytes;     /* sizeof(gq_psgd_batch) */
    int32_t nseg;
    int64_t nitems;            /* tiles */
    const int64_t *seg_table;
    const int32_t *item_seg;
    const int64_t *lay;
    const int32_t *aitem_seg;
    int64_t naitems;
    const int64_t *state;
    float *pwork;
    float *cpart;
    int32_t *flags;
    const int64_t *dense_table;
    int32_t ndense;
    int32_t rank;              /* r: 1, 2 or 4, of every tensor of the group */
    uint64_t seed;             /* of Q0 */
} gq_psgd_batch;

int gq_psgd_abi_version(void);
const char *gq_psgd_last_error(void);

/*
 * One record of the state table's user for every tensor of the group: launches (A) project, (B) orthogonalise, (C)
 * back-project, (C') fold, and (D) residual where asked for.  The launch arguments do not depend on the data: the sequence
 * replays from a graph.
 * ef_scale not NaN: error feedback -- (A) reads M' = M + ef_scale * e and stores it into e, (C) and (D) read it there, (D)
 * stores e = M' - D.  M itself is never written.
 * out != NULL: the dense decode D at out + out offset, by (D).  (D) is launched under error feedback or when out != NULL.
 */
int gq_psgd_compress_batched(const gq_psgd_batch *b, uint8_t *wire, float ef_scale, float *out, void *stream);

/*
 * Decode-mean of R payloads (payload rho at gathered + rho * user_stride_bytes) into out + out offset, one launch; see
 * DECODE-MEAN above.  n and r are the TABLE's, whatever the payloads' headers say: no byte outside the sections is read and none
 * outside `out` is written.  `plain` is accepted for the family's signature and changes nothing (x / 1.0f is x).
 */
int gq_psgd_decode_sum_batched(const gq_psgd_batch *b, const uint8_t *gathered, int64_t user_stride_bytes, int R, float *out,
                               int plain, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GQ_PSGD_H */
