/*
 * libgq_sketch.so -- a count-sketch compressor on gfx950 (Sketched-SGD, Ivkin et al. 2019; FetchSGD, Rothchild et al. 2020): the one
 * wire of this family that ADDS.  The sketches of R users add cell by cell into the sketch of their sum; the heavy hitters of the
 * mean are recovered once, whatever R is.
 *
 * Conventions of include/gq_topk.h:
 *   - return value: GQ_OK (0) or a negative GQ_ERR_* code (values of include/gq_hsq.h); gq_sketch_last_error() gives text;
 *   - every pointer is device memory except the descriptor itself (and the arguments of gq_sketch_build_lists, which are host
 *     memory); work goes to `stream` (a hipStream_t, NULL = default);
 *   - nothing is allocated inside: the caller owns every table and every scratch buffer the descriptor names;
 *   - every launch argument depends on the layout and the seed alone: both sequences replay from a HIP graph;
 *   - float32 tensors only, no draws, no atomics of any kind on floats: the bytes depend on the input alone.
 *
 * PER TENSOR   n elements, 4096 * 2 * rows <= n < 2^31.  An item is GQ_SKETCH_CHUNK = 4,096 consecutive elements; item a holds the
 *              elements [4096 a, min(n, 4096 (a + 1))), position t = 0 .. 4095 inside it; items = ceil(n / 4096).
 *              rows r in {1, 3, 5}.  A row is nwin WINDOWS of exactly 4,096 f32 cells, nwin = max(1, ceil(items / (C * r))), C the
 *              host's cell ratio.  A tensor is sketched only if 2 * r * nwin <= items (the host sends any other as it is).
 *
 * HASH         a function of (seed, row j, item a, position t) alone.  G = 0x9E3779B97F4A7C15, M = 0xD6E8FEB86659FD93, fin = the
 *              splitmix64 finaliser (z ^= z >> 30, z *= 0xBF58476D1CE4E5B9, z ^= z >> 27, z *= 0x94D049BB133111EB, z ^= z >> 31),
 *              all sums and products mod 2^64:
 *                  K_j      = fin(seed + (j + 1) * G)                            the row's key
 *                  A_j      = ((K_j >> 20) & 0xfff) | 1                          an odd 12-bit multiplier
 *                  H_j(a)   = fin(K_j + (a + 1) * G)
 *                  window   = ((H_j(a) >> 32) * nwin) >> 32                      multiply-high of the high half
 *                  off      = H_j(a) & 0xfff
 *                  cell     = (A_j * t + off) & 0xfff                            a bijection of the item's positions onto the window
 *                  S_j(a,g) = fin(K_j + ((a << 6) + g + 1) * M),  g = t >> 6     one finaliser per 64 elements
 *                  sign     = bit (t & 63) of S_j(a, t >> 6): the element enters as bits(w) ^ (sign << 31), i.e. w * (+-1), exactly
 *              Two elements of one item never share a cell.  Two items of one row share a window with probability 1 / nwin, and then
 *              EVERY position of the one meets exactly one position of the other: the structure's price is that the collisions of
 *              an item pair are correlated across positions; rows are independent through K_j.
 *
 * SUM ORDER    The items of window (j, v) in ascending order form its LIST; the list is cut into CHUNKS of GQ_SKETCH_CHUNK_ITEMS = 8
 *              entries.  Per cell:   partial_c = (((+0 + x_0) + x_1) + ... )   over the chunk's entries in list order,
 *                                    cell      = (((+0 + partial_0) + partial_1) + ... )   in chunk order,
 *              x = the signed element that maps to the cell.  A position past the tensor's end enters as +0 (signed like any other).
 *              No sum that starts at +0 is ever -0 under round-to-nearest, so such a term -- and a term -0 -- changes nothing: a
 *              tensor of -0 alone, a window without items and a last item of one element all give cells of +0 where nothing else falls.
 *
 * WIRE SECTION of one tensor, at a 4-byte aligned offset of ONE user's wire: a 16-byte header { n u32, r u32, nwin u32, 0 }, then
 *              r * nwin * 4096 f32, row-major (row j, window v, cell).  EVERY byte is written by a compress; a compress writes the
 *              sections, the dense copies of dense_table and no other byte of the wire.
 *
 * DECODE-MEAN  T[cell] = ((+0 + c_0) + ... + c_{R-1}) / (float)R    payloads in order, a true division;
 *              with error accumulation (etab != NULL, plain == 0)   T[cell] = T[cell] + E[cell]   after the division.
 *              est_i = median over j of  sign_j(i) * T_j[cell_j(i)]  (the sign flips the value's sign bit).  With cx(x, y) =
 *              "if (y < x) swap x and y" (an f32 compare: false for a NaN, false between -0 and +0):
 *                  r = 1   the value
 *                  r = 3   cx(0,1) cx(1,2) cx(0,1)                                      -> p[1]
 *                  r = 5   cx(0,1) cx(3,4) cx(0,3) cx(1,4) cx(1,2) cx(2,3) cx(1,2)      -> p[2]      (p[j] = row j's value)
 *              KEPT SET: top-k's (include/gq_topk.h) on the estimates, k from the segment table: key = bits(est) & 0x7fffffff, a NaN
 *              as 0x7fffffff; the k largest keys, of the keys equal to the k-th largest the lowest indices.
 *              out_i = est_i where kept, +0 elsewhere.
 *              Then, with error accumulation:  E[cell] = T[cell] - sketch(out)[cell], sketch() the compress with SUM ORDER's sums.
 *
 * CHUNKED RECOVERY (recover == GQ_SKETCH_RECOVER_CHUNKED; GQ_SKETCH_MIN_CR <= cr <= GQ_SKETCH_MAX_CR).  T, est and E as above; the
 *              KEPT SET alone differs: it is PER ITEM.  Item a of len elements keeps its own kt = len / cr (integer division) largest
 *              keys, key as above (bits(est) & 0x7fffffff, a NaN as 0x7fffffff, so above +inf); of the keys equal to the item's
 *              kt-th largest, the lowest element indices.  kt == 0 (a last item shorter than cr): the item keeps nothing.
 *              out_i = est_i where kept (the estimate's own bits, a -0 included), +0 elsewhere.  The k of the segment table is not
 *              read.  A tensor keeps sum over its items of len / cr <= n / cr elements.
 */
#ifndef GQ_SKETCH_H
#define GQ_SKETCH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GQ_SKETCH_ABI_VERSION 2      /* 2: gq_sketch_batch ends with { recover, cr } */
#define GQ_SKETCH_CHUNK 4096         /* elements per item, cells per window */
#define GQ_SKETCH_CHUNK_ITEMS 8      /* list entries per chunk */
#define GQ_SKETCH_HEADER_BYTES 16    /* n, r, nwin, 0 in front of a section's cells */
#define GQ_SKETCH_HIST_BINS 2048     /* histogram words per tensor (the select of include/gq_topk.h) */
#define GQ_SKETCH_MAX_ROWS 5
#define GQ_SKETCH_RECOVER_GLOBAL 0   /* the tensor's k largest estimates */
#define GQ_SKETCH_RECOVER_CHUNKED 1  /* every item's own len / cr largest estimates */
#define GQ_SKETCH_MIN_CR 2           /* cr of the chunked recovery */
#define GQ_SKETCH_MAX_CR 4096
#define GQ_SKETCH_BATCH_BYTES_V1 168 /* the descriptor without { recover, cr }: GQ_SKETCH_RECOVER_GLOBAL */

/*
 * The tensors of one group.  W = the group's windows, numbered tensor by tensor, row-major inside a tensor; U = its units (a unit
 * is one chunk of one window's list), the units of a window consecutive and in chunk order.
 *   seg_table int64[nseg][8] = { source (float *), n, first item, wire offset (bytes, a multiple of 4), k, out offset (floats),
 *                                nwin, 0 }
 *   item_seg  int32[nitems]: the tensor of every item
 *   lay       int64[nseg]: the tensor's first window
 *   win_tab   int32[W][4] = { tensor, first unit, chunks (0: a window without items), 0 }
 *   unit_tab  int32[U][4] = { window, first entry in `list`, entries (1 .. 8), 0 }
 *   list      uint32[...]: an entry is  item + (off << 19)  (gq_sketch_build_lists)
 *   part      float[U][4096]: the chunks' partial sums;  table float[W][4096]: T;  est float[out floats]: the estimates
 *   dec_table int64[nseg][8]: seg_table with source = est + out offset (the select's launches read it)
 *   hist      uint32[nseg][GQ_SKETCH_HIST_BINS], zero; a decode leaves it zero again.  state int32[nseg][4], counts int32[nitems][2]
 *             part, table, est, state and counts are written before they are read: garbage in them changes nothing.
 *   etab      int64[nseg]: E of every tensor (float *, r * nwin * 4096 each), or NULL: no error accumulation
 *   dense_table int64[ndense][3]: gq_topk_batch.dense_table
 * A compress needs seg_table, lay, win_tab, unit_tab, list, part (and everything else where it is asked for `out`).
 *   recover, cr  the last two fields.  struct_bytes tells the two layouts apart: GQ_SKETCH_BATCH_BYTES_V1 (a caller built against
 *             version 1) is read as GQ_SKETCH_RECOVER_GLOBAL.  Under GQ_SKETCH_RECOVER_CHUNKED est, dec_table, hist, state and counts
 *             are not read and may be NULL; cr is read in that mode alone.
 */
typedef struct gq_sketch_batch {
    uint32_t struct_bytes;     /* sizeof(gq_sketch_batch) */
    int32_t nseg;
    int64_t nitems;
    const int64_t *seg_table;
    const int32_t *item_seg;
    const int64_t *lay;
    const int32_t *win_tab;
    const int32_t *unit_tab;
    const uint32_t *list;
    float *part;
    float *table;
    float *est;
    const int64_t *dec_table;
    uint32_t *hist;
    int32_t *state;
    int32_t *counts;
    const int64_t *etab;
    const int64_t *dense_table;
    int32_t ndense;
    int32_t rows;
    int64_t nwindows;
    int64_t nunits;
    uint64_t seed;
    int32_t recover;           /* GQ_SKETCH_RECOVER_* */
    int32_t cr;                /* GQ_SKETCH_RECOVER_CHUNKED: an item keeps len / cr elements */
} gq_sketch_batch;

int gq_sketch_abi_version(void);
const char *gq_sketch_last_error(void);

/*
 * HOST memory, no device work: the lists of one tensor of `items` items.  list[rows * items]: the entries window by window (row j,
 * window v), ascending items inside a window; starts[rows * nwin + 1]: the first entry of every window, then rows * items.
 */
int gq_sketch_build_lists(uint64_t seed, int rows, int64_t items, int64_t nwin, uint32_t *list, int64_t *starts);

/*
 * Two launches: the sketch launch (a workgroup per unit: the chunk's items staged through LDS, 16 cells per thread in registers)
 * and the fold launch (a workgroup per window: the chunks in order, the header, the dense copies).  ef_scale must be NaN (this
 * compressor keeps no per-user residual).  out != NULL: also the decode-mean of this one payload WITHOUT error accumulation at
 * out + out offset (eleven launches more; two under GQ_SKETCH_RECOVER_CHUNKED).
 */
int gq_sketch_compress_batched(const gq_sketch_batch *b, uint8_t *wire, float ef_scale, float *out, void *stream);

/*
 * DECODE-MEAN of R payloads (payload r at gathered + r * user_stride_bytes, 4-byte aligned) into out + out offset: the sum launch,
 * the estimate launch, the select's six, count, scan, store -- and with error accumulation (etab != NULL and plain == 0) the sketch
 * and fold launches once more, E = T - sketch(out).  plain (R == 1 only): one payload's decode, E neither read nor written.
 * Under GQ_SKETCH_RECOVER_CHUNKED the sum launch and ONE recover launch (a workgroup per item: the rows' windows through LDS, the
 * median, a radix select of the item's kt-th largest key in a 256-bin LDS histogram, the dense store) stand for the first eleven.
 */
int gq_sketch_decode_sum_batched(const gq_sketch_batch *b, const uint8_t *gathered, int64_t user_stride_bytes, int R, float *out,
                                 int plain, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GQ_SKETCH_H */
