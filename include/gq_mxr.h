/*
 * libgq_mxr.so -- the block-scaled small-float compressor of include/gq_mx.h behind a randomized Hadamard rotation, on gfx950.
 *
 * A block of 32 elements shares one power-of-two scale taken from its largest magnitude, so one large entry sets the grid for
 * its 31 neighbours.  A rotation by  H * diag(signs) / 16  (H the 256-point Walsh-Hadamard matrix, entries +-1) in front of the
 * quantiser spreads such an entry over 256 elements; the inverse rotation behind the decode brings the values back.  The
 * rotation is orthogonal, so stochastic rounding stays unbiased, and it is additions only.
 *
 * The conventions are include/gq_mx.h's: return codes, gq_mxr_last_error(), nothing allocated, no scratch, ONE launch per call,
 * and every launch argument depends on the layout alone, so both launches replay from a HIP graph.  seg_table, item_seg,
 * dense_table, items of GQ_MX_ITEM_ELEMS, formats (the two 6-bit ones and their zero pad included), wire sections, draw numbering
 * and random modes are exactly gq_mx.h's: the wire format does not change, and a receiver needs the same sign words to decode.
 *
 * ROTATION BLOCK   GQ_MXR_BLOCK = 256 consecutive elements of the flattened tensor, starting at multiples of 256.  A tensor of n
 *              elements has n / 256 (integer) rotated blocks; its last n % 256 elements are NOT rotated (a tensor below 256
 *              elements is plain MX).  A rotation block is 8 whole MX blocks, an item is 16 whole rotation blocks: nothing
 *              straddles an item or a tensor.
 *
 * SIGNS        Four 64-bit words: element j (0 ... 255) of every rotation block owns bit  j & 63  of  signs[j >> 6].
 *              The host side derives them from a seed as outputs 0 ... 3 of splitmix64 started at the seed (uint64 arithmetic):
 *                  state += 0x9E3779B97F4A7C15;  z = state;
 *                  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  output = z ^ (z >> 31)
 *              The library takes the words as they are (all-zero: the pure Hadamard transform).
 *
 * FORWARD TRANSFORM of a rotation block of w (w is g, or g + ef_scale * err exactly as in gq_mx.h):
 *     1. x_j = w_j with its sign bit xor-ed with the element's sign bit.  A bit operation: NaN payloads and zeros just flip sign.
 *     2. Eight butterfly stages t = 0, 1, ..., 7 IN THIS ORDER, stride h = 2^t: for every j with bit t clear
 *            (x_j, x_{j+h}) <- (x_j + x_{j+h}, x_j - x_{j+h})
 *        each ONE f32 addition or subtraction, rounded to nearest even, never contracted; a stage reads only the results of the
 *        stage before it.
 *     3. x'_j = x_j * 2^-4: one f32 multiplication, exact unless the result is subnormal, and then it is that one rounding.
 *     Non-finite values and overflow follow IEEE arithmetic: an infinity or a NaN anywhere in a rotation block reaches all 256
 *     outputs (inf - inf), hence scale byte 0xFF in all 8 MX blocks.
 *
 * COMPRESS     The wire section is, bit for bit, what gq_mx_compress_batched writes for the tensor x' with the same draws; x' is
 *              the rotated blocks followed by the unrotated tail, and element i of x' owns draw  first draw + i.
 *
 * INVERSE TRANSFORM of a rotation block of a decoded tensor y: the same eight stages in the same order, then the multiplication
 *              by 2^-4, then the xor of the same sign bits.  The tail passes through unchanged.  H * H = 256 * I: in exact
 *              arithmetic this inverts the forward transform.
 *
 * DENSE DECODE AND ERROR FEEDBACK of the compress launch:  D = the inverse transform of the decoded values of the codes just
 *              written; `out` receives D; with error feedback w is stored back into the source and err = w - D, same launch.
 *
 * DECODE-MEAN  m = the value gq_mx_decode_sum_batched defines (+0 start, payloads ascending, a true division by (float)R; plain
 *              with R == 1 leaves d_0 as it is); `out` receives the inverse transform of m -- the mean first, then ONE inverse
 *              rotation, whatever R is.
 *
 * TENSOR-SIDE TYPE  gq_mx.h's, for the *_bf16 entry points: bf16 sources are widened (exact) in front of the forward transform, and
 *              everything above runs on the widened values.  narrow (gq_mx.h, to the bit) applies at the same three stores, and
 *              what it rounds is the INVERSE TRANSFORM's f32 output: D into the compress launch's `out`, the inverse transform
 *              of m into the decode-mean's `out`; under error feedback w goes back into the source narrowed and err = w - D
 *              from the unrounded w.  The inverse transform's output is a sum of 256 terms and fits no 8-bit significand in
 *              general: with rotation a plain decode is rounded like any f32.  The wire is the f32 twin's, byte for byte.
 */
#ifndef GQ_MXR_H
#define GQ_MXR_H

#include <stdint.h>

#include "gq_mx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GQ_MXR_ABI_VERSION 2
#define GQ_MXR_BLOCK 256          /* elements of a rotation block: 8 MX blocks */

/* gq_mx_batch's fields (include/gq_mx.h: the same tables), then the sign words; the kernels take the words by value. */
typedef struct gq_mxr_batch {
    uint32_t struct_bytes;     /* sizeof(gq_mxr_batch) */
    int32_t nseg;
    int64_t nitems;
    const int64_t *seg_table;
    const int32_t *item_seg;
    const int64_t *dense_table;
    int32_t ndense;
    int32_t format;            /* GQ_MX_FP4, GQ_MX_FP8, GQ_MX_FP6_E2M3 or GQ_MX_FP6_E3M2 */
    uint64_t signs[4];
} gq_mxr_batch;

int gq_mxr_abi_version(void);
const char *gq_mxr_last_error(void);

/* gq_mx_compress_batched over the rotated tensors (arguments and refusals as there); out and the residual are inverse-rotated. */
int gq_mxr_compress_batched(const gq_mxr_batch *b, uint8_t *wire, int random_mode, const float *r, uint64_t seed, float ef_scale,
                            float *out, void *stream);

/* gq_mx_decode_sum_batched, then one inverse rotation of the mean (arguments and refusals as there). */
int gq_mxr_decode_sum_batched(const gq_mxr_batch *b, const uint8_t *gathered, int64_t user_stride_bytes, int R, float *out, int plain,
                              void *stream);

/* The two launches over bf16 tensors (TENSOR-SIDE TYPE above; arguments and refusals as the f32 twins', `out` 2-byte aligned). */
int gq_mxr_compress_batched_bf16(const gq_mxr_batch *b, uint8_t *wire, int random_mode, const float *r, uint64_t seed, float ef_scale,
                                 uint16_t *out, void *stream);
int gq_mxr_decode_sum_batched_bf16(const gq_mxr_batch *b, const uint8_t *gathered, int64_t user_stride_bytes, int R, uint16_t *out,
                                   int plain, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GQ_MXR_H */
