/*
 * libgq_drive.so -- a rotated 1-bit gradient compressor (DRIVE: Vargaftik et al., NeurIPS 2021; EDEN, ICML 2022) on gfx950.
 *
 * A block of 256 elements is rotated by  H * diag(signs) / 16  (include/gq_mxr.h's randomized Hadamard rotation), the SIGN of every
 * rotated coordinate is kept -- one bit per element -- and ONE f32 scale S per block.  The decode is  S * R^-1 sign(R x).  With
 * S = |x|^2 / |R x|_1 the decode is unbiased over the rotation's randomness and <decode, x> = |x|^2 (up to rounding); with
 * S = |R x|_1 / 256 it has the least squared error of any scale.  1.125 bits per element on the wire, no draws at all.
 *
 * The conventions are include/gq_mx.h's: return codes (GQ_OK or a negative GQ_ERR_* of include/gq_hsq.h), gq_drive_last_error(),
 * every pointer but the descriptor is device memory, nothing allocated, no scratch, ONE launch per call, and every launch
 * argument depends on the layout alone, so both launches replay from a HIP graph with nothing to step.  seg_table, item_seg,
 * dense_table and items of GQ_MX_ITEM_ELEMS are exactly gq_mx.h's (the segment table's `first draw` column is not read).
 * Tensors are float32.  Everything below is defined to the bit.
 *
 * BLOCKS       GQ_DRIVE_BLOCK = 256 consecutive elements of the flattened tensor, starting at multiples of 256.  A tensor of n
 *              elements has nb = ceil(n / 256) blocks; the last one is filled with +0 up to 256, so EVERY block is rotated (this
 *              differs from gq_mxr.h, whose tail stays unrotated: a zero-padded block keeps <D, x> = |x|^2).  An item is
 *              GQ_MX_ITEM_ELEMS = 4096 elements = 16 blocks: nothing straddles an item or a tensor.
 *
 * SIGNS        gq_mxr.h's, word for word: four 64-bit words, element j (0 ... 255) of every block owns bit  j & 63  of
 *              signs[j >> 6].  The host side derives them from a seed as outputs 0 ... 3 of splitmix64 started at the seed:
 *                  state += 0x9E3779B97F4A7C15;  z = state;
 *                  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  output = z ^ (z >> 31)
 *              The library takes the words as they are (all-zero: the pure Hadamard transform).
 *
 * SIGNS, STEPPED   The *_stepped entry points take no words: `rotation` is the address of a device uint64[2] = { seed, step }, and
 *              word k (k = 0 ... 3) of a launch is output number 4 * step + k of the splitmix64 stream started at `seed`:
 *                  z = seed + (4 * step + k + 1) * 0x9E3779B97F4A7C15,  then the finaliser above (the two multiplications and
 *                  the three xor-shifts);  all arithmetic on uint64, mod 2^64.
 *              Step 0 gives exactly the fixed words of that seed.  Step t of seed s is step 0 of seed s + 4 t * 0x9E3779B97F4A7C15.
 *              The words repeat after 2^62 steps.  gq_drive_batch.signs is not read.  The launch reads the pair and never writes it:
 *              whoever owns it moves the step word between launches (gq_mean_rows and the step tails of libgq_hsq.so add one to
 *              the step word of every pair they are given), and a launch replayed from a HIP graph -- its argument is the pair's
 *              ADDRESS, which does not change -- rotates by the words of the step it finds.  The wire does not carry the step and
 *              does not change by a byte: every payload of one decode-mean must have been compressed at the same (seed, step), and
 *              the decode-mean must run at that (seed, step).  Everything below is the same, word for word, in both forms.
 *
 * SIGNS, PER STREAM   The *_streams entry points give every payload of one mean a rotation of its own (DRIVE and EDEN are schemes
 *              for distributed mean estimation with one private rotation per client: the errors of R users then average out even
 *              when their gradients are equal).  A stream sigma is a non-negative integer.  The sign words of (seed, step, sigma)
 *              are the STEPPED words of (seed_sigma, step), with
 *                  seed_0 = seed
 *                  seed_sigma = fin(seed + sigma * 0xD6E8FEB86659FD93)    for sigma >= 1
 *              fin: the finaliser above (the two multiplications and the three xor-shifts); all arithmetic on uint64, mod 2^64.
 *              Stream 0 is therefore exactly the stepped rotation, bit for bit.  `rotation` is the same device { seed, step } pair,
 *              ONE for the whole parameter list, read and never written.  compress takes its stream by value; payload r of a
 *              decode-mean is decoded under stream  first_stream + r.  The wire does not change by a byte.  Transforms, code, scale,
 *              wire section and decoded values below are the same, word for word, under the stream's words; the decode-mean is
 *              DECODE-MEAN, PER STREAM.
 *
 * FORWARD TRANSFORM of a block of w (w is g, or under error feedback w = g + ef_scale * err: the product rounded, then the sum,
 *              as in gq_mx.h) -- gq_mxr.h's, word for word:
 *     1. x_j = w_j with its sign bit xor-ed with the element's sign bit.  A bit operation.
 *     2. Eight butterfly stages t = 0, 1, ..., 7 IN THIS ORDER, stride h = 2^t: for every j with bit t clear
 *            (x_j, x_{j+h}) <- (x_j + x_{j+h}, x_j - x_{j+h})
 *        each ONE f32 addition or subtraction, rounded to nearest even, never contracted; a stage reads only the results of the
 *        stage before it.
 *     3. x'_j = x_j * 2^-4: one f32 multiplication.
 *
 * INVERSE TRANSFORM of a block y -- gq_mxr.h's, word for word: the same eight stages in the same order, then the multiplication
 *              by 2^-4, then the xor of the same sign bits.
 *
 * CODE         The code of element j is the IEEE sign bit of x'_j: a bit test, -0 gives 1.
 *
 * SCALE        L1 = the sum of |x'_j|, Q = the sum of x'_j * x'_j (each product ONE f32 multiplication, never fused into the
 *              additions), j = 0 ... 255.  Both sums run as a balanced tree in index order: level t = 0 ... 7 replaces every pair
 *              of neighbours at stride 2^t by their ONE f32 sum,  v_j <- v_j + v_{j + 2^t}  for j a multiple of 2^(t+1); the
 *              result is v_0 after level 7.  (Three levels inside a lane, five across the 32 lanes that own the block.)
 *     scale_mode GQ_DRIVE_UNBIASED (0):  S = Q / L1          scale_mode GQ_DRIVE_MSE (1):  S = L1 / 256.0f
 *              ONE f32 division, rounded to nearest even.  L1 == 0:  S = +0 (in both modes).
 *              Overflow and underflow follow IEEE: a Q that overflows gives S = +inf (no element of the block then decodes to a
 *              finite value), a Q that underflows to 0 gives S = +0.
 *
 * NON-FINITE   An infinity or a NaN among the x'_j of a block (from an infinity or a NaN in w, or from an overflow inside the
 *              stages) reaches L1:  L1 = +inf or a NaN  gives  S = the NaN 0x7fc00000  in both modes, and the whole block decodes
 *              to NaN.  The sign and payload of a NaN that an addition produces or passes on are the hardware's choice: the
 *              256 code bits of such a block (all written) and WHICH NaN a value decodes to -- there, in a block with S = +inf
 *              and wherever else the inverse transform meets inf - inf -- are not part of the contract; that it is a NaN is.
 *              Every other bit of every output is defined by this text.
 *
 * WIRE SECTION of one tensor (at a 16-byte aligned offset of ONE user's wire):
 *     nb * 32 bytes            the codes: element j of block b is bit  j & 7  of byte  32 b + (j >> 3)
 *     nb * 4 bytes             the scales: S of block b as a little-endian f32 at 4 b
 *     zero bytes up to a multiple of 16
 *     nb * 32 + _up(nb * 4) bytes (_up: to a multiple of 16), EVERY one of them written, the pad included, and the code bits of a
 *     last block behind element n - 1 too: they are the transform's own outputs.  The wire depends on the input alone.
 *     No launch loads a byte outside the sections it is given, and none stores one outside them (+ the dense tensors' copy).
 *     1.125 bits per element.
 *
 * DECODED VALUES of a section:  y_j = S of the block with its sign bit xor-ed with the code of element j  (j = 0 ... 255, the
 *              elements behind n - 1 of a last block included: the inverse transform needs all 256).
 *
 * COMPRESS     ONE launch writes the wire sections and the dense tensors' copy.  out != NULL: D = the first n elements of the
 *              inverse transform of y, at out + out offset.  ef_scale not NaN: w is stored back into the source and
 *              err = w - D (one f32 subtraction), in the same launch; a tensor whose error buffer is 0 is compressed without.
 *
 * DECODE-MEAN  ONE launch over R payloads.  In the rotated domain
 *                  m_j = (+0 + y_0j + ... + y_{R-1,j}) / (float)R        payloads ascending, a true division
 *              plain (R == 1 only):  m_j = y_0j as it is, no addition and no division.  Then ONE inverse transform, whatever R is;
 *              its first n elements go to out + out offset.  Every payload must have been compressed under the same sign words.
 *
 * DECODE-MEAN, PER STREAM   ONE launch over R payloads.  D_r = the inverse transform, under stream first_stream + r, of payload r's
 *              decoded values y_r: R inverse transforms per block and no addition in the rotated domain.  In the gradient's domain
 *                  m_j = (+0 + D_0j + ... + D_{R-1,j}) / (float)R        payloads ascending, one f32 addition each, a true division
 *              plain (R == 1 only):  m_j = D_0j as it is.  The first n elements go to out + out offset.  NON-FINITE is as above.
 */
#ifndef GQ_DRIVE_H
#define GQ_DRIVE_H

#include <stdint.h>

#include "gq_mx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GQ_DRIVE_ABI_VERSION 1
#define GQ_DRIVE_BLOCK 256        /* elements that share a scale: a rotation block */
#define GQ_DRIVE_UNBIASED 0       /* S = |x'|^2 / |x'|_1 */
#define GQ_DRIVE_MSE 1            /* S = |x'|_1 / 256 */

/* gq_mxr_batch's fields (include/gq_mx.h: the same tables) with scale_mode in the place of format; the kernels take the sign
 * words by value.  seg_table int64[nseg][8] = { source, n (>= 1), first item, wire offset (a multiple of 16), -, out offset
 * (floats), -, error buffer (0 = none) }.  Sources, error buffers and outputs need 4-byte alignment only. */
typedef struct gq_drive_batch {
    uint32_t struct_bytes;     /* sizeof(gq_drive_batch) */
    int32_t nseg;
    int64_t nitems;
    const int64_t *seg_table;
    const int32_t *item_seg;
    const int64_t *dense_table;
    int32_t ndense;
    int32_t scale_mode;        /* GQ_DRIVE_UNBIASED or GQ_DRIVE_MSE */
    uint64_t signs[4];
} gq_drive_batch;

int gq_drive_abi_version(void);
const char *gq_drive_last_error(void);

/*
 * The codes and scales of every tensor into `wire` (16-byte aligned; + the dense tensors' copy), ONE launch.  ef_scale not NaN:
 * error feedback; out != NULL (4-byte aligned): the dense decode D.
 * Refused (nothing is launched): a descriptor of another size, scale_mode outside {0, 1}, bad sizes, a null table, a null or
 * misaligned wire, a misaligned out.
 */
int gq_drive_compress_batched(const gq_drive_batch *b, uint8_t *wire, float ef_scale, float *out, void *stream);

/*
 * Decode-mean of R payloads (payload r at gathered + r * user_stride_bytes, any alignment) into out + out offset, ONE launch.
 * Refused: as above, null pointers, R < 1, a negative stride with R > 1, plain with R != 1.
 */
int gq_drive_decode_sum_batched(const gq_drive_batch *b, const uint8_t *gathered, int64_t user_stride_bytes, int R, float *out, int plain,
                                void *stream);

/*
 * The same two launches under SIGNS, STEPPED: `rotation` is the device { seed, step } pair (8-byte aligned), b->signs is not read.
 * ONE launch per call, no scratch, every launch argument depends on the layout alone.  Refused: everything the calls above
 * refuse, and a null or misaligned rotation.
 */
int gq_drive_compress_batched_stepped(const gq_drive_batch *b, const uint64_t *rotation, uint8_t *wire, float ef_scale, float *out,
                                      void *stream);
int gq_drive_decode_sum_batched_stepped(const gq_drive_batch *b, const uint64_t *rotation, const uint8_t *gathered,
                                        int64_t user_stride_bytes, int R, float *out, int plain, void *stream);

/*
 * The same two launches under SIGNS, PER STREAM: `rotation` is the device { seed, step } pair (8-byte aligned), b->signs is not read;
 * `stream` / `first_stream` are passed by value, payload r of the gather decodes under stream first_stream + r (DECODE-MEAN, PER
 * STREAM).  ONE launch per call, no scratch, no LDS, every launch argument depends on the layout and the wire slot alone.  Refused:
 * everything the stepped calls refuse, a negative stream or first_stream, and first_stream + R overflowing int32.
 */
int gq_drive_compress_batched_streams(const gq_drive_batch *b, const uint64_t *rotation, int32_t stream, uint8_t *wire, float ef_scale, float *out,
                                      void *stream_handle);
int gq_drive_decode_sum_batched_streams(const gq_drive_batch *b, const uint64_t *rotation, int32_t first_stream, const uint8_t *gathered,
                                        int64_t user_stride_bytes, int R, float *out, int plain, void *stream_handle);

#ifdef __cplusplus
}
#endif
#endif /* GQ_DRIVE_H */
