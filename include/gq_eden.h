/*
 * libgq_eden.so -- a rotated 2-, 3- or 4-bit gradient compressor (EDEN: Vargaftik et al., ICML 2022, DRIVE's sequel) on gfx950.
 *
 * A block of 256 elements is rotated by  H * diag(signs) / 16  (include/gq_mxr.h's randomized Hadamard rotation).  After the
 * rotation a block's coordinates are close to Gaussian whatever the gradient looked like, so every coordinate is replaced by the
 * nearest of the 2^b Lloyd-Max centroids of N(0, 1), scaled by the block's own spread -- b bits per element -- and ONE f32 scale S
 * per block is kept.  The decode is  S * R^-1 (+-c_m).  With S = |x|^2 / <|R x|, c_m> the decode is unbiased over the rotation's
 * randomness and <decode, x> = |x|^2 (up to rounding); with S = <|R x|, c_m> / |c_m|^2 it has the least squared error of any scale.
 * b + 0.125 bits per element on the wire, no draws at all.  One bit is libgq_drive.so (include/gq_drive.h).
 *
 * The conventions are include/gq_mx.h's: return codes (GQ_OK or a negative GQ_ERR_* of include/gq_hsq.h), gq_eden_last_error(),
 * every pointer but the descriptor is device memory, nothing allocated, no scratch, ONE launch per call, and every launch
 * argument depends on the layout alone, so both launches replay from a HIP graph with nothing to step.  seg_table, item_seg,
 * dense_table and items of GQ_MX_ITEM_ELEMS are exactly gq_mx.h's (the segment table's `first draw` column is not read).
 * Tensors are float32.  Everything below is defined to the bit.
 *
 * BLOCKS       GQ_EDEN_BLOCK = 256 consecutive elements of the flattened tensor, starting at multiples of 256.  A tensor of n
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
 * SIGNS, STEPPED   include/gq_drive.h's, word for word.  The *_stepped entry points take no words: `rotation` is the address of a
 *              device uint64[2] = { seed, step }, and word k (k = 0 ... 3) of a launch is output number 4 * step + k of the
 *              splitmix64 stream started at `seed`:
 *                  z = seed + (4 * step + k + 1) * 0x9E3779B97F4A7C15,  then the finaliser above (the two multiplications and
 *                  the three xor-shifts);  all arithmetic on uint64, mod 2^64.
 *              Step 0 gives exactly the fixed words of that seed.  Step t of seed s is step 0 of seed s + 4 t * 0x9E3779B97F4A7C15.
 *              The words repeat after 2^62 steps.  gq_eden_batch.signs is not read.  The launch reads the pair and never writes it:
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
 * SUMS         Every sum over a block's 256 values below runs as a balanced tree in index order: level t = 0 ... 7 replaces every
 *              pair of neighbours at stride 2^t by their ONE f32 sum,  v_j <- v_j + v_{j + 2^t}  for j a multiple of 2^(t+1); the
 *              result is v_0 after level 7.  (Three levels inside a lane, five across the 32 lanes that own the block.)
 *
 * BITS         b = 2, 3 or 4 (gq_eden_batch.bits).  Anything else is refused.
 *
 * TABLES       L = 2^(b-1) magnitudes c_0 < ... < c_{L-1} and L - 1 thresholds t_0 < ... < t_{L-2}: float32 constants given by
 *              their bit patterns -- the float32 nearest to the Lloyd-Max fixed point of N(0, 1) (c_i the mean of |z| on its cell,
 *              t_i = (c_i + c_{i+1}) / 2 taken in float64).  The bit patterns are the contract:
 *     b = 2    c = 0x3ee7d2c9 0x3fc1555d                                        (0.452780 1.510418)
 *              t = 0x3f7b4a0f                                                   (0.981599)
 *     b = 3    c = 0x3e7af9f8 0x3f418990 0x3fac0538 0x4009b97a                  (0.245094 0.756005 1.343909 2.151946)
 *              t = 0x3f002407 0x3f866500 0x3fdfbc17                             (0.500550 1.049957 1.747927)
 *     b = 4    c = 0x3e0379fd 0x3ec6ae44 0x3f28215e 0x3f713d39 0x3fa0cc2f 0x3fcf1c25 0x40046ac7 0x402ee2bf
 *                                                (0.128395 0.388048 0.656759 0.942340 1.256231 1.618046 2.069017 2.732590)
 *              t = 0x3e8435a1 0x3f05bc40 0x3f4caf4b 0x3f8cb566 0x3fb7f42a 0x3febf8da 0x4019a6c3
 *                                                (0.258222 0.522404 0.799550 1.099286 1.437139 1.843532 2.400803)
 *
 * SPREAD       Q = the sum of x'_j * x'_j (each product ONE f32 multiplication, never fused into the additions).
 *              sigma = sqrtf(Q * 2^-8): ONE f32 multiplication, then ONE correctly rounded f32 square root.
 *
 * CODE         theta_i = t_i * sigma, ONE f32 multiplication each.  m_j = the number of i with |x'_j| > theta_i: the compare is
 *              strict, |.| clears the sign bit.  code_j = m_j | (IEEE sign bit of x'_j) << (b - 1); a -0 has sign 1.
 *
 * SCALE        P = the sum of |x'_j| * c_{m_j}, C2 = the sum of c_{m_j} * c_{m_j} (each product ONE f32 multiplication).
 *     scale_mode GQ_EDEN_UNBIASED (0):  S = Q / P           scale_mode GQ_EDEN_MSE (1):  S = P / C2
 *              ONE f32 division, rounded to nearest even.  (At one magnitude c = 1 these are DRIVE's Q / L1 and L1 / 256.)
 *              P == 0:  S = +0 (in both modes).
 *              Overflow and underflow follow IEEE: a Q that overflows with P finite gives sigma = +inf, every m_j = 0, and
 *              S = +inf in the unbiased mode (no element of the block then decodes to a finite value), a finite P / C2 in mse;
 *              a Q that underflows to 0 with P > 0 gives sigma = 0, every nonzero |x'_j| the top magnitude, and S = +0 in the
 *              unbiased mode, P / C2 in mse.
 *
 * NON-FINITE   An infinity or a NaN among the x'_j of a block (from an infinity or a NaN in w, or from an overflow inside the
 *              stages) reaches P:  P = +inf or a NaN  gives  S = the NaN 0x7fc00000  in both modes, and the whole block decodes
 *              to NaN.  The sign and payload of a NaN that an addition produces or passes on are the hardware's choice: the
 *              256 codes of such a block (all written) and WHICH NaN a value decodes to -- there, in a block with S = +inf
 *              and wherever else the inverse transform meets inf - inf -- are not part of the contract; that it is a NaN is.
 *              Every other bit of every output is defined by this text.
 *
 * WIRE SECTION of one tensor (at a 16-byte aligned offset of ONE user's wire):
 *     nb * 32 b bytes          the codes: element j of block k owns bits  b j ... b j + b - 1  of that block's string of 32 b
 *                              bytes read as one little-endian number (bit i of the string: bit i & 7 of byte i >> 3).  A lane's
 *                              eight codes are therefore b whole bytes, at byte b * lane of the block.
 *     nb * 4 bytes             the scales: S of block k as a little-endian f32 at 4 k
 *     zero bytes up to a multiple of 16
 *     nb * 32 b + _up(nb * 4) bytes (_up: to a multiple of 16), EVERY one of them written, the pad included, and the codes of a
 *     last block behind element n - 1 too: they are the transform's own outputs.  The wire depends on the input alone.
 *     No launch loads a byte outside the sections it is given, and none stores one outside them (+ the dense tensors' copy).
 *     b + 0.125 bits per element.
 *
 * DECODED VALUES of a section:  y_j = (S * c_{m_j}), ONE f32 multiplication, with its sign bit xor-ed with the code's sign bit
 *              (j = 0 ... 255, the elements behind n - 1 of a last block included: the inverse transform needs all 256).
 *
 * COMPRESS     ONE launch writes the wire sections and the dense tensors' copy.  out != NULL: D = the first n elements of the
 *              inverse transform of y, at out + out offset.  ef_scale not NaN: w is stored back into the source and
 *              err = w - D (one f32 subtraction), in the same launch; a tensor whose error buffer is 0 is compressed without.
 *
 * DECODE-MEAN  ONE launch over R payloads.  In the rotated domain
 *                  m_j = (+0 + y_0j + ... + y_{R-1,j}) / (float)R        payloads ascending, a true division
 *              plain (R == 1 only):  m_j = y_0j as it is, no addition and no division.  Then ONE inverse transform, whatever R is;
 *              its first n elements go to out + out offset.  Every payload must have been compressed under the same sign words
 *              and the same bits.
 *
 * DECODE-MEAN, PER STREAM   ONE launch over R payloads.  D_r = the inverse transform, under stream first_stream + r, of payload r's
 *              decoded values y_r: R inverse transforms per block and no addition in the rotated domain.  In the gradient's domain
 *                  m_j = (+0 + D_0j + ... + D_{R-1,j}) / (float)R        payloads ascending, one f32 addition each, a true division
 *              plain (R == 1 only):  m_j = D_0j as it is.  The first n elements go to out + out offset.  NON-FINITE is as above.
 */
#ifndef GQ_EDEN_H
#define GQ_EDEN_H

#include <stdint.h>

#include "gq_mx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GQ_EDEN_ABI_VERSION 1
#define GQ_EDEN_BLOCK 256        /* elements that share a scale: a rotation block */
#define GQ_EDEN_UNBIASED 0       /* S = Q / P */
#define GQ_EDEN_MSE 1            /* S = P / C2 */
#define GQ_EDEN_MIN_BITS 2
#define GQ_EDEN_MAX_BITS 4

/* gq_drive_batch's fields (include/gq_drive.h: the same tables) plus bits; the sign words stay last, the kernels take them by
 * value.  seg_table int64[nseg][8] = { source, n (>= 1), first item, wire offset (a multiple of 16), -, out offset (floats), -,
 * error buffer (0 = none) }.  Sources, error buffers and outputs need 4-byte alignment only. */
typedef struct gq_eden_batch {
    uint32_t struct_bytes;     /* sizeof(gq_eden_batch) */
    int32_t nseg;
    int64_t nitems;
    const int64_t *seg_table;
    const int32_t *item_seg;
    const int64_t *dense_table;
    int32_t ndense;
    int32_t scale_mode;        /* GQ_EDEN_UNBIASED or GQ_EDEN_MSE */
    int32_t bits;              /* 2, 3 or 4 */
    int32_t reserved;          /* 0 */
    uint64_t signs[4];
} gq_eden_batch;

int gq_eden_abi_version(void);
const char *gq_eden_last_error(void);

/*
 * The codes and scales of every tensor into `wire` (16-byte aligned; + the dense tensors' copy), ONE launch.  ef_scale not NaN:
 * error feedback; out != NULL (4-byte aligned): the dense decode D.
 * Refused (nothing is launched): a descriptor of another size, bits outside {2, 3, 4}, scale_mode outside {0, 1}, bad sizes, a
 * null table, a null or misaligned wire, a misaligned out.
 */
int gq_eden_compress_batched(const gq_eden_batch *b, uint8_t *wire, float ef_scale, float *out, void *stream);

/*
 * Decode-mean of R payloads (payload r at gathered + r * user_stride_bytes, any alignment) into out + out offset, ONE launch.
 * Refused: as above, null pointers, R < 1, a negative stride with R > 1, plain with R != 1.
 */
int gq_eden_decode_sum_batched(const gq_eden_batch *b, const uint8_t *gathered, int64_t user_stride_bytes, int R, float *out, int plain,
                               void *stream);

/*
 * The same two launches under SIGNS, STEPPED: `rotation` is the device { seed, step } pair (8-byte aligned), b->signs is not read.
 * ONE launch per call, no scratch, every launch argument depends on the layout alone.  Refused: everything the calls above
 * refuse, and a null or misaligned rotation.
 */
int gq_eden_compress_batched_stepped(const gq_eden_batch *b, const uint64_t *rotation, uint8_t *wire, float ef_scale, float *out,
                                     void *stream);
int gq_eden_decode_sum_batched_stepped(const gq_eden_batch *b, const uint64_t *rotation, const uint8_t *gathered,
                                       int64_t user_stride_bytes, int R, float *out, int plain, void *stream);

/*
 * The same two launches under SIGNS, PER STREAM: `rotation` is the device { seed, step } pair (8-byte aligned), b->signs is not read;
 * `stream` / `first_stream` are passed by value, payload r of the gather decodes under stream first_stream + r (DECODE-MEAN, PER
 * STREAM).  ONE launch per call, no scratch, no LDS, every launch argument depends on the layout and the wire slot alone.  Refused:
 * everything the stepped calls refuse, a negative stream or first_stream, and first_stream + R overflowing int32.
 */
int gq_eden_compress_batched_streams(const gq_eden_batch *b, const uint64_t *rotation, int32_t stream, uint8_t *wire, float ef_scale, float *out,
                                     void *stream_handle);
int gq_eden_decode_sum_batched_streams(const gq_eden_batch *b, const uint64_t *rotation, int32_t first_stream, const uint8_t *gathered,
                                       int64_t user_stride_bytes, int R, float *out, int plain, void *stream_handle);

#ifdef __cplusplus
}
#endif
#endif /* GQ_EDEN_H */
