/*
 * libgq_mx.so -- a block-scaled small-float gradient compressor (OCP Microscaling: MXFP4 / MXFP6 / MXFP8) on gfx950.
 *
 * A library of its own next to libgq_hsq.so, with the conventions of libgq_sign.so and libgq_maurey.so:
 *   - return value: GQ_OK (0) or a negative GQ_ERR_* code (values of include/gq_hsq.h); gq_mx_last_error() gives text;
 *   - every pointer is device memory except the descriptor itself; work goes to `stream` (a hipStream_t, NULL = default);
 *   - nothing is allocated inside and there is no scratch: a compress is ONE launch, a decode-mean is ONE launch, and every
 *     launch argument depends on the layout alone, so both replay from a HIP graph.
 *
 * 32 consecutive elements of the flattened tensor share one power-of-two scale byte (E8M0); every element is one small float.
 * Everything below is defined to the bit: the scale is a power of two, so the decode is exact, and the rounding of an element
 * is a comparison of two exact f32 values.
 *
 * FORMATS      format 0  FP4 E2M1        bits 4, mb 1, bias 1, emax 2, magnitude codes 0..7   (cmax 7,   mag 6)
 *              format 1  FP8 E4M3 (OCP)  bits 8, mb 3, bias 7, emax 8, magnitude codes 0..126 (cmax 126, mag 448); no
 *                        infinities; magnitude code 127 (the format's NaN) is never written
 *              format 0x23  FP6 E2M3     bits 6, mb 3, bias 1, emax 2, magnitude codes 0..31  (cmax 31,  mag 7.5)
 *              format 0x32  FP6 E3M2     bits 6, mb 2, bias 3, emax 4, magnitude codes 0..31  (cmax 31,  mag 28)
 *                        (the ids of the 6-bit formats: exponent bits, mantissa bits as hex digits; neither has infinities
 *                        or NaNs, every one of the 64 codes is a value)
 *     mag(c) = c * 2^(1-bias-mb)                                      for c < 2^mb  (the format's subnormals)
 *     mag(c) = (2^mb + (c & (2^mb - 1))) * 2^((c >> mb) - bias - mb)  otherwise;    strictly increasing in c
 *     A code is  sign << (bits - 1) | c,  sign = the element's own sign bit (+-0 keep their sign).
 *
 * BLOCKS       A tensor of n elements is nb = ceil(n / 32) blocks; the ragged end is padded with +0.  w is the gradient, or
 *              under error feedback w = g + ef_scale * err (the product rounded, then the sum; -ffp-contract=off).
 *
 * BLOCK EXPONENT (integers only)
 *     a = the largest  bits(w_i) & 0x7fffffff  of the block
 *     a >= 0x7f800000 (an infinity or a NaN in the block): the scale byte is 0xFF and EVERY code of the block is 0; every
 *              element of the block decodes to the NaN 0x7fc00000.
 *     otherwise  E = a >> 23,  M = a & 0x7fffff,  ea = E ? E - 127 : -126,
 *              over = E != 0 && M > MTHR,   MTHR = 0x400000 (FP4: 1.5), 0x600000 (FP8, FP6 E3M2: 1.75) or 0x700000 (FP6 E2M3: 1.875),
 *              e = max(ea - emax + over, -127),   scale byte = e + 127   (0 ... 253).
 *     Then |w_i| * 2^-e <= mag(cmax) for every element: nothing is ever clamped.  An all-zero block gets byte 0.
 *
 * ELEMENT      y = ldexp(|w|, -e)         one rounding (to nearest even); exact unless the result is subnormal
 *              q = 2^(1-bias-mb) if y < 2^(1-bias), else 2^(floor(log2 y) - mb)
 *              t = y / q,  k = trunc(t),  frac = t - k         both exact (f32)
 *              c_lo = the code with mag(c_lo) = k * q;  the element's code is c_lo or c_lo + 1:
 *              with draws   up iff frac > r                     (an f32 comparison, strict, as in QSGD)
 *              random_mode GQ_RANDOM_OFF   up iff frac > 0.5 || (frac == 0.5 && (c_lo & 1))   nearest, ties to the even code
 *     c_lo + 1 is taken only where frac > 0, so the code never exceeds cmax.
 *
 * DRAWS        (modes and seed handling of include/gq_maurey.h)
 *     GQ_RANDOM_GIVEN           r is a caller's f32 buffer: element i of tensor s reads r[first draw + i]
 *     GQ_RANDOM_DEVICE          r = the library's counter-based generator at (seed, first draw + i): j * 2^-24, j = 0 ... 2^24 - 1
 *     GQ_RANDOM_DEVICE_COUNTER  seed is the address of a device { seed, step } pair (uint64[2]): a replay draws afresh once
 *                               the step word has moved (gq_mean_rows / a step tail of libgq_hsq.so moves it)
 *     With the generator's r, P(up) = ceil(frac * 2^24) / 2^24: the compressor is unbiased to within 2^-24 of a grid step q.
 *
 * WIRE SECTION of one tensor (at a 16-byte aligned offset of ONE user's wire):
 *     _up(nb) bytes               the scale bytes, block b at byte b; zero bytes up to _up(nb)     (_up: to a multiple of 16)
 *     FP4: 16 bytes per block     element 2i in the low nibble of byte i, element 2i + 1 in the high nibble
 *     FP8: 32 bytes per block     element i in byte i
 *     FP6: 24 bytes per block     the codes of block b are the 24 bytes at 24 b; read as a 192-bit little-endian bit string,
 *                                 element i occupies bits 6i .. 6i+5 (the convention of GQ_LEVELS_PACKED6)
 *     zero bytes up to a multiple of 16 (FP6 with an odd nb: 8 bytes; none otherwise)
 *     The codes of the padding elements are 0.  The section, _up(nb) + _up(16 nb), _up(nb) + _up(24 nb) or _up(nb) + _up(32 nb)
 *     bytes, is a multiple of 16, and EVERY byte of it is written, that pad included: the wire depends on the input (and the
 *     draws) alone.
 *     No launch loads a byte outside the sections it is given, and none stores one outside them (+ the dense tensors' copy).
 *
 * DECODE       An element's value is  +-ldexp(mag(c), e),  e = scale byte - 127: one exact scaling -- for every code and every
 *              scale byte a compress writes the result is representable (subnormal results included) unless it reaches 2^128,
 *              which ldexp gives as +-inf (a block whose maximum is within half a grid step of 2^128 can round up to it).
 *              Scale byte 0xFF: the NaN 0x7fc00000 for every element of the block, whatever its codes are.  A decode reads
 *              the FP8 magnitude code 127, which no compress writes, by the same formula (480 * 2^e).
 *
 * TENSOR-SIDE TYPE  T is float (the entry points above all) or bf16 (the *_bf16 entry points; an f16 could follow, none exists).  T is
 *              the type of four things: the sources, the compress launch's `out`, the decode-mean's `out` and the dense-copy
 *              sources.  Error buffers, given draws r and the wire stay f32, f32 and bytes: THE WIRE DOES NOT CHANGE -- the payload
 *              of a bf16 source is, byte for byte, the payload of the f32 launch on the widened tensor, and a bf16 rank and an
 *              f32 rank exchange payloads freely.
 *     widen(h)   the f32 with the bits h << 16: exact, NaNs and signed zeros included.  Everything above that is defined on w
 *              (block exponent, element code, draws, error feedback w = g + ef_scale * err) is computed on widened values,
 *              unchanged.
 *     narrow(x)  round to nearest even onto bf16, in integers on b = bits(x):
 *                  (b & 0x7fffffff) > 0x7f800000 (a NaN):  0x7FC0
 *                  otherwise:                              (b + 0x7FFF + ((b >> 16) & 1)) >> 16
 *              The second rule carries into the exponent, reaches +-inf at the top and rounds f32 subnormals onto bf16's grid as
 *              they are (what a CPU float32 -> bfloat16 cast of torch does).
 *     narrow applies at every store of an f32 value into a T location: the compress launch's `out`, the source written back
 *              under error feedback, the decode-mean's `out`.  Under error feedback the residual keeps full precision:
 *              err = w - decoded from the UNROUNDED w; only the copy written back into the source is narrowed.  The decode-mean
 *              computes its f32 result exactly as above and narrows once, at the store.
 *     Exactness: every value ONE payload decodes to has a significand of at most 2 (FP4) or 4 (both FP6, E4M3) bits, which fits
 *              bf16's 8: a plain decode is exact in bf16 unless the value has a bit below 2^-133 (bf16's smallest subnormal),
 *              where bf16's subnormal grid rounds it -- possible only below 2^-130 (FP4: 2^-132), under the scale bytes 0 ... 6.
 *              A mean of several payloads is rounded like any f32.
 *     Alignment: T locations need the alignment of T only (2 bytes).  A lane's 8 elements are ONE 16-byte access where they are
 *              16-byte aligned and scalar accesses otherwise -- the f32 rule, where they are two.  The segment table's out
 *              offset counts elements of T.  The dense-copy table of a bf16 compress launch names bf16 sources (2-byte
 *              aligned), which it widens into the wire's f32 dense region.
 */
#ifndef GQ_MX_H
#define GQ_MX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GQ_MX_ABI_VERSION 2
#define GQ_MX_BLOCK 32            /* elements that share a scale byte */
#define GQ_MX_ITEM_ELEMS 4096     /* elements (128 blocks) per item: every launch walks a tensor in items of this size */
#define GQ_MX_FP4 0
#define GQ_MX_FP8 1
#define GQ_MX_FP6_E2M3 0x23
#define GQ_MX_FP6_E3M2 0x32

/*
 * The tensors of one group, table-driven like gq_sign_batch: ONE launch serves all of them.
 *   seg_table int64[nseg][8] = { source (float *), n (>= 1), first item, wire offset (bytes, a multiple of 16), -,
 *                                out offset (floats), first draw, error buffer (float *, 0 = none) }
 *   item_seg  int32[nitems]: the tensor of every item; the items of tensor s are first .. first + ceil(n / GQ_MX_ITEM_ELEMS) - 1
 *   dense_table int64[ndense][3] = { source (float *), byte offset in ONE user's wire (a multiple of 4), elements }: the
 *             uncompressed tensors the compress launch copies into the wire as they are (gq_sign_batch.dense_table)
 * Sources, error buffers and outputs need 4-byte alignment only (16-byte aligned runs take float4 accesses).
 */
typedef struct gq_mx_batch {
    uint32_t struct_bytes;     /* sizeof(gq_mx_batch) */
    int32_t nseg;
    int64_t nitems;
    const int64_t *seg_table;
    const int32_t *item_seg;
    const int64_t *dense_table;
    int32_t ndense;
    int32_t format;            /* GQ_MX_FP4, GQ_MX_FP8, GQ_MX_FP6_E2M3 or GQ_MX_FP6_E3M2 */
} gq_mx_batch;

int gq_mx_abi_version(void);
const char *gq_mx_last_error(void);

/*
 * The scale bytes and codes of every tensor into `wire` (16-byte aligned; + the dense tensors' copy), ONE launch.
 * random_mode: GQ_RANDOM_OFF, GQ_RANDOM_GIVEN (r), GQ_RANDOM_DEVICE (seed) or GQ_RANDOM_DEVICE_COUNTER (seed = an address).
 * ef_scale not NaN: error feedback (ps_quantizer.py:35-39) -- w = g + ef_scale * err, w is stored back into the source and
 * err = w - decoded, in the same launch (a tensor whose error buffer is 0 is compressed without).  Otherwise the source is
 * only read.
 * out != NULL: the dense decoded tensor at out + out offset.
 */
int gq_mx_compress_batched(const gq_mx_batch *b, uint8_t *wire, int random_mode, const float *r, uint64_t seed, float ef_scale,
                           float *out, void *stream);

/*
 * Decode-mean of R payloads (payload r at gathered + r * user_stride_bytes, any alignment) into out + out offset, one launch:
 *     out[i] = (+0 + d_0[i] + ... + d_{R-1}[i]) / (float)R     payloads in ascending order, a true division
 * plain (R == 1 only): d_0 as it is, no addition and no division (a -0 stays -0).  With R > 1 `plain` is ignored: the mean.
 */
int gq_mx_decode_sum_batched(const gq_mx_batch *b, const uint8_t *gathered, int64_t user_stride_bytes, int R, float *out, int plain,
                             void *stream);

/*
 * The two launches over bf16 tensors (TENSOR-SIDE TYPE above): sources, `out` and dense-copy sources are bf16, every other
 * argument, the wire and the refusals are the f32 twin's -- except that `out` may be 2-byte aligned.
 */
int gq_mx_compress_batched_bf16(const gq_mx_batch *b, uint8_t *wire, int random_mode, const float *r, uint64_t seed, float ef_scale,
                                uint16_t *out, void *stream);
int gq_mx_decode_sum_batched_bf16(const gq_mx_batch *b, const uint8_t *gathered, int64_t user_stride_bytes, int R, uint16_t *out,
                                  int plain, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GQ_MX_H */
