/*
 * libgq_sign.so -- signSGD (SignSGDCompressor, signsgd_compressor.py:4-12) on gfx950, on a 2-bit wire.
 *
 * A library of its own next to libgq_hsq.so and libgq_topk.so, with their conventions:
 *   - return value: GQ_OK (0) or a negative GQ_ERR_* code (values of include/gq_hsq.h); gq_sign_last_error() gives text;
 *   - every pointer is device memory except the descriptor itself; work goes to `stream` (a hipStream_t, NULL = default);
 *   - nothing is allocated inside; every launch argument depends on the layout alone, so the launches replay from a graph.
 *
 * The reference compresses with torch.sign(v) and decompresses with the identity.  What torch.sign gives on an MI355X (ROCm
 * torch 2.10, measured on ±0, ±NaN with payloads, ±inf, ±min subnormal, ±FLT_MAX, ±1) is what it gives on the CPU:
 *     sign(+0) = sign(-0) = +0,  sign(NaN) = +0 for either sign and any payload,  sign(x) = ±1 for every other x
 *     (±inf and subnormals included).  It never returns -0 or NaN.
 * So three codes carry every decoded value and the wire loses nothing.
 *
 * Wire section of one tensor of n elements (at a 16-byte aligned offset of ONE user's wire): _up(ceil(n / 16) * 4) bytes,
 * _up(x) = x rounded up to a multiple of 16.  Element i sits in bits 2*(i%16) .. 2*(i%16)+1 of the little-endian uint32
 * word i/16 (equivalently: bits 2*(i%4) .. of byte i/4), a two's-complement 2-bit field:
 *     0b00 = +0, 0b01 = +1, 0b11 = -1, 0b10 = reserved (never written).
 * Every bit past element n-1, up to the end of the section, is zero: the bytes depend on the input alone.
 */
#ifndef GQ_SIGN_H
#define GQ_SIGN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GQ_SIGN_ABI_VERSION 1
#define GQ_SIGN_ITEM_BYTES 4096   /* wire bytes per item (16384 elements): every launch walks a tensor in items of this size */

/*
 * The tensors of one group, table-driven like gq_topk_batch: ONE launch serves all of them.
 *   seg_table int64[nseg][8] = { source (float *), n, first item, wire offset (bytes, a multiple of 16), -,
 *                                out offset (floats), -, error buffer (float *, 0 = none) }
 *   item_seg  int32[nitems]: the tensor of every item; the items of tensor s are first .. first + max(1, ceil(S / GQ_SIGN_ITEM_BYTES)) - 1,
 *             S = the tensor's section bytes
 *   dense_table int64[ndense][3] = { source (float *), byte offset in ONE user's wire (a multiple of 4), elements }: the
 *             uncompressed tensors the compress launch copies into the wire as they are (gq_qsgd_batch.dense_table)
 * Sources, error buffers and outputs need 4-byte alignment only (16-byte aligned runs take float4 accesses).
 */
typedef struct gq_sign_batch {
    uint32_t struct_bytes;     /* sizeof(gq_sign_batch) */
    int32_t nseg;
    int64_t nitems;
    const int64_t *seg_table;
    const int32_t *item_seg;
    const int64_t *dense_table;
    int32_t ndense;
    int32_t reserved;
} gq_sign_batch;

int gq_sign_abi_version(void);
const char *gq_sign_last_error(void);

/*
 * The 2-bit codes of every tensor into `wire` (+ the dense tensors' copy), ONE launch.
 * ef_scale not NaN: error feedback (ps_quantizer.py:35-39) -- w = v + ef_scale * err (the product rounded, then the sum), w is
 * stored back into the source and err = w - sign(w).  Otherwise w = v and the source is only read.
 * out != NULL: the dense sign(w) at out + out offset (+0.0f, +1.0f or -1.0f).
 */
int gq_sign_compress_batched(const gq_sign_batch *b, uint8_t *wire, float ef_scale, float *out, void *stream);

/*
 * Decode-mean of R payloads (payload r at gathered + r * user_stride_bytes) into out + out offset, one launch:
 *     out[i] = (float)(c_0[i] + ... + c_{R-1}[i]) / (float)R     an exact integer sum, then a true division
 * which equals gq_mean_rows' (+0 + s_0[i] + ... + s_{R-1}[i]) / R over the dense sign tensors s_r (every partial sum is a
 * small integer, exact in f32, and no -0 occurs).  plain (R == 1 only): the payload's values, no division (the same values).
 */
int gq_sign_decode_sum_batched(const gq_sign_batch *b, const uint8_t *gathered, int64_t user_stride_bytes, int R, float *out,
                               int plain, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GQ_SIGN_H */
