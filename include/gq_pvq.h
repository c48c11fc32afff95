/*
 * libgq_pvq.so -- the ProbabilisticVectorCompressor (probabilistic_vector_compressor.py:8-77) in multi-tensor form, gfx950.
 *
 * The compressor's signature is HSQ's -- (codes, levels, lb, ub) -- and so are its level quantiser and its decode
 * (codewords[codes] * norms, :67-77 against nearest_neighbor_compressor.py:80-90).  What differs is the encode: the
 * codeword of a subvector is SAMPLED with probability |p_k| / ||p||_1, p = c_dagger . v (see gq_pvq_encode in gq_hsq.h).
 * This library holds that one launch for every tensor of a model at once; levels, decode-mean and the fused forms are the
 * calls of libgq_hsq.so over the same descriptor (gq_hsq_levels_batched, gq_hsq_decode_sum_batched[_tail],
 * gq_hsq_levels_decode_batched).
 */
#ifndef GQ_PVQ_H
#define GQ_PVQ_H

#include <stdint.h>

#include "gq_hsq.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GQ_PVQ_ABI_VERSION 1
int gq_pvq_abi_version(void);
const char *gq_pvq_last_error(void);

/* hsq: the group's gq_hsq_batch as the level / decode calls take it -- d, K, code_bytes, nseg, ntiles, seg_table, tile_seg,
 * u_flat and seg_minmax are read here; hsq->codebook is the DECODE codebook (the compressor's codewords) and is not read by
 * the encode.  c_dagger: pinv(codewords^T), [K, d] f32, 16-byte aligned. */
typedef struct gq_pvq_batch {
    uint32_t struct_bytes;     /* sizeof(gq_pvq_batch) */
    int32_t reserved;
    const gq_hsq_batch *hsq;
    const float *c_dagger;
} gq_pvq_batch;

/* 1 when the multi-tensor encode serves the shape: d in {8, 16, 32}, K a multiple of 32 in [32, 256], byte codes. */
int gq_pvq_batched_serves(int d, int K, int code_bytes);

/*
 * Encode of every tensor of the group into ONE user's `wire`: codes into each segment's codes section, u = sign(p_code) * l1
 * into u_flat[tile * 64 + i], (min, max) of u folded into seg_minmax in the order-mapped form gq_hsq_levels_batched reads
 * (the caller resets the words to { 0xFFFFFFFF, 0 } before each encode).  Per tensor the result is gq_pvq_encode's, bit for
 * bit, given the same draws.
 * Draws, one uniform per subvector:
 *   GQ_RANDOM_GIVEN           r_flat, laid out like u_flat (padding slots are not read)
 *   GQ_RANDOM_DEVICE          in-kernel, from `seed` and the subvector's index in the padded space
 *   GQ_RANDOM_DEVICE_COUNTER  `seed` is the address of device words { seed, step }: what gq_hsq_levels_batched takes
 *   GQ_RANDOM_DEVICE_KEYED    as DEVICE, the stream of a subvector keyed by the bits of its l1 as well
 * In the device modes the seed is salted, so that the level launch, given the SAME seed argument, draws from another stream.
 * A GQ_RANDOM_DEVICE_COUNTER address that is null or not 8-byte aligned is refused: GQ_ERR_INVALID_ARG, nothing is launched
 * (as gq_rq_encode2_batched does; the words are read with 64-bit loads).
 * ef_scale: NaN = no error feedback; otherwise every tile of a row with an error buffer (seg_table[seg][7] != 0) is read as
 * v = grad + ef_scale * error (product rounded, then the sum: ps_quantizer.py:35), v is stored back over grad and v is
 * encoded; gq_hsq_levels_batched(write_error = 1) then leaves error = v - decoded.
 */
int gq_pvq_encode_batched(const gq_pvq_batch *b, uint8_t *wire, int random_mode, uint64_t seed, const float *r_flat,
                          float ef_scale, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GQ_PVQ_H */
