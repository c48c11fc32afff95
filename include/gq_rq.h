/*
 * libgq_rq.so -- the ResidualCompressor (residual_compressor.py:7-32) in multi-tensor form, gfx950.
 *
 * The compressor is two stages: NearestNeighbor on the gradient, the probabilistic vector compressor on what stage 1 leaves
 * (`residuals -= decompressed`, :22); its decode is torch.stack([d1, d2]).sum(0) = (0 + d1) + d2.  A tensor travels as TWO HSQ
 * sections back to back -- stage 1's and stage 2's, each laid out as the HSQ wire lays out codes | levels | lb, ub -- and a
 * group of tensors is described by two gq_hsq_batch descriptors over ONE tile space (the same tile_seg, nseg, ntiles, d, K and
 * widths; level_bytes 0, 1, 2 or 4: no packed levels), whose segment tables differ in their wire offsets (columns 3 .. 5).  Stage 1's encode and both level launches are
 * libgq_hsq.so's (gq_hsq_encode_batched, gq_hsq_levels_batched over either descriptor).  This library holds the two launches
 * that are the compressor's own: stage 2's encode, which reads stage 1's payload from the wire, and the decode-mean.
 */
#ifndef GQ_RQ_H
#define GQ_RQ_H

#include <stdint.h>

#include "gq_hsq.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GQ_RQ_ABI_VERSION 1
int gq_rq_abi_version(void);
const char *gq_rq_last_error(void);

/* stage1: the descriptor gq_hsq_encode_batched / gq_hsq_levels_batched take for stage 1 -- its seg_table carries the gradient
 *   pointers (column 0), the error buffers (column 7), stage 1's wire offsets and the tensors' offsets in `out`; its codebook
 *   is stage 1's (the decode codebook of the NearestNeighborCompressor).
 * stage2: the same tile space over stage 2's sections; columns 0 and 7 of its table are not read (the gradient comes from
 *   stage 1's table); codebook = the probabilistic vector compressor's codewords; u_flat and seg_minmax are stage 2's own.
 * c_dagger: pinv(codewords^T) of stage 2, [K, d] f32, 16-byte aligned; both codebooks 16-byte aligned too.
 * level2_words: two device words, or NULL.  With GQ_RANDOM_DEVICE_COUNTER the encode leaves { a seed for stage 2's level
 *   launch, 0 } there: gq_hsq_levels_batched(stage2, GQ_RANDOM_DEVICE_COUNTER, seed = that address) then draws from a stream of
 *   the step's words that neither stage 1's level launch nor this encode uses. */
typedef struct gq_rq_batch {
    uint32_t struct_bytes;     /* sizeof(gq_rq_batch) */
    int32_t reserved;
    const gq_hsq_batch *stage1;
    const gq_hsq_batch *stage2;
    const float *c_dagger;
    uint64_t *level2_words;
} gq_rq_batch;

/* 1 when the two launches serve the shape: d in {8, 16, 32}, K a multiple of 32 in [32, 256], byte codes (gq_pvq_batched_serves). */
int gq_rq_batched_serves(int d, int K, int code_bytes);

/*
 * Stage 2's encode of every tensor of the group into ONE user's `wire`, behind stage 1's encode and level launch for that
 * wire: a tile is staged as  v - codebook1[code1] * norm1  (the product rounded, then the difference: the reference's
 * `residuals -= decompressed`), code1 and the level of norm1 read from stage 1's sections of `wire`, norm1 de-quantised as
 * probabilistic_scalar_compressor.py:31-32 does it (level_bytes == 0: the f32 projection as it travels), and encoded as
 * gq_pvq_encode_batched encodes a tile: codes into stage 2's codes section, u into stage2->u_flat, (min, max) folded into
 * stage2->seg_minmax (reset by the caller to { 0xFFFFFFFF, 0 } before each encode).  Per tensor the result is
 * gq_pvq_encode's stage1 form, bit for bit, given the same draws.  v is what stage 1's encode left in the gradient buffers
 * (with error feedback: grad + ef_scale * error).
 * Draws, one uniform per subvector: GQ_RANDOM_GIVEN (r_flat, laid out like u_flat), GQ_RANDOM_DEVICE, GQ_RANDOM_DEVICE_COUNTER
 * (`seed` = the address of the { seed, step } words), GQ_RANDOM_DEVICE_KEYED (keyed by the bits of the subvector's l1).  In the
 * device modes the seed is salted: a level launch given the SAME seed argument draws from another stream.
 */
int gq_rq_encode2_batched(const gq_rq_batch *b, uint8_t *wire, int random_mode, uint64_t seed, const float *r_flat, void *stream);

/*
 * Decode-mean over R payloads (`gathered` + r * user_stride_bytes), every tensor of the group:
 *   acc = x_0;  acc = acc + x_r (r = 1 .. R-1, payloads ascending);  x_r = (0 + d1_r) + d2_r,  d_k = codebook_k[code] * norm
 * -- the inner sum is the compressor's own torch.stack([d1, d2]).sum(0), rounded before it enters the sum over the payloads
 * (ps_quantizer.py:47-48) -- then the mean as gq_hsq_decode_sum_batched takes it.  x_r is never -0 (the inner sum starts from
 * +0), so the plain decompress of ONE payload and the aggregate of one payload are the same bits.
 * mode: GQ_RQ_MEAN (the aggregate), GQ_RQ_PLAIN (R == 1: the decompress of one payload -- the ring's hop, the round trips),
 *   GQ_RQ_ERROR (R == 1, error feedback): error = v - x into the buffers of stage1->seg_table[:, 7], v read from column 0
 *   (ps_quantizer.py:37-39; rows without an error buffer are skipped); `out` is not written and may be NULL.
 * Only d, K, the widths, n_bit, nseg, ntiles, seg_table, tile_seg and codebook of the two descriptors are read.
 */
#define GQ_RQ_MEAN 0
#define GQ_RQ_PLAIN 1
#define GQ_RQ_ERROR 2
int gq_rq_decode_sum_batched(const gq_rq_batch *b, const uint8_t *gathered, int64_t user_stride_bytes, int R, float *out,
                             int mode, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GQ_RQ_H */
