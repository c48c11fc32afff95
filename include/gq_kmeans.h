/*
 * libgq_kmeans.so -- Lloyd k-means on gfx950 for training HSQ codebooks (the reference's codebook_generator.py runs scipy's
 * kmeans2 on row-normalised Gaussians on the host), with two objectives and a result that is defined bit for bit.
 *
 * A library of its own next to libgq_hsq.so, with the conventions of the other small libraries:
 *   - return value: GQ_OK (0) or a negative GQ_ERR_* code (values of include/gq_hsq.h); gq_kmeans_last_error() gives text;
 *   - every pointer is device memory; work goes to `stream` (a hipStream_t, NULL = default), with no host synchronisation
 *     anywhere, also not between iterations;
 *   - nothing is allocated inside; every launch argument depends on the layout (N, d, K, metric, iters, the device's CU count)
 *     alone, so the launches replay from a graph.
 *
 * X is float32 [N, d] (the points, row-major), C is float32 [K, d] (the centroids, row-major).  Both need 4-byte alignment
 * only (16-byte aligned X with d % 4 == 0 takes float4 loads; the values are the same).  Supported: 1 <= d <= GQ_KMEANS_MAX_D,
 * 1 <= K <= GQ_KMEANS_MAX_K, 1 <= N <= GQ_KMEANS_MAX_N; anything else returns GQ_ERR_INVALID_ARG (a null or misaligned
 * pointer, a size below 1, iters < 1, an unknown metric) or GQ_ERR_UNSUPPORTED (a size above the range) before any launch.
 *
 * ONE ITERATION.  All f32 operations are single, separately rounded operations (-ffp-contract=off); fmaf is the fused one.
 *
 *   1. Half norm (GQ_KMEANS_EUCLID only).  hn_k = the chain acc = fmaf(c_kj, c_kj, acc) over j = 0 .. d-1 ascending, from
 *      acc = +0.0f.  h_k = 0.5f * hn_k.
 *   2. Score.  dot_ik = the chain acc = fmaf(x_ij, c_kj, acc) over j = 0 .. d-1 ascending, from acc = +0.0f (the chain of the
 *      HSQ encode's exact score).   euclid: t_ik = dot_ik - h_k (one f32 subtraction).   absdot: t_ik = fabsf(dot_ik).
 *   3. Label.  label_i = 0, best = t_i0; then for k = 1 .. K-1 ascending: if (t_ik > best) { best = t_ik; label_i = k; }.
 *      The comparison is strict, so the lowest index wins a tie, and label_i is in [0, K) for every input, NaN and
 *      infinities included (the labels of such rows are unspecified beyond that; nothing is read or written out of range).
 *      sign_i = -1 if the metric is absdot and dot_{i,label_i} < 0, else +1 (dot = -0.0f, +0.0f or NaN: +1).
 *   4. Accumulate, in integers, so that the order of the additions cannot matter:
 *          q_ij = __double2ll_rn((double)x_ij * 0x1p40)       (round to nearest even of the exact product)
 *          S_kj += sign_i * q_ij,   n_k += 1                  for k = label_i, in int64 (wrapping two's complement)
 *      Precondition: N * max|x_ij| <= 2^22, so that no |S_kj| exceeds 2^62 (unit rows at any supported N satisfy it).
 *   5. Update, row by row.  n_k == 0: row k is unchanged bit for bit.  Otherwise
 *          euclid:  c_kj = (float)((double)S_kj / ((double)n_k * 0x1p40))
 *          absdot:  f_j = (double)S_kj;  r = sqrt(sum_j f_j * f_j), the sum in f64 over j ascending from +0.0, the multiply
 *                   and the add rounded separately, sqrt correctly rounded;  r == 0: the row is unchanged;  otherwise
 *                   c_kj = (float)(f_j / r).
 *      Every f64 operation is IEEE round-to-nearest-even; (float) rounds to nearest even.
 *
 * The k-means objective of `euclid` is the usual one: argmax_k (<x, c_k> - |c_k|^2 / 2) = argmin_k |x - c_k|^2, and the update
 * is the cluster's mean (scipy.cluster.vq.kmeans2's iteration).  `absdot` is the objective HSQ encodes with: a point goes to
 * the centroid with the largest |<x, c_k>|, points with a negative projection enter the sum mirrored, and the centroid is the
 * sum normalised to unit length (a sign-invariant spherical k-means), so no two centroids settle as an antipodal pair.
 *
 * tests/kmeans_contract.py restates all of this in numpy; the library equals it bit for bit.
 */
#ifndef GQ_KMEANS_H
#define GQ_KMEANS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GQ_KMEANS_ABI_VERSION 1
#define GQ_KMEANS_MAX_D 64
#define GQ_KMEANS_MAX_K 4096
#define GQ_KMEANS_MAX_N 4194304      /* 2^22 */

#define GQ_KMEANS_EUCLID 0
#define GQ_KMEANS_ABSDOT 1
/*
 * OR-ed into `metric` (gq_kmeans_run): every point adds into the workspace with global atomics, also where the per-workgroup
 * partial sums would fit in LDS (8 * K * (d + 1) <= GQ_KMEANS_LDS_PARTIAL_BYTES; above that size this is what runs anyway).
 * The results are the same bits; the flag exists so that the two forms can be timed against each other (tools/kmeans_time.py).
 */
#define GQ_KMEANS_GLOBAL_ATOMICS 0x100
#define GQ_KMEANS_LDS_PARTIAL_BYTES 40960

/*
 * The assignment launch walks the points in passes of GQ_KMEANS_THREADS * P points per workgroup, P = 4 (d <= 16), 2 (d <= 32)
 * or 1 points per lane, on min(ceil(N / (GQ_KMEANS_THREADS * P)), GQ_KMEANS_BLOCKS_PER_CU * CUs) workgroups, each striding over
 * the passes (tests size an N from this so that every workgroup strides).
 */
#define GQ_KMEANS_THREADS 256
#define GQ_KMEANS_BLOCKS_PER_CU 2

int gq_kmeans_abi_version(void);
const char *gq_kmeans_last_error(void);

/* Bytes of gq_kmeans_run's workspace: S int64[K * d], then n int64[K].  0 for K or d outside the supported range. */
size_t gq_kmeans_workspace_bytes(int K, int d);

/*
 * One assignment (steps 1 to 3) of X to the centroids C: labels int32[N], signs int8[N] (may be NULL).  One launch.
 */
int gq_kmeans_assign(const float *X, int64_t N, int d, const float *C, int K, int metric, int32_t *labels, int8_t *signs,
                     void *stream);

/*
 * `iters` >= 1 iterations on C in place: 1 + 2 * iters launches.  labels (int32[N]), signs (int8[N], may be NULL) and counts
 * (int64[K], the n_k) are those of the LAST assignment, the one made with the centroids as they were before the last update
 * (what scipy's kmeans2 returns).  workspace: gq_kmeans_workspace_bytes(K, d) bytes, 8-byte aligned; the library zeroes it in
 * its own launches, so nothing in it has to be zero before the call, and it is zero again afterwards.
 * X must not overlap C or the outputs.
 */
int gq_kmeans_run(const float *X, int64_t N, int d, float *C, int K, int metric, int iters, int32_t *labels, int8_t *signs,
                  int64_t *counts, void *workspace, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GQ_KMEANS_H */
