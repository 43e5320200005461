/*
 * subgc_neighbours_hip.h -- the nearest-image search of consensus re-ranking in libsubgc_hip.so (gfx950): `find_NNimg`
 * (misc/consensus_reranking/concensus_reranking_utils/consensus_reranking.py:59-119), the stage in front of `consensus_rerank`
 * (subgc_consensus_cook / _score / _rank of subgc_hip.h, subgc_consensus_bleu_* of subgc_consensus_hip.h).
 *
 * Same library, same contract as the other public headers, which all stay as they are: every function returns 0 (SUBGC_OK) or a
 * negative SUBGC_E* code with the text in subgc_last_error(), never allocates device memory and never synchronises the device,
 * enqueues on `stream` (a hipStream_t passed as void*), all pointers are BORROWED device pointers, outputs are caller-allocated,
 * everything is per call and there is no global state.  subgc_version() does not change with this header.
 *
 * What is replaced:
 *   consensus_reranking.py:105, :113    scipy.spatial.distance.cdist(feat_arr_te, feat_arr_tr, 'euclidean') in float64
 *                                       (conf_cr.py:14,42: 2048-dimensional features, distance_metric = 'euclidean');
 *   consensus_reranking.py:108, :114    np.argsort(dis_trte, axis=1)[:, :num_NNimg] (conf_cr.py:51: num_NNimg = 1000).
 *
 * The distance contract.  scipy's euclidean cdist is, bit for bit, the sequential sum
 *       s = 0;  for d = 0 .. D-1 ascending:  t = a[d] - b[d];  s = s + t * t;      dist = sqrt(s)
 * in fp64 with every operation rounded on its own (no fused multiply-add) and a correctly rounded square root.  The device follows
 * that loop: the order of d and the zero start are part of the contract, so equal inputs give the reference's bits.  Non-finite
 * inputs are data: inf - inf is NaN, as in scipy.
 *
 * The order contract.  The list of a row is its k smallest distances in ascending (distance, index) order: where np.argsort's
 * quicksort leaves the order of exactly equal distances unspecified, the lower index comes first.  NaN sorts after +inf, as
 * np.argsort puts it last.  No float arithmetic and no float atomics take part in the selection: equal inputs give equal bits.
 */
#ifndef SUBGC_NEIGHBOURS_HIP_H
#define SUBGC_NEIGHBOURS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* dist[i * ldd + j] = the euclidean distance of query row i (q + i * ldq, D values) and train row j (x + j * ldx, D values), fp64, by
 * the loop in the head of this file: cdist(feat_arr_te, feat_arr_tr, 'euclidean') of consensus_reranking.py:105 (all rows) and :113
 * (one row at a time; the same bits).  i < Q, j < N; ld* are in elements.  Elements of q / x beyond column D of a row, rows beyond Q / N
 * and the columns of dist beyond N are neither read nor written.  Refused (SUBGC_EINVAL, the numbers in the text): a null pointer,
 * Q / N / D < 1, ldq < D, ldx < D, ldd < N, N >= 2^31.
 * One workgroup of 256 lanes per 64 x 64 tile of pairs, a 4 x 4 micro-tile per lane on the fp64 vector ALU, both operands staged
 * through LDS in chunks of 32 columns; 16-byte global reads where the base and the row pitch allow them. */
int subgc_nn_dist_f64(const double* q, int64_t ldq, int Q, const double* x, int64_t ldx, int64_t N, int D, double* dist, int64_t ldd,
                      void* stream);

/* idx[i * k + c], val[i * k + c], c < k: the index and the value of the c-th smallest entry of row i (dist + i * ldd, N entries) in
 * ascending (distance, index) order: np.argsort(dis_trte, axis=1)[:, :num_NNimg] of consensus_reranking.py:108 / :114 with the tie
 * rule in the head of this file.  The key of an entry is its bit pattern with the sign bit cleared, read as an unsigned integer.
 * val may be NULL.  Refused (SUBGC_EINVAL, the numbers in the text): a null dist / idx, Q / N < 1, ldd < N, N >= 2^31, k outside
 * 1 .. min(N, 1024).
 * One workgroup per row: an MSB-first radix select over eight 8-bit digits (256-bin integer LDS histograms) finds the k-th key;
 * smaller keys are kept, and of the keys equal to it those at the lowest indices, found by a scan in ascending index order; the kept
 * (key, index) pairs are sorted by a bitonic network in LDS. */
int subgc_nn_select_f64(const double* dist, int64_t ldd, int Q, int64_t N, int k, int32_t* idx, double* val, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SUBGC_NEIGHBOURS_HIP_H */
