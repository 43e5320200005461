/*
 * subgc_gcn_agg_hip.h -- "aggregate first" for the collection units WITHOUT BatchNorm in libsubgc_hip.so (gfx950).
 *
 * A collection unit (graph_conv_unit.py:28-36) is relu( A fc_rgt(fc_lft(source)) / (rowsum(A) + 1e-7) ).  With gcn_bn = 0 everything in
 * front of the ReLU is linear, so where the targets are fewer than the sources (nodes <- relations: 37 against 65 rows per image) the 0/1
 * map A is applied to the 1024-wide SOURCE rows and the two Linear layers run on the target rows:
 *     relu( (S A X) Wl^T Wr^T + s (bl Wr^T + br) ),   S = diag(0.5 / (cnt + 1e-7)),  s = S cnt.
 * The pieces: the aggregation and its backward gather (csrc/graph.hip), a per-row scale on the fp32 GEMM's bias (csrc/gemm_f32.hip:
 * A (X W^T + 1 b^T) = (A X) W^T + rowsum(A) b^T) and the row-weighted column sums that are the bias gradients.
 *
 * A header of its own, registered in `_lib.HEADERS` (subgc_hip.h and the earlier headers keep their entry points and counts).
 * Same library, same contract: every function returns 0 (SUBGC_OK) or a negative SUBGC_E* code with the text in
 * subgc_last_error(), never allocates device memory, never synchronises the device, enqueues on `stream` (a hipStream_t passed as void*),
 * all pointers are BORROWED device pointers, outputs are caller-allocated.  No float atomics: every sum runs in a fixed order.
 */
#ifndef SUBGC_GCN_AGG_HIP_H
#define SUBGC_GCN_AGG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* For every target row i of image b and both roles r (0: the node is the relation's subject, 1: its object), over the CSR lists of
 * subgc_csr_build (ptr int32 [2, B, N + 1], edges int32 [2, B, K], ascending k):
 *     Xagg_r[b, i, :] = (sum_j X[b, j, :]) * 0.5 / (cnt_r + 1e-7)        rows added in list order, then ONE division and ONE halving
 *     s_r[b, i]       = 0.5 * cnt_r / (cnt_r + 1e-7)                     0 for a row without neighbours (its Xagg row is 0 too)
 * X [B, K, L], Xagg_r [B, N, L], s_r [B * N], all fp32, contiguous, 16-byte aligned; L % 4 == 0 (anything else is SUBGC_EINVAL).
 * The 0.5 is the role average of graph_conv.py:26: a power of two, it commutes exactly with the ReLU and with every rounding.        */
int subgc_gcn_agg_fwd(const float* X, const int32_t* ptr, const int32_t* edges, float* Xagg0, float* Xagg1, float* s0, float* s1,
                      int B, int N, int K, int L, void* stream);

/* Its backward: every relation k has ONE subject and ONE object (rel_ind int64 [B, K, 2], clamped to [0, N) as subgc_csr_build clamps),
 * so d(source) is a gather of two target rows:
 *     dX[b, k, :] (+)= w_0[subj] dXagg0[b, subj, :] + w_1[obj] dXagg1[b, obj, :],    w_r[i] = 0.5 / (cnt_r[i] + 1e-7)
 * `accumulate` != 0 adds to what dX holds.  Same layout and alignment rules as the forward.                                            */
int subgc_gcn_agg_bwd(const float* dXagg0, const float* dXagg1, const int64_t* rel_ind, const int32_t* ptr, float* dX, int accumulate,
                      int B, int N, int K, int L, void* stream);

/* ReLU masks of the two roles from the stored outputs, one launch: dz_r[i] = y_r[i] > 0 ? dy[i] : 0 for i < n (fp32, contiguous).       */
int subgc_gcn_agg_relu_bwd(const float* dy, const float* y0, const float* y1, float* dz0, float* dz1, int64_t n, void* stream);

/* subgc_gemm_f32 with a per-row scale on the bias: C = epilogue(op(A) op(B) + bias_scale[row] * bias).  bias_scale fp32 [M]; NULL means
 * subgc_gemm_f32's own epilogue, bit for bit (the call is then subgc_gemm_f32 without its weight-streaming form for M <= 80).
 * Arguments, flags (SUBGC_GEMM_RELU, SUBGC_GEMM_ACCUM, mode and tuning bits), workspace and dispatch are subgc_gemm_f32's; the scale
 * reaches the tile epilogue and the split-K reduce pass.                                                                                */
int subgc_gemm_f32_rowbias(int transA, int transB, int M, int N, int K, const float* A, int64_t lda, const float* B, int64_t ldb, float* C,
                           int64_t ldc, const float* bias, const float* bias_scale, int flags, void* workspace, size_t ws_bytes,
                           void* stream);

/* subgc_gemm_f32_pair with the per-row bias scales of its two problems (both or none).  SUBGC_GEMM_RELU is honoured here: a product with
 * a ReLU never takes a split-K form, so the ReLU is applied by the tile epilogue after bias_scale[row] * bias.                         */
int subgc_gemm_f32_pair_rowbias(int transA, int transB, int M, int N, int K, const float* A1, const float* A2, int64_t lda, const float* B1,
                                const float* B2, int64_t ldb, float* C1, float* C2, int64_t ldc, const float* bias1, const float* bias2,
                                const float* bias_scale1, const float* bias_scale2, int flags, void* workspace, size_t ws_bytes,
                                void* stream);

/* Row-weighted column sums of one or two fp32 matrices of one shape (the bias gradients under aggregation, db = sum_i s[i] dY[i, :]):
 *     out_q[c] (+)= sum_i w_q[i] X_q[i, c]      q < n_mat (1 or 2), X_q [M, N] with leading dimension ldx, w_q [M] (NULL = all ones)
 * Slabs of rows are summed by one workgroup each into workspace[q][slab][N] and added in slab order by a second launch; the slab
 * size depends on (M, N) alone, so the result is a function of the inputs and the shape.  The workspace must hold
 * subgc_colsum_rows_workspace_bytes(M, N, n_mat) bytes and be 4-byte aligned.                                                          */
int subgc_colsum_rows_f32(int n_mat, const float* X0, const float* X1, int64_t ldx, int M, int N, const float* w0, const float* w1,
                          float* out0, float* out1, int accumulate, void* workspace, size_t ws_bytes, void* stream);
int subgc_colsum_rows_workspace_bytes(int M, int N, int n_mat, size_t* bytes);

#ifdef __cplusplus
}
#endif
#endif /* SUBGC_GCN_AGG_HIP_H */
