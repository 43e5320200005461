/*
 * subgc_criterion_hip.h -- the label-smoothed language loss of libsubgc_hip.so (gfx950): `--label_smoothing` (opts.py:105).
 *
 * The fifth public header.  subgc_hip.h is the model's drop-in boundary (LanguageModelCriterion lives there: subgc_masked_nll_*),
 * subgc_metrics_hip.h, subgc_grounding_hip.h and subgc_controllability_hip.h hold the evaluation scores; all four stay as they are.  Same
 * library, same contract as those: every function returns 0 (SUBGC_OK) or a negative SUBGC_E* code with the text in subgc_last_error(),
 * never allocates device memory and never synchronises the device (debug bounds mode excepted, subgc_debug_bounds), enqueues on `stream`
 * (a hipStream_t passed as void*), all pointers are BORROWED device pointers, outputs are caller-allocated, everything is per call and
 * there is no global state.  subgc_version() does not change with this header.
 *
 * What is replaced:
 *   misc/utils.py:126-156   LabelSmoothing: the masked KL divergence (nn.KLDivLoss, unreduced) against the smoothed target distribution
 *                           true_dist[q, c] = (c == target_q ? 1 - smoothing : smoothing / (V - 1)), summed over c, weighted by the mask,
 *                           divided by the mask sum.
 * With V the row width (vocab_size + 1), s = smoothing, conf = 1 - s, e = s / (V - 1) and H = conf log conf + s log e (0 log 0 = 0 at both
 * ends), the row term is closed:
 *   row_q = H - conf lp[q, w_q] - e (slp_q - lp[q, w_q]),   slp_q = sum_c lp[q, c],      loss = sum_q m_q row_q / sum_q m_q
 *   d loss / d lp[q, c]     = -g_q (c == w_q ? conf : e),                                 g_q = dloss m_q / sum m
 *   d loss / d logits[q, c] =  g_q (softmax[q, c] - (c == w_q ? conf : e))               (the smoothed target sums to 1)
 * so the dense true_dist is never formed and the forward needs ONE extra scalar per row, slp, taken from the row pass that produces lse.
 * conf, e and H are formed once per call on the host in fp64 and rounded to fp32; the kernels work in fp32.
 * No float atomics: every sum is a per-lane sequence, a wave tree and a sequence over the waves, so equal inputs give equal bits with or
 * without subgc_deterministic.  `smoothing` outside [0, 1] (NaN included) is SUBGC_EINVAL with the number in the error text; at V == 1
 * only smoothing == 0 is accepted (e has no meaning).  Targets are clamped into [0, V - 1] like in subgc_masked_nll_*; debug bounds mode
 * checks them first and reports instead.
 */
#ifndef SUBGC_CRITERION_HIP_H
#define SUBGC_CRITERION_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One read of every row of x [rows, V] (ld ldx), nothing written back (misc/utils.py:126-156: the sum over the vocabulary of the KL terms).
 *   lse != NULL: x holds RAW logits; lse[r] = log sum_c exp(x[r, c]) exactly as subgc_row_lse_f32 forms it, and
 *                slp[r] = sum_c (x[r, c] - lse[r]): the subtraction is made per element while the row is in registers (sum x - V lse
 *                would lose the digits that a common offset of the logits occupies);
 *   lse == NULL: x holds log-probabilities; slp[r] = sum_c x[r, c].
 * Order of the sum: lane i adds its columns i, i + 256, ... in ascending order, then the wave tree, then the four waves in order.
 * V <= 256 * 64, like subgc_log_softmax_rows.                                                                                         */
int subgc_row_lse_sum_f32(const float* x, int64_t ldx, int rows, int V, float* lse, float* slp, void* stream);

/* LabelSmoothing.forward (misc/utils.py:126-156) in the closed form above.  logp [S, T, V] contiguous; target / mask are [S, T] views with
 * row strides t_stride / m_stride; slp [S * T] from subgc_row_lse_sum_f32; loss: one float; scratch2 = {num, den} for the backward, as for
 * subgc_masked_nll_fwd.  lse (may be NULL): logp holds raw logits and lp[q, w] = logp[q, w] - lse[q] (slp is then the lse form's).
 * den_override (device float*, may be NULL): the denominator over rows this call does not see (the packed decoder hands in the rows before
 * the reference's early break, AttModel.py:171-172, and the sum of ALL mask entries).  The rows not given are the mask-0 tail and the rows
 * the reference leaves at zero; a masked-in zero row has lp = 0 and contributes m H, so num += H (*den_override - den of the rows given).  */
int subgc_smoothed_nll_fwd(const float* logp, const int64_t* target, int64_t t_stride, const float* mask, int64_t m_stride,
                           const float* slp, double smoothing, float* loss, float* scratch2, int S, int T, int V,
                           const float* den_override, const float* lse, void* stream);

/* Backward of the criterion with respect to its input (misc/utils.py:126-156 under autograd): dlogp[q, c] = -dloss m_q / den *
 * (c == w_q ? conf : e), den = scratch2[1].  Dense [S, T, V]; EVERY element is written, the caller need not zero the buffer.          */
int subgc_smoothed_nll_bwd(const int64_t* target, int64_t t_stride, const float* mask, int64_t m_stride, const float* scratch2,
                           const float* dloss, double smoothing, float* dlogp, int S, int T, int V, void* stream);

/* The same backward fused through the log-softmax (misc/utils.py:126-156 applied to the decoder's log-probabilities, AttModel.py:336):
 * dlogits[q, c] = g_q (exp(logp[q, c] - lse[q]) - (c == w_q ? conf : e)); never materialises dlogp or true_dist.  The arguments are those of
 * subgc_nll_logsoftmax_bwd plus `smoothing`: logp [S * T, V] contiguous (raw logits when lse != NULL), dlogits [S * T, >= V] (ld ld_out) fp32
 * or bf16 (out_bf16), rows with mask 0 or active[q] == 0 (active may be NULL) are written as zeros.  Four columns per lane when V % 4 == 0,
 * ld_out % 4 == 0 and both bases are aligned (16 bytes; 8 for a bf16 output), one column per lane otherwise: same values either way.  */
int subgc_smoothed_logsoftmax_bwd(const float* logp, const int64_t* target, int64_t t_stride, const float* mask, int64_t m_stride,
                                  const float* scratch2, const float* dloss, double smoothing, void* dlogits, int64_t ld_out, int S, int T,
                                  int V, const int32_t* active, int out_bf16, const float* lse, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SUBGC_CRITERION_HIP_H */
