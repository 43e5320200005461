/*
 * subgc_selfcritical_hip.h -- the kernels of self-critical sequence training (SCST) in libsubgc_hip.so (gfx950): the reward-weighted
 * criterion `RewardCriterion` (misc/utils.py:89-109), the token choice of its rollout, and the reward of a rollout.
 *
 * The sixth public header.  subgc_hip.h is the model's drop-in boundary, subgc_metrics_hip.h, subgc_grounding_hip.h and
 * subgc_controllability_hip.h hold the evaluation scores, subgc_criterion_hip.h the label-smoothed loss; all five stay as they are.  Same
 * library, same contract as those: every function returns 0 (SUBGC_OK) or a negative SUBGC_E* code with the text in subgc_last_error(),
 * never allocates device memory and never synchronises the device (debug bounds mode excepted, subgc_debug_bounds), enqueues on `stream`
 * (a hipStream_t passed as void*), all pointers are BORROWED device pointers, outputs are caller-allocated, everything is per call and
 * there is no global state.  subgc_version() does not change with this header.
 *
 * What is replaced:
 *   misc/utils.py:89-109    RewardCriterion: loss = sum((-input * reward + gpn_loss * exp(reward)) * m) / sum(m) with the mask of :98-99,
 *                           m[s, 0] = 1, m[s, t] = seq[s, t - 1] > 0; the reference defines the class and the options around it
 *                           (opts.py:24, :66, :149-152; train.py:151 hands gts / gt_indices to LossWrapper.forward) and never runs it.
 *   AttModel.py:295-316     the token choice of `_sample`; the reference has the greedy and the top-k branch, SCST needs the branch of the
 *                           upstream project it descends from, sample_max = 0: a draw from the whole tempered distribution.
 *   misc/utils.py:59-81     decode_sequence, whose upstream twin for the reward (array_to_str) keeps the end token as a word.
 * SCST is REINFORCE on the decoder with the greedy caption's score as the baseline: reward = score(sampled) - score(greedy).  The
 * decoder's state depends on the sampled tokens only as inputs, so the gradient of a sampled forward is the gradient of a teacher-forced
 * forward on the sampled tokens with the loss below: the fused forms take the arguments of subgc_masked_nll_fwd / subgc_nll_logsoftmax_bwd
 * plus `reward`.
 * No float atomics: every sum is a per-lane sequence, a wave tree and a sequence over the four waves, so equal inputs give equal bits with
 * or without subgc_deterministic.  Token ids are clamped into [0, V - 1] like in subgc_masked_nll_*; debug bounds mode checks them first
 * and reports instead.
 */
#ifndef SUBGC_SELFCRITICAL_HIP_H
#define SUBGC_SELFCRITICAL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The token choice of one rollout step for n rows of which the first n_sample SAMPLE and the others are GREEDY (AttModel.py:295-316 with
 * the sample_max = 0 branch the reference lacks; one launch serves the sampled caption and its greedy baseline).
 *   rows [0, n_sample):  a draw from softmax(logits / temp) by inverse CDF in COLUMN order with u[r] in [0, 1):
 *       pick = #{c : u >= cdf_c}, clamped to V - 1, cdf_c = (sum of e_0 .. e_c) / (sum of all e), e_c = exp(logits[c] / temp - max).
 *       The sums are fp32 in a fixed order: lane i adds its chunk of ceil(V / 256) consecutive columns in ascending order, the 256 chunk
 *       sums pass a scan (a fixed tree per wave, the four wave totals in order), and every lane walks its own chunk on top of its base.
 *       A column of mass 0 in front of the first or behind the last positive one is never picked (u < 1 = cdf there).
 *       lp = logits[pick] / temp - log sum_c exp(logits[c] / temp): shift-invariant, so raw logits and log-probabilities give the same.
 *   rows [n_sample, n):  the first arg-max, exactly subgc_decode_pick with k = 0 on the same row: lp is the value itself, or with
 *       raw_logits != 0 the log-softmax at the arg-max, -log sum_c exp(x[c] - max).  Bit for bit the same tokens and lp.
 * Everything else is subgc_decode_pick's contract: unfinished &= it > 0 (t == 0: unfinished = it > 0); it *= unfinished;
 * seq[r, t] = it; seqlp[r, t] = lp; next_tok[r] = it; *n_unfinished = 1 by a plain store when a row is unfinished (a flag; may be NULL);
 * prev_count != NULL and *prev_count == 0: nothing is written (the reference has left its loop, AttModel.py:318-319).  Capturable.
 * One workgroup of 256 per row, one read of the row; V <= 16384, ld >= V, temp > 0, 0 <= n_sample <= n, 0 <= t < T.                  */
int subgc_sc_pick(const float* logits, int64_t ld, int n, int n_sample, int V, float temp, const float* u, int t, int64_t* seq,
                  float* seqlp, int T, int64_t* next_tok, int32_t* unfinished, int32_t* n_unfinished, const int32_t* prev_count,
                  int raw_logits, void* stream);

/* From the rollout's tokens seq2 [2 S, T] (sampled half first, greedy half second) in one launch:
 *   labels [S, T + 2] = [0, sampled row, 0]: the teacher-forced replay's input (AttModel.py:151-177 reads labels[:, :-1]);
 *   mask [S, T + 1]: m[s, 0] = 1, m[s, t] = sampled[s, t - 1] > 0 for 1 <= t < T, m[s, T] = 0 -- RewardCriterion's own mask
 *     (misc/utils.py:98-99) padded by the one step the replay computes beyond it;
 *   score_rows [2 S, T + 1]: the rows as the reward scores them.  eos_id > 0: a row's first 0 within its T columns becomes eos_id and
 *     everything behind it 0; a row without a 0 is copied and followed by 0 (the upstream array_to_str of misc/utils.py:59-81: the end
 *     token is scored as a word).  eos_id == 0: the T columns are copied unchanged, followed by 0.
 * Debug bounds mode checks seq2 against [0, V - 1].  labels, mask or score_rows may be NULL (that output is not wanted).            */
int subgc_sc_prepare(const int64_t* seq2, int S, int T, int V, int64_t eos_id, int64_t* labels, float* mask, int64_t* score_rows,
                     void* stream);

/* The self-critical reward (opts.py:149-152: --cider_reward_weight, --bleu_reward_weight) from the fp64 row records subgc_accuracy_rows
 * wrote for the 2 S scored rows (row_d [2 S, ld_d >= SUBGC_ACC_ROW_F64]; columns SUBGC_ACC_BLEU + 3 and SUBGC_ACC_CIDER):
 *   scores[r] = w_cider * CIDEr_r + w_bleu * BLEU4_r (fp64, [2 S]); reward[s, t] = (float)(scores[s] - scores[S + s]) for every t < T1
 *   ([S, T1] contiguous); mean_reward[0] = the mean of reward[:, 0], summed in fp64 in a fixed order.
 * Weights that are not finite are SUBGC_EINVAL with the numbers in the text.                                                          */
int subgc_sc_reward(const double* row_d, int ld_d, int S, int T1, double w_cider, double w_bleu, float* reward, float* mean_reward,
                    double* scores, void* stream);

/* RewardCriterion.forward (misc/utils.py:89-109) on gathered log-probabilities: input, reward [S, T] fp32 and seq [S, T] int64, all
 * contiguous; gpn_loss [S] or NULL.  Any per-token reward is accepted.  The mask is formed from seq inside the kernel (:98-99).
 *   loss = sum((-input * reward + gpn_loss[s] * exp(reward)) * m) / sum(m);   scratch2 = {num, den} for the backward.                 */
int subgc_reward_nll_fwd(const float* input, const int64_t* seq, const float* reward, const float* gpn_loss, float* loss,
                         float* scratch2, int S, int T, void* stream);

/* Its backward (misc/utils.py:89-109 under autograd): dinput[s, t] = -dloss reward m / den, every element written; with gpn_loss given,
 * dgpn[s] = dloss sum_t exp(reward[s, t]) m[s, t] / den (the row sum in fp64).  `reward` gets no gradient: it is data, as in the reference. */
int subgc_reward_nll_bwd(const int64_t* seq, const float* reward, const float* gpn_loss, const float* scratch2, const float* dloss,
                         float* dinput, float* dgpn, int S, int T, void* stream);

/* RewardCriterion (misc/utils.py:89-109, gpn_loss = None) fused on the decoder's rows: the arguments of subgc_masked_nll_fwd plus
 * `reward` ([S, T] view, row stride r_stride).  logp [S, T, V] contiguous, raw logits when lse != NULL (lp[q, w] = logp[q, w] - lse[q]);
 * target / mask [S, T] views with row strides; den_override (may be NULL) as in subgc_masked_nll_fwd.
 *   num = -sum_q r_q m_q lp[q, w_q];  den = sum_q m_q or *den_override;  loss = num / den;  scratch2 = {num, den}.
 * Order of the sums: lane i of 256 adds its rows i, i + 256, ... in ascending order, then the wave tree, then the four waves in order.  */
int subgc_reward_logits_fwd(const float* logp, const int64_t* target, int64_t t_stride, const float* mask, int64_t m_stride,
                            const float* reward, int64_t r_stride, float* loss, float* scratch2, int S, int T, int V,
                            const float* den_override, const float* lse, void* stream);

/* The backward of that loss through the log-softmax (misc/utils.py:89-109 applied to the decoder's log-probabilities, AttModel.py:336):
 * dlogits[q, c] = g_q (exp(logp[q, c] - lse[q]) - [c == w_q]), g_q = dloss (r_q m_q) / den, den = scratch2[1]; g_q may be negative or
 * zero.  The arguments are those of subgc_nll_logsoftmax_bwd plus `reward`: dlogits [S * T, >= V] (ld ld_out) fp32 or bf16 (out_bf16),
 * rows with mask 0 or active[q] == 0 (active may be NULL) are written as zeros.  Four columns per lane when V % 4 == 0, ld_out % 4 == 0
 * and both bases are aligned (16 bytes; 8 for a bf16 output), one column per lane otherwise: same values either way.  With reward == 1
 * every value is the one subgc_nll_logsoftmax_bwd writes.                                                                             */
int subgc_reward_logsoftmax_bwd(const float* logp, const int64_t* target, int64_t t_stride, const float* mask, int64_t m_stride,
                                const float* reward, int64_t r_stride, const float* scratch2, const float* dloss, void* dlogits,
                                int64_t ld_out, int S, int T, int V, const int32_t* active, int out_bf16, const float* lse, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SUBGC_SELFCRITICAL_HIP_H */
