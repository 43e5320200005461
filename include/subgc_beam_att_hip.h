/*
 * subgc_beam_att_hip.h -- attention of the winning beams in libsubgc_hip.so (gfx950): beam search that remembers on WHICH state row
 * every word of every beam was produced, and the gather that turns that ancestry into the time-major attention buffer the grounding
 * kernels read.
 *
 * The tenth public header.  subgc_hip.h is the model's drop-in boundary; subgc_metrics_hip.h, subgc_grounding_hip.h,
 * subgc_controllability_hip.h, subgc_criterion_hip.h, subgc_selfcritical_hip.h, subgc_consensus_hip.h, subgc_forced_hip.h and
 * subgc_control_input_hip.h stay as they are, and so does subgc_beam_step (signature and bits).  Same library, same contract as those:
 * every function returns 0 (SUBGC_OK) or a negative SUBGC_E* code with the text in subgc_last_error(), never allocates device memory
 * and never synchronises the device, enqueues on `stream` (a hipStream_t passed as void*) and can be captured into a hipGraph, all
 * pointers are BORROWED device pointers, outputs are caller-allocated, everything is per call and there is no global state.
 * subgc_version() does not change with this header.
 *
 * What is replaced: nothing the reference can do.  misc/eval_utils.py:45 asserts beam_size == 1 for the grounding evaluation and
 * AttModel.py:179-234 (`_sample_sentences`) never asks get_logprobs_state (AttModel.py:328-340) for `return_att`; the result equals
 * what that function returns with return_att=True when it is driven along a winning beam's tokens.
 * No arithmetic on attention weights: rows are copied bit for bit.  No float atomics.
 * Out of scope: the attention of the beams that did not win (the ancestry of every finished beam is recorded, only one per sub-graph
 * is gathered per call), bf16.
 */
#ifndef SUBGC_BEAM_ATT_HIP_H
#define SUBGC_BEAM_ATT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SUBGC_BEAM_ATT_MAX_T 64      /* words of a beam (subgc_beam_step's limit) */
#define SUBGC_BEAM_ATT_MAX_BD 16     /* beams per group (subgc_beam_step's limit) */
#define SUBGC_BEAM_ATT_MAX_KK 18     /* leading columns per row (subgc_beam_step's limit) */
#define SUBGC_BEAM_ATT_MAX_N 4096    /* columns of an attention row */

/* CaptionModel.py:28-94,126-166 -- subgc_beam_step, every argument and every common output (seq, lps, sums, done_*, tok, src) bit for
 * bit, plus the ANCESTRY of every beam, forked exactly as `seq` is forked (CaptionModel.py:76-90):
 *   anc [n][G][T][bd] int32: after the step of loop iteration t, for a live group g (tau = t - g) and every r <= tau,
 *     anc[s][g][r][vix] = the slot (0 .. bd-1 within the group) that the beam now in slot vix held after its word r;
 *     anc[s][g][tau][vix] = vix.  The decoder step that produced the logits of word r + 1 ran on state row (s * G + g) * bd + that slot.
 *   done_anc [n][G][cap][T] int32: the column of a finished beam, filed next to done_seq in the same slot; 0 behind its length.
 * anc needs no zeroing between searches (entries are written before they are read); done_anc is read only below done_cnt.
 * Limits as subgc_beam_step: T <= 64, bd <= 16, kk <= 18.                                                                            */
int subgc_beam_step_anc(const float* tv, const int32_t* ti, int32_t* seq, float* lps, float* sums, int32_t* done_cnt, int32_t* done_seq,
                        float* done_lps, float* done_p, int32_t* done_len, int32_t* anc, int32_t* done_anc, int64_t* tok, int32_t* src,
                        int n, int t, int T, int G, int bd, int kk, int unk, int constraint, float lam, int cap, void* stream);

/* The attention rows of one finished beam per sub-graph, in the layout subgc_grounding_argmax reads (AttModel.py:321-324 keeps the same
 * rows for a greedy decode; get_logprobs_state(return_att=True), AttModel.py:328-340, computes them along the beam's tokens).
 *   al_step [steps][rows][N] fp32 (slice stride ld_step >= rows * N elements, rows = n * G * bd, row stride N): slice 0 holds the
 *     attention rows of the <bos> step, slice t + 1 those of the decoder step issued in loop iteration t; steps >= T + G - 1.
 *   pick [n][2] int32: (group g, finished-beam slot j) of the beam chosen for sub-graph s; done_len / done_anc as subgc_beam_step_anc
 *     filed them.  The caller checks 0 <= g < G and 0 <= j < done_cnt[s][g] on the host; the kernel clamps g, j, the slot and the step.
 *   out [T + 1][n][N] fp32 (strides ld_t, ld_row in elements): for word position w < len = min(done_len[s][g][j], T)
 *     out[0, s, :] = al_step[0, (s * G + g) * bd, :]                       (the rows of a sub-graph agree in the <bos> step, and
 *                                                                           groups g > 0 restart from that snapshot),
 *     out[w, s, :] = al_step[w + g, (s * G + g) * bd + done_anc[s][g][j][w - 1], :]   for w >= 1,
 *     and zero rows for len <= w <= T: beam search never feeds its last word (CaptionModel.py:170-171), so unlike a greedy decode
 *     there is no attention row behind the last word.
 * One workgroup per (sub-graph, word position), lanes over the N columns.  N <= SUBGC_BEAM_ATT_MAX_N (4096), T <= 64, bd <= 16.        */
int subgc_beam_att_gather(const float* al_step, int64_t ld_step, int steps, int rows, int N, const int32_t* done_anc,
                          const int32_t* done_len, const int32_t* pick, int n, int G, int bd, int cap, int T, float* out, int64_t ld_t,
                          int64_t ld_row, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SUBGC_BEAM_ATT_HIP_H */
