/*
 * subgc_decode_rules_hip.h -- decode rules in libsubgc_hip.so (gfx950): block_trigrams, the repeat ban (decoding_constraint), the
 * bad-ending ban and the UNK penalty for the non-beam token loop, as ONE row pass in front of the unchanged pick kernels.
 *
 * The fourteenth public header.  subgc_hip.h is the model's drop-in boundary and keeps its entry points; the other twelve stay as they
 * are.  Same library, same contract as those: every function returns 0 (SUBGC_OK) or a negative SUBGC_E* code with the text in
 * subgc_last_error(), never allocates device memory and never synchronises the device (debug bounds mode excepted,
 * subgc_debug_bounds), enqueues on `stream` (a hipStream_t passed as void*) and can be captured into a hipGraph, all pointers are
 * BORROWED device pointers, everything is per call and there is no global state.  subgc_version() does not change with this header.
 *
 * What is replaced: nothing of the reference's -- its `_sample` loop (AttModel.py:282-319) applies none of these rules; its beam
 * search applies the repeat ban and the UNK penalty (CaptionModel.py:128-131).  The rules sit where the upstream project this model
 * descends from applies them: on the log-probabilities of a step, between AttModel.py:289 (get_logprobs_state) and :295 (the choice).
 * No atomics of any kind; every sum and every count has a fixed order, so equal inputs give equal bits.
 * Beam search calls the same entry point with rules 1 and 4 alone (eval_kwargs["beam_rules"]): every state row's history is the words of
 * the beam that occupies it, word w of beam group g in column g + w behind g columns of -1, and the top-k reads the ruled row.
 * Out of scope: the self-critical rollout, forced decode.
 */
#ifndef SUBGC_DECODE_RULES_HIP_H
#define SUBGC_DECODE_RULES_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SUBGC_RULES_MAX_V 16384   /* columns of a logits row */
#define SUBGC_RULES_MIN_V 8
#define SUBGC_RULES_MAX_T 64      /* steps of a row: the history is staged in LDS */
#define SUBGC_RULES_MAX_BAD 64    /* ids of the bad-ending list */

/* flag bits */
#define SUBGC_RULE_TRIGRAMS 1     /* block_trigrams */
#define SUBGC_RULE_UNK 2          /* suppress_unk */
#define SUBGC_RULE_REPEAT 4       /* decoding_constraint */
#define SUBGC_RULE_BAD_END 8      /* block_bad_endings */
#define SUBGC_RULE_ALL 15

/* columns of `stats` */
#define SUBGC_RULE_STAT_TRIGRAM 0 /* steps on which a trigram penalty was applied */
#define SUBGC_RULE_STAT_REPEAT 1  /* ... the repeat ban */
#define SUBGC_RULE_STAT_BAD_END 2 /* ... the bad-ending ban */
#define SUBGC_RULE_STAT_CHANGED 3 /* ... the first arg-max before the rules != the first arg-max after them */

/* The rules of decode step t, in place on row r of `logits` [n, V] (row stride ld floats), for every row.  The row first becomes its
 * log-softmax, lp_c = (x_c - max) - log(sum_c exp(x_c - max)), fp32, in subgc_forced_pick's chunk-then-scan order: max = the maximum
 * of the row; e_c = expf(x_c - max); lane i of the 256 adds its chunk of CH = ceil(V / 256) consecutive columns
 * [i * CH, min(V, (i + 1) * CH)) in ascending order; the 256 chunk sums pass an inclusive scan (the fixed shift-by-1, 2, 4 .. 32 tree
 * inside each wave of 64, then the totals of the waves in front added in wave order) and the sum is the scan's last element; logf of
 * it; two subtractions.  max and the logarithm are one number per row, so equal logits give equal lp bits.
 * Then the rules act, reading only the row's own history h = seq[r * T + 0 .. t - 1] (finished rows are rows like any other), in this
 * order:
 *   1. SUBGC_RULE_TRIGRAMS, t >= 3: for every j in 0 .. t - 3 with h[j] == h[t-2] and h[j+1] == h[t-1], column h[j+2] collects one
 *      count (an integer; ascending j).  A column with count c > 0 becomes lp + (float) c * trigram_pen: one product, one sum, each
 *      rounded on its own (no FMA contraction).  trigram_pen is what the caller formed, float32(float32(-0.693) * float32(alpha));
 *      -inf is a hard block.  Columns with count 0 are not touched, so 0 * inf never appears.
 *   2. SUBGC_RULE_UNK: column V - 1 becomes lp - 1000.0f (CaptionModel.py:131).
 *   3. SUBGC_RULE_REPEAT, t >= 1: column h[t-1] becomes -inf (CaptionModel.py:128-129).
 *   4. SUBGC_RULE_BAD_END, t >= 1: when h[t-1] is one of bad_ids[0 .. n_bad - 1] (device int32), column 0 (the end token) becomes -inf.
 * A history token outside [0, V) compares like any other value and touches no column; debug bounds mode checks the history first and
 * reports instead.
 *   stats (int32 [n, 4], may be NULL): row-owned counters, incremented by plain stores of one lane (columns SUBGC_RULE_STAT_*); the
 *     caller zeroes them before step 0.  The arg-max comparison is made on the fp32 log-softmax row and the ruled row.
 *   prev_count != NULL and *prev_count == 0: nothing is written, as the pick kernels do.
 * One workgroup of 256 per row, one read and one write of the row (staged in LDS), the trigram matches found by one wave.
 * SUBGC_RULES_MIN_V <= V <= SUBGC_RULES_MAX_V, ld >= V, any n >= 0, 0 <= t < T <= SUBGC_RULES_MAX_T (T: the row stride of seq),
 * 0 <= n_bad <= SUBGC_RULES_MAX_BAD, flags within SUBGC_RULE_ALL; each refusal names the number.  The pick kernels then run on the
 * ruled row with raw_logits = 0.                                                                                                     */
int subgc_decode_rules(float* logits, int64_t ld, int n, int V, const int64_t* seq, int T, int t, int flags, float trigram_pen,
                       const int32_t* bad_ids, int n_bad, int32_t* stats, const int32_t* prev_count, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SUBGC_DECODE_RULES_HIP_H */
