/*
 * subgc_controllability_hip.h -- the set-controllability entry point of libsubgc_hip.so (gfx950): Noun IoU of a decode batch.
 *
 * The fourth public header.  subgc_hip.h is the model's drop-in boundary, subgc_metrics_hip.h holds the accuracy scores and
 * subgc_grounding_hip.h the grounding scores; all three stay as they are.  Same library, same contract as those: every function returns 0
 * (SUBGC_OK) or a negative SUBGC_E* code with the text in subgc_last_error(), never allocates device memory and never synchronises the
 * device (debug bounds mode excepted, subgc_debug_bounds), enqueues on `stream` (a hipStream_t passed as void*), all pointers are BORROWED
 * device pointers, outputs are caller-allocated, and there is no global state.  subgc_version() does not change with this header.
 *
 * What is replaced (the set-controllability table; `test.py --sct 1` writes the captions):
 *   misc/controllability/noun_iou.py:14-17                   prep_seq: the words of a caption that have a vector, repeats kept
 *   misc/controllability/noun_iou.py:19-47                   NounIoU.score: cosine similarities, (s + 1) / 2, a maximum-weight assignment
 *                                                            of min(m, n) pairs (munkres), iou = I / (m + n - I)
 *   misc/controllability/controllability_score.py:40-52,74   the group mean per generated caption (the corpus mean is taken on the host)
 * Words are integer rows of a vector table cooked once on the host.  BLEU / ROUGE-L / CIDEr of the same groups (lines 54-69) are
 * subgc_accuracy_rows of subgc_metrics_hip.h with the group in the place of the image.
 * No float atomics; the order of every sum is fixed by the inputs: equal inputs give equal bits, the assignment included.
 * Out of scope: METEOR and SPICE (Java), PTB tokenisation.
 */
#ifndef SUBGC_CONTROLLABILITY_HIP_H
#define SUBGC_CONTROLLABILITY_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SUBGC_CTL_MAX_WORDS 64    /* vector words of a caption, on either side: one wave owns one column per lane */

/* subgc_control_noun_iou (noun_iou.py:19-47, controllability_score.py:47-52): per token row the mean Noun IoU against the ground-truth
 * captions of its group.  One launch; one workgroup per row, one wave per (row, caption) pair.
 *   tok [rows, T] int32 (tok64 = 0) or int64 (1), 1 <= T <= SUBGC_CTL_MAX_WORDS: the generated captions.  A row's words are those before
 *     the first id <= 0, minus trailing words w with bad[w] != 0 unless every word is one (bad NULL: no trimming; misc/utils.py:74-80,
 *     the rule of subgc_consensus_cook / subgc_grounding_material).
 *   tok_noun [n_tok_noun]: word id -> row of the vector table, -1 = the word has no vector; an id outside the table, or a value outside
 *     [0, n_noun), has none.  The n predicted words are the row's words that have a vector, in sentence order, repeats kept.
 *   vec [n_noun, d] fp32, d >= 1: the vectors; norm [n_noun] fp64: their Euclidean norms, computed once at cook time.
 *   row_group [rows]: the ground-truth group of each row (0 .. n_groups - 1).  -1, or any other value outside that range, is "no group":
 *     iou[r] = 0 and every pair slot of the row is written as 0 / -1.
 *   Reference tables: group g owns captions gcap_off[g] .. gcap_off[g+1]-1 (n_caps in all); caption c the vector rows
 *     gn[gn_off[c] .. gn_off[c+1]) (n_gn in all; at most SUBGC_CTL_MAX_WORDS are read), in sentence order with repeats: its m words.
 *   pair_off [rows + 1]: row r's pairs are pair_off[r] .. pair_off[r+1]-1, pair q of them being the q-th caption of its group (the host
 *     forms pair_off from gcap_off; n_pairs = pair_off[rows]).  Slots beyond the group's captions are written as 0 / -1 and not counted.
 * Outputs:
 *   pair_mn [n_pairs, 2] int32: the m and n that were used;  pair_iou [n_pairs] fp32: m == 0 -> 1 (this test comes first); n == 0 -> 0;
 *     else I / ((m + n) - I) with I the sum of the assigned similarities;
 *   assign [n_pairs, SUBGC_CTL_MAX_WORDS] int8: for ground-truth word i < m the predicted word matched to it, else -1 (also beyond m):
 *     exactly min(m, n) entries are >= 0 and no predicted word appears twice;
 *   iou [rows] fp32: the mean of the row's counted pairs (0 when there is none).
 * Arithmetic (FMA contraction is off for the whole file, every operation is rounded on its own):
 *   dot = sum over k = 0 .. d-1, in this order, of (double)a[k] * (double)b[k], accumulated in fp64 (every product is exact);
 *   cos = dot / max(norm_a * norm_b, 1e-8) in fp64, rounded once to fp32;  s = (cos + 1) / 2 in fp32;
 *   the assignment maximises the sum of s over min(m, n) pairs: shortest augmenting paths with dual potentials (the Jonker-Volgenant form
 *     of the Hungarian method), the smaller side as rows, one lane per column, the column minimum of each step taken with ties to the
 *     lowest column index.  Potentials and slacks are fp64 (differences of fp32 entries are exact there), so the result is optimal for
 *     the fp32 matrix up to fp64 rounding of the potentials.  Only the VALUE of the assignment enters the score;
 *   I = the fp32 sum of the chosen s, sequentially over the ground-truth words in ascending order;
 *   iou = I / ((float)(m + n) - I) in fp32, a correctly rounded division;
 *   the group mean = the fp32 sum of the pair values in caption order, sequentially, divided (correctly rounded) by their number.
 * Every index is clamped into its buffer; debug bounds mode checks row_group, pair_off and the offset tables (monotone, inside their
 * buffers) and the gn and tok_noun values against n_noun first and reports instead.                                               */
int subgc_control_noun_iou(const void* tok, int tok64, int T, const uint8_t* bad, int bad_n, int rows, const int32_t* tok_noun, int n_tok_noun,
                           const float* vec, const double* norm, int n_noun, int d, const int32_t* row_group, int n_groups,
                           const int32_t* pair_off, int n_pairs, const int32_t* gcap_off, int n_caps, const int32_t* gn_off, const int32_t* gn,
                           int n_gn, float* iou, float* pair_iou, int32_t* pair_mn, int8_t* assign, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SUBGC_CONTROLLABILITY_HIP_H */
