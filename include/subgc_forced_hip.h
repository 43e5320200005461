/*
 * subgc_forced_hip.h -- forced decode in libsubgc_hip.so (gfx950): a decode that FOLLOWS given tokens, the log-probabilities of those
 * tokens, and from its teacher-forced attention the grounding accuracy on ground-truth sentences.
 *
 * The eighth public header.  subgc_hip.h is the model's drop-in boundary; subgc_metrics_hip.h, subgc_grounding_hip.h,
 * subgc_controllability_hip.h, subgc_criterion_hip.h, subgc_selfcritical_hip.h and subgc_consensus_hip.h stay as they are.  Same library,
 * same contract as those: every function returns 0 (SUBGC_OK) or a negative SUBGC_E* code with the text in subgc_last_error(), never
 * allocates device memory and never synchronises the device (debug bounds mode excepted, subgc_debug_bounds), enqueues on `stream` (a
 * hipStream_t passed as void*) and can be captured into a hipGraph, all pointers are BORROWED device pointers, outputs are
 * caller-allocated, everything is per call and there is no global state.  subgc_version() does not change with this header.
 *
 * What is replaced:
 *   AttModel.py:282-319     the loop of `_sample` with the token choice (:295-316) replaced by a given token: what the reference reaches
 *                           only through its training graph (AttModel.py:122-177 with misc/utils.py:111-124 LanguageModelCriterion), and
 *                           for attention through get_logprobs_state(return_att=True) (AttModel.py:328-340).
 *   misc/grounding/eval_grd_flickr30k_entities.py:63-109   FlickrGrdEval.gt_grd_eval, the evaluator's default mode (`--eval_mode GT`,
 *                           :246): grounding accuracy on ground-truth sentences; the events are lines 70-94, the corpus number line 97.
 *   misc/grd_utils.py:49-60 the {'idx_in_sent','bbox'} list of a sentence, here for EVERY word of a forced row.
 *   misc/grounding/tools/bbox_transform.py:194-220   bbox_overlaps_batch for N = K = 1, shared with subgc_grounding_score.
 * No float atomics; every sum has a fixed order, stated below, so equal inputs give equal bits.  The corpus number (line 97) is formed
 * on the host from the event codes, so it accumulates across batches and ranks.
 * Out of scope: choosing the sub-graph a ground-truth sentence is decoded on (the caller's), CoreNLP, beam search along given tokens.
 */
#ifndef SUBGC_FORCED_HIP_H
#define SUBGC_FORCED_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SUBGC_FORCED_MAX_V 16384   /* columns of a logits row */
#define SUBGC_FORCED_MAX_T 64      /* steps of a forced row (SUBGC_GRD_MAX_WORDS) */

/* event codes of subgc_gt_grounding_score (one byte each); MISS / HIT are SUBGC_GRD_MISS / SUBGC_GRD_HIT */
#define SUBGC_GTG_MISS 0           /* a box was compared: IoU <= iou_thresh (a 0, line 94) */
#define SUBGC_GTG_HIT 1            /* a box was compared: IoU > iou_thresh (a 1, line 94) */
#define SUBGC_GTG_UNGROUNDED 2     /* process_idx is not among the row's idx_in_sent (a 0, lines 86-87) */
#define SUBGC_GTG_NOROW 3          /* the pair has no row: "image not grounded" (a 0, lines 82-83) */
#define SUBGC_GTG_NONE 255         /* padding of an output slot behind SUBGC_GTG_MAX_OBJ objects */
#define SUBGC_GTG_MAX_OBJ 64       /* annotated objects of a reference caption (SUBGC_GRD_MAX_OBJ) */

/* The token filing of one forced decode step (AttModel.py:295-316 with `it` given): subgc_decode_pick's / subgc_sc_pick's contract with
 * the choice replaced by tok = forced[r * ld_f + t].  Row r is LIVE at step t when t == 0 or unfinished[r] != 0 before the step.
 *   seq[r * T + t] = tok for a live row, 0 otherwise; next_tok[r] = the same value; unfinished[r] = live && tok > 0;
 *   seqlp[r * T + t] = lp for a live row, 0 otherwise -- the end token's own step is live and gets its log-probability, as
 *     LanguageModelCriterion's mask counts it (misc/utils.py:115-124);
 *   *n_unfinished = 1 by a plain store when a row is unfinished (a flag, zeroed by the caller; may be NULL); prev_count != NULL and
 *     *prev_count == 0: nothing is written (no row was unfinished after the previous step; AttModel.py:318-319).
 *   raw_logits != 0:  lp = (x[tok] - max) - log(sum_c exp(x[c] - max)), fp32, NO temperature.  The order is subgc_sc_pick's
 *     chunk-then-scan order: max = the maximum of the row; e_c = expf(x[c] - max); lane i of the 256 adds its chunk of
 *     CH = ceil(V / 256) consecutive columns [i * CH, min(V, (i + 1) * CH)) in ascending order; the 256 chunk sums pass an inclusive
 *     scan (the fixed shift-by-1, 2, 4 .. 32 tree inside each wave of 64, then the totals of the waves in front added in wave order)
 *     and the sum is the scan's last element; logf of it; two subtractions.
 *   raw_logits == 0:  lp = x[tok], the row holds log-probabilities.
 * One workgroup of 256 per row, one read of the row (staged in LDS).  V <= SUBGC_FORCED_MAX_V, ld >= V, any n >= 0,
 * 0 <= t < Tf <= SUBGC_FORCED_MAX_T, ld_f >= Tf, T >= Tf (the row stride of seq and seqlp).  A token outside [0, V) is clamped into
 * it; debug bounds mode checks column t of `forced` first and reports instead.                                                       */
int subgc_forced_pick(const float* logits, int64_t ld, int n, int V, const int64_t* forced, int64_t ld_f, int Tf, int t, int64_t* seq,
                      float* seqlp, int T, int64_t* next_tok, int32_t* unfinished, int32_t* n_unfinished, const int32_t* prev_count,
                      int raw_logits, void* stream);

/* Once after the loop, one thread per row: row r's live steps are t = 0 and every t < Tf with seq[r, 0 .. t-1] all > 0 (what
 * subgc_forced_pick filed).  ll[r] (fp64) = the sum of (double) seqlp[r * T + t] over the live steps in ascending t: the caption's
 * log-likelihood; n_tok[r] = the number of live steps (the words and, where the row holds it, the end token).  T >= Tf >= 1.        */
int subgc_forced_finish(const int64_t* seq, const float* seqlp, int T, int n, int Tf, double* ll, int32_t* n_tok, void* stream);

/* misc/grd_utils.py:49-60 for every forced row, EVERY word position: the padded {'idx_in_sent','bbox'} list.
 *   node [rows, T1], n_words [rows]: what subgc_grounding_argmax wrote when called with one row per "image" (seg = 0 .. rows, order and
 *     pick NULL): the box row word position j attended to most, and the words of the row.
 *   row_img [rows]: the row's image among the n_img images of box_off [n_img + 1] / boxes [n_boxes, 4] fp32 (image scale): image i's
 *     boxes are rows box_off[i] .. box_off[i+1]-1.
 *   Entry j < mat_n[r] = min(n_words[r], T1, SUBGC_FORCED_MAX_T): mat_idx[r * ld_m + j] = j, mat_box[(r * ld_m + j) * 4 ..] = the box
 *     of node[r, j], copied bit for bit.  ld_m >= min(T1, SUBGC_FORCED_MAX_T).
 * Every index is clamped into its buffer (a node outside the image's boxes names its nearest box; an image without boxes gives zeros);
 * debug bounds mode checks row_img, box_off and node first and reports instead.                                                      */
int subgc_gt_grounding_material(const int32_t* node, int T1, const int32_t* n_words, int rows, const int32_t* row_img,
                                const int32_t* box_off, int n_img, const float* boxes, int n_boxes, int32_t* mat_n, int32_t* mat_idx,
                                float* mat_box, int ld_m, void* stream);

/* eval_grd_flickr30k_entities.py:70-94: one wave per (reference caption, forced row) pair, one lane per annotated object.
 *   mat_n [rows], mat_idx [rows, ld_m], mat_box [rows, ld_m, 4]: the lists (subgc_gt_grounding_material's, or a finished submission
 *     file's packed the same way: `idx_in_sent` and `bbox` of pred[img][num_sent]); at most SUBGC_FORCED_MAX_T entries are read.
 *   pair_cap [n_pairs]: the pair's reference caption s (0 .. n_caps - 1); it owns the objects obj_off[s] .. obj_off[s+1]-1 (at most
 *     SUBGC_GTG_MAX_OBJ; n_obj in all) with obj_idx (process_idx) and obj_box [n_obj, 4] fp32 (process_bnd_box) -- the tables of
 *     subgc_grounding_score.  pair_row [n_pairs]: its row, or < 0: no row.
 *   out [out_off[p] .. out_off[p+1]): one code per object in annotation order (out_off [n_pairs + 1], n_out bytes in all):
 *     pair_row < 0 -> NOROW; obj_idx not among the row's mat_idx -> UNGROUNDED; else the FIRST entry with that index (`.index`, line
 *     89): HIT when IoU(entry box, object box) > iou_thresh, else MISS.  Slot bytes behind SUBGC_GTG_MAX_OBJ objects: NONE.
 *   IoU: subgc_grounding_score's device function itself (bbox_transform.py:194-220, fp32, every operation rounded on its own -- no FMA
 *     contraction --, correctly rounded division; a GT box with w == 1 and h == 1 -> 0; after that a predicted box with w == 1 and
 *     h == 1 -> -1; a NaN overlap is no hit): the two kernels agree bit for bit.
 * Every index is clamped into its buffer; debug bounds mode checks pair_cap, pair_row (< rows), obj_off and out_off first and reports
 * instead.                                                                                                                            */
int subgc_gt_grounding_score(const int32_t* mat_n, const int32_t* mat_idx, const float* mat_box, int ld_m, int rows,
                             const int32_t* pair_cap, const int32_t* pair_row, int n_pairs, const int32_t* obj_off, int n_caps,
                             const int32_t* obj_idx, const float* obj_box, int n_obj, float iou_thresh, const int32_t* out_off,
                             uint8_t* out, int n_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SUBGC_FORCED_HIP_H */
