/*
 * subgc_grounding_hip.h -- the grounding-score entry points of libsubgc_hip.so (gfx950): F1_all / F1_loc material of a decode batch.
 *
 * The third public header.  subgc_hip.h is the model's drop-in boundary and subgc_metrics_hip.h holds the accuracy scores; both stay as
 * they are.  Same library, same contract as those: every function returns 0 (SUBGC_OK) or a negative SUBGC_E* code with the text in
 * subgc_last_error(), never allocates device memory and never synchronises the device (debug bounds mode excepted, subgc_debug_bounds),
 * enqueues on `stream` (a hipStream_t passed as void*), all pointers are BORROWED device pointers, outputs are caller-allocated, and
 * there is no global state.  subgc_version() does not change with this header.
 *
 * What is replaced (the Flickr30k-Entities grounding table):
 *   misc/grd_utils.py:49-60                  the word -> lemma -> detection class look-ups that fill {'clss','idx_in_sent','bbox'}
 *   misc/grounding/grounding_score.py -> misc/grounding/eval_grd_flickr30k_entities.py:129-198   FlickrGrdEval.grd_eval, modes 'all' and
 *                                            'loc', for one submission entry per image
 *   misc/grounding/tools/bbox_transform.py:194-220   bbox_overlaps_batch for N = K = 1
 * Classes, lemmas and words are integer ids cooked once on the host (Stanford CoreNLP is consulted for reference tokens and class words
 * only, at cook time); every match is an integer comparison.  The IoU is fp32 in the reference's operation order, every operation
 * rounded separately (no FMA contraction, correctly rounded division); no float atomics; the order of every output is fixed by the
 * inputs: equal inputs give equal bits.  Corpus numbers (lines 200-205) are formed on the host from the event codes, so they accumulate
 * across batches and ranks.
 * Out of scope: gt_grd_eval (boxes on ground-truth sentences, lines 63-109), CoreNLP itself, the controllability scores.
 */
#ifndef SUBGC_GROUNDING_HIP_H
#define SUBGC_GROUNDING_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* event codes (one byte each) */
#define SUBGC_GRD_MISS 0          /* a box was compared: IoU <= iou_thresh (a 0 in both modes) */
#define SUBGC_GRD_HIT 1           /* a box was compared: IoU > iou_thresh (a 1 in both modes) */
#define SUBGC_GRD_SKIP 2          /* precision: the class is not annotated but excused by an un-annotated token's lemma (line 164-165) */
#define SUBGC_GRD_HALLUCINATED 3  /* precision: a 0 in mode 'all', nothing in mode 'loc' (line 166-168) */
#define SUBGC_GRD_ABSENT 4        /* recall: the class is not predicted: a 0 in mode 'all', nothing in mode 'loc' (line 196-198) */
#define SUBGC_GRD_NONE 255        /* padding of a precision slot behind the image's predicted words */

#define SUBGC_GRD_MAX_WORDS 64    /* predicted words of an image (the decode's T <= 64) */
#define SUBGC_GRD_MAX_OBJ 64      /* annotated objects of a reference caption */

/* subgc_grounding_material (misc/grd_utils.py:49-60): per batch image the padded list {'clss','idx_in_sent','bbox'} of its chosen caption.
 *   tok [rows, T] int32 (tok64 = 0) or int64 (1), T <= 64: the RANKED token rows (subgc_eval_rank_rows' seq_sorted); image i owns rows
 *     seg[i] .. seg[i+1]-1 and its chosen caption is row seg[i] + pick[i] (pick NULL: 0), the caption subgc_grounding_argmax described.
 *   The words considered are those before the first id <= 0, minus trailing words w with bad[w] != 0 unless every word is one (bad NULL:
 *     no trimming; misc/utils.py:74-80, the rule of subgc_consensus_cook), cut at n_words[i] and at T1: `sent.split()` and
 *     `[:len(node_ind)]`.
 *   node [I, T1]: the box row every word position attended to (subgc_grounding_argmax); n_words [I].
 *   tok_class [n_tok_class]: vocabulary id -> class id, -1 = the word names no detection class (wd_to_lemma, lemma_det_id_dict,
 *     det_id_to_det_wd folded into one table); an id outside the table names none.
 *   box_off [I + 1], boxes [n_boxes, 4] fp32: image i's boxes in image scale are rows box_off[i] .. box_off[i+1]-1.
 *   Outputs, in word order as tmp_result is filled: mat_n [I] the count, mat_cls / mat_idx [I, ld_m] class id and word index,
 *     mat_box [I, ld_m, 4] the box of the word's node, copied bit for bit.  ld_m >= min(T, T1).  An image without rows gets count 0.
 * Every index is clamped into its buffer (a node outside the image's boxes names its nearest box; an image without boxes gives zeros);
 * debug bounds mode checks seg, pick, box_off and node first and reports instead.                                                     */
int subgc_grounding_material(const void* tok, int tok64, int T, const uint8_t* bad, int bad_n, int rows, const int32_t* seg,
                             const int32_t* pick, int I, const int32_t* node, int T1, const int32_t* n_words, const int32_t* tok_class,
                             int n_tok_class, const int32_t* box_off, const float* boxes, int n_boxes, int32_t* mat_n, int32_t* mat_cls,
                             int32_t* mat_idx, float* mat_box, int ld_m, void* stream);

/* subgc_grounding_score (eval_grd_flickr30k_entities.py:129-198): the precision and recall events of every (batch image, reference
 * caption of its image) pair, one wave per pair.
 *   mat_n / mat_cls / mat_box with ld_m: the lists subgc_grounding_material wrote (at most SUBGC_GRD_MAX_WORDS entries are read).
 *   img_ref [I]: batch image i's image in the reference tables (0 .. n_ref - 1); pair_off [I + 1]: its pairs are pair_off[i] ..
 *     pair_off[i+1]-1, pair q of them being its q-th reference caption (the host forms pair_off from cap_off; n_pairs = pair_off[I]).
 *   Reference tables: image j owns captions cap_off[j] .. cap_off[j+1]-1 (n_caps in all); caption s the objects obj_off[s] ..
 *     obj_off[s+1]-1 (at most SUBGC_GRD_MAX_OBJ; n_obj in all) with obj_cls (process_clss as class ids), obj_idx (process_idx) and
 *     obj_box [n_obj, 4] fp32 (process_bnd_box); ex_lemma [ex_off[s] .. ex_off[s+1]) the ascending lemma ids of its un-annotated
 *     non-empty tokens (exclude_obj, lines 147-149); class_lemma [n_class]: the lemma id of every class word.
 *   Precision events (lines 151-168), pair p: prec [prec_off[p] .. prec_off[p+1]), event k for the image's k-th predicted word
 *     (k < min(mat_n, slot length); the rest of the slot holds SUBGC_GRD_NONE): the class is among the caption's -> its object with the
 *     smallest word index, HIT / MISS by IoU > iou_thresh; else class_lemma[class] among ex_lemma -> SKIP; else HALLUCINATED.
 *   Recall events (lines 180-198), pair p: rec [rec_off[p] .. rec_off[p+1]), one per object in annotation order: the class is predicted
 *     -> its FIRST predicted entry, HIT / MISS; else ABSENT.
 *   IoU (bbox_transform.py:194-220, N = K = 1, fp32): w = x2 - x1 + 1, h = y2 - y1 + 1; iw, ih clamped at 0;
 *     ua = (area_pred + area_gt) - iw * ih; overlap = (iw * ih) / ua; a GT box with w == 1 and h == 1 -> 0; after that a predicted box
 *     with w == 1 and h == 1 -> -1.  A NaN overlap is no hit.
 * Every index is clamped into its buffer; debug bounds mode checks img_ref, pair_off and the offset tables (monotone, inside their
 * buffers) first and reports instead.                                                                                              */
int subgc_grounding_score(const int32_t* mat_n, const int32_t* mat_cls, const float* mat_box, int ld_m, int I, const int32_t* img_ref,
                          int n_ref, const int32_t* pair_off, int n_pairs, const int32_t* cap_off, int n_caps, const int32_t* obj_off,
                          const int32_t* obj_cls, const int32_t* obj_idx, const float* obj_box, int n_obj, const int32_t* ex_off,
                          const int32_t* ex_lemma, int n_ex, const int32_t* class_lemma, int n_class, float iou_thresh,
                          const int32_t* prec_off, uint8_t* prec, int n_prec, const int32_t* rec_off, uint8_t* rec, int n_rec,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SUBGC_GROUNDING_HIP_H */
