/*
 * subgc_control_input_hip.h -- the input side of the controllability experiment in libsubgc_hip.so (gfx950): from a user's control
 * signal (a set of region boxes per wanted caption) to the sub-graph rows the `sct` decode reads.
 *
 * The ninth public header.  subgc_hip.h is the model's drop-in boundary; subgc_metrics_hip.h, subgc_grounding_hip.h,
 * subgc_controllability_hip.h, subgc_criterion_hip.h, subgc_selfcritical_hip.h, subgc_consensus_hip.h and subgc_forced_hip.h stay as
 * they are.  Same library, same contract as those: every function returns 0 (SUBGC_OK) or a negative SUBGC_E* code with the text in
 * subgc_last_error(), never allocates device memory and never synchronises the device, enqueues on `stream` (a hipStream_t passed as
 * void*) and can be captured into a hipGraph, all pointers are BORROWED device pointers, outputs are caller-allocated, everything is per
 * call and there is no global state.  subgc_version() does not change with this header.
 *
 * What is replaced: dataloaders/dataloader_test_sct.py `DataLoader.__getitem__`
 *   dataloader_test_sct.py:207-228   bb_intersection_over_union, as numpy >= 2 evaluates it on fp32 rows (fp32 areas, fp32 quotient);
 *   dataloader_test_sct.py:261-295   the triple loop region x detection box, the IoU >= 0.5 / best-match filter;
 *   dataloader_test_sct.py:314-355   --use_greedy_subg: seed nodes -> their classes' nodes -> touching relations -> their endpoints;
 *   dataloader_test_sct.py:356-368   --use_gt_subg: the precomputed sub-graph whose seed set equals the matched set.
 * (:371-380, the rows of the chosen precomputed sub-graph, are subgc_mask_compact / subgc_pad_segments_i64 of subgc_hip.h.)
 * No float atomics; integers and wave intrinsics only, so equal inputs give equal bits whatever the batch.
 *
 * Shared conventions.  B images; image b owns the region sets set_off[b] .. set_off[b+1]-1 (set_off [B + 1] int64, ascending from 0 to
 * n_sets) and n_obj detection boxes / nodes, 1 <= n_obj <= SUBGC_SCT_MAX_OBJ: one lane of a wave64 each.  A node set is a 64-bit mask,
 * bit k = node k.  One wave per region set in every kernel.  status [n_sets] int32: SUBGC_SCT_OK, SUBGC_SCT_NO_OVERLAP or
 * SUBGC_SCT_NO_GT.  Inputs are taken as finite (the host module refuses non-finite boxes): a NaN IoU never matches.
 * Not built: the numpy 1.x evaluation of :225 (an fp64 quotient), and the "keep all SG nodes" branch of :290-291, which the reference
 * cannot reach (np.max of an empty list raises before it).
 */
#ifndef SUBGC_CONTROL_INPUT_HIP_H
#define SUBGC_CONTROL_INPUT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SUBGC_SCT_MAX_OBJ 64        /* detection boxes / nodes of an image: one lane each */
#define SUBGC_SCT_MAX_REGIONS 64    /* rows R of a region set */
#define SUBGC_SCT_MAX_REL 1024      /* rel_num: 16 chunks of 64 relations */
#define SUBGC_SCT_GT_LISTS 5        /* precomputed ground-truth sub-graphs per image (subgraph_mask_list[:5]) */

#define SUBGC_SCT_OK 0
#define SUBGC_SCT_NO_OVERLAP 1      /* no region of the set overlaps any detection box: the reference raises ValueError (np.max([]), :289) */
#define SUBGC_SCT_NO_GT 2           /* no precomputed seed list equals the matched set: the reference indexes with None (:371) */

/* dataloader_test_sct.py:261-295 for every region set.
 *   boxes [B, n_obj, 4] fp32: the detector's boxes (x1, y1, x2, y2); img_wh [B, 2] fp32: (w, h).  Box k of image b is scaled as :263
 *     does, `boxes * max(w, h) / 592` in fp32: one rounded product, then one correctly rounded (IEEE) division.
 *   regions [n_sets, R, 5] fp32: x1, y1, x2, y2, flag.  The valid regions of a set are its FIRST v rows, v = the number of rows whose
 *     flag is non-zero (:271-272).
 *   IoU (:207-228), fp32, every operation rounded on its own (no FMA contraction), in the reference's order and `+ 1` convention:
 *     xA = max(r.x1, d.x1), yA = max(r.y1, d.y1), xB = min(r.x2, d.x2), yB = min(r.y2, d.y2);
 *     iw = (xB - xA) + 1, ih = (yB - yA) + 1, each replaced by 0 when not > 0; inter = iw * ih;
 *     areaA = ((r.x2 - r.x1) + 1) * ((r.y2 - r.y1) + 1), areaB likewise; iou = inter / ((areaA + areaB) - inter), correctly rounded.
 *     This is NOT the grounding evaluators' IoU (bbox_transform.py:194-220): no degenerate-box rules.
 *   Region j < v is matched to the detection box of the largest IoU under the reference's strict `>` starting from 0 (:276-282): equal
 *     maxima go to the LOWEST box index, a maximum of 0 (or an unordered one) leaves the region unmatched.
 *   Filter (:287-293): the matched regions with IoU >= 0.5; when there are none, the matched regions that reach the set's best IoU.
 * Outputs: seed_mask [n_sets] uint64 = the nodes of the kept matches (a node matched twice is one bit); match_idx [n_sets, R] int32 and
 *   match_iou [n_sets, R] fp32 = per region the matched box and its IoU BEFORE the filter, -1 and 0 for an unmatched or invalid row;
 *   status [n_sets] = SUBGC_SCT_NO_OVERLAP when no region is matched (seed_mask 0), else SUBGC_SCT_OK.  Every element is written.
 * 1 <= n_obj <= SUBGC_SCT_MAX_OBJ and 1 <= R <= SUBGC_SCT_MAX_REGIONS are refused otherwise, with the number in the text.          */
int subgc_sct_match(const float* boxes, const float* img_wh, int B, int n_obj, const float* regions, const int64_t* set_off, int n_sets,
                    int R, uint64_t* seed_mask, int32_t* match_idx, float* match_iou, int32_t* status, void* stream);

/* dataloader_test_sct.py:314-355 for every region set, from subgc_sct_match's seed_mask and status.
 *   object_dist [B, n_obj, C] fp32 -> object_cls [B, n_obj] int32 (an OUTPUT, written by a launch of its own in front): the FIRST
 *     maximum of every row (np.argmax, :265).
 *   rel_ind [sum_k, 2] int64 with rel_off [B + 1] int64: image b's relations are rows rel_off[b] .. rel_off[b+1]-1, at most rel_num - 1
 *     of them are read (the host module refuses more: the reference's row assignment :352 cannot hold them).
 *   Nodes: the seeds, then every node whose class equals a seed's class (:321-325).  Relations, in chunks of 64 with one lane each: kept
 *     when an endpoint is one of those nodes (:328-333; an endpoint outside [0, n_obj) touches nothing).  The kept relations' endpoints
 *     join the nodes (:336).  A node's new id is the number of kept nodes below it (:340-343).
 *   Rows per set, every element written:
 *     gpn_obj_ind [n_sets, obj_num] int64: the kept node ids ascending, then obj_num - 1;  att_masks [n_sets, obj_num] fp32: 1 on that
 *     prefix, then 0;  gpn_pool_mtx [n_sets, obj_num, obj_num] fp32: 1 on the prefix of the diagonal (may be NULL, like
 *     subgc_mask_compact);  gpn_pred_ind [n_sets, rel_num] int64: the kept relation rows ascending, then rel_num - 1;
 *     gpn_nrel_ind [n_sets, rel_num, 2] int64: the kept relations' renumbered endpoints in relation order, then obj_num - 1.
 *   A set whose status is not SUBGC_SCT_OK gets the padding values alone.
 * n_obj <= min(SUBGC_SCT_MAX_OBJ, obj_num - 1), 2 <= rel_num <= SUBGC_SCT_MAX_REL, C >= 1.                                          */
int subgc_sct_extract_greedy(const float* object_dist, int C, const int64_t* rel_ind, const int64_t* rel_off, int B, int n_obj,
                             const int64_t* set_off, const uint64_t* seed_mask, const int32_t* status, int n_sets, int obj_num,
                             int rel_num, int32_t* object_cls, int64_t* gpn_obj_ind, float* att_masks, float* gpn_pool_mtx,
                             int64_t* gpn_pred_ind, int64_t* gpn_nrel_ind, void* stream);

/* dataloader_test_sct.py:356-368 for every region set, from subgc_sct_match's seed_mask.
 *   gt_seed [n_seed] int64 with gt_seed_off [B * SUBGC_SCT_GT_LISTS + 1] int64: list j of image b (`mask[4]` of subgraph_mask_list[j],
 *     j < 5) is gt_seed[gt_seed_off[5 b + j] .. gt_seed_off[5 b + j + 1]); repeats allowed (np.unique, :361), ids outside [0, n_obj)
 *     belong to no node set and make the list equal to none.
 *   choice [n_sets] int32 = the FIRST j whose set of distinct nodes equals the set's seed_mask, compared as 64-bit masks; -1 when there
 *     is none or the set's status is not SUBGC_SCT_OK.
 *   status [n_sets], read and written: SUBGC_SCT_OK becomes SUBGC_SCT_NO_GT when no list is equal; other values stay.
 * The rows of sub-graph 5 b + choice then come from subgc_mask_compact / subgc_pad_segments_i64 (:371-380).                          */
int subgc_sct_gt_lookup(const int64_t* gt_seed, const int64_t* gt_seed_off, int n_seed, int B, int n_obj, const int64_t* set_off,
                        const uint64_t* seed_mask, int n_sets, int32_t* choice, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SUBGC_CONTROL_INPUT_HIP_H */
