// Grounding accuracy on ground-truth sentences (include/subgc_forced_hip.h): FlickrGrdEval.gt_grd_eval
// (misc/grounding/eval_grd_flickr30k_entities.py:63-109).  The forced decode of a reference caption leaves one attention arg-max per word
// (subgc_grounding_argmax, one row per "image"); material_kernel turns it into the {'idx_in_sent','bbox'} list of misc/grd_utils.py:49-60
// for EVERY word, score_kernel writes one byte per annotated object (lines 70-94).  One wave per row / per (caption, row) pair.  The IoU
// is subgc_grounding_score's own device function (grounding_iou.h), compiled here too with FMA contraction off for the whole file.  No
// atomics: every output has one writer.
#include "common.h"

#include "../../include/subgc_forced_hip.h"

#pragma clang fp contract(off)

#include "caption.h"      // after the pragma, like grounding.hip
#include "grounding_iou.h"

namespace {

constexpr int kWords = SUBGC_FORCED_MAX_T;
constexpr int kObj = SUBGC_GTG_MAX_OBJ;

// One wave per forced row; lane j = word position j.
__global__ __launch_bounds__(64) void gt_material_kernel(const int32_t* __restrict__ node, int T1, const int32_t* __restrict__ n_words, int rows,
                                                         const int32_t* __restrict__ row_img, const int32_t* __restrict__ box_off, int n_img,
                                                         const float* __restrict__ boxes, int n_boxes, int32_t* __restrict__ mat_n,
                                                         int32_t* __restrict__ mat_idx, float* __restrict__ mat_box, int ld_m) {
    const int r = blockIdx.x, lane = threadIdx.x;
    int L = n_words[r];
    L = L < T1 ? L : T1;
    L = L < kWords ? L : kWords;
    L = L < ld_m ? L : ld_m;
    L = L < 0 ? 0 : L;
    if (lane == 0) mat_n[r] = L;
    if (lane >= L) return;
    const int i = clampi(row_img[r], 0, n_img - 1);
    const int b0 = clampi(box_off[i], 0, n_boxes), b1 = clampi(box_off[i + 1], b0, n_boxes);
    const int64_t o = (int64_t)r * ld_m + lane;
    mat_idx[o] = lane;
    float4 bx = make_float4(0.f, 0.f, 0.f, 0.f);
    if (b1 > b0) {
        const int64_t q = b0 + clampi(node[(int64_t)r * T1 + lane], 0, b1 - b0 - 1);
        bx = make_float4(boxes[q * 4], boxes[q * 4 + 1], boxes[q * 4 + 2], boxes[q * 4 + 3]);
    }
    mat_box[o * 4] = bx.x;
    mat_box[o * 4 + 1] = bx.y;
    mat_box[o * 4 + 2] = bx.z;
    mat_box[o * 4 + 3] = bx.w;
}

// One wave per (reference caption, forced row) pair; lane = annotated object.
__global__ __launch_bounds__(64) void gt_score_kernel(const int32_t* __restrict__ mat_n, const int32_t* __restrict__ mat_idx,
                                                      const float* __restrict__ mat_box, int ld_m, int rows, const int32_t* __restrict__ pair_cap,
                                                      const int32_t* __restrict__ pair_row, const int32_t* __restrict__ obj_off, int n_caps,
                                                      const int32_t* __restrict__ obj_idx, const float* __restrict__ obj_box, int n_obj,
                                                      float iou_thresh, const int32_t* __restrict__ out_off, uint8_t* __restrict__ out, int n_out) {
    __shared__ int p_idx[kWords];
    const int p = blockIdx.x, lane = threadIdx.x;
    const int s = clampi(pair_cap[p], 0, n_caps - 1);
    const int q0 = clampi(obj_off[s], 0, n_obj), q1 = clampi(obj_off[s + 1], q0, n_obj);
    const int no = q1 - q0 < kObj ? q1 - q0 : kObj;
    const int row = pair_row[p] < rows ? pair_row[p] : rows - 1;          // < 0: the pair has no row
    const int cap_m = ld_m < kWords ? ld_m : kWords;
    const int np = row >= 0 ? clampi(mat_n[row], 0, cap_m) : 0;
    const int64_t mb = (int64_t)(row >= 0 ? row : 0) * ld_m;
    p_idx[lane] = lane < np ? mat_idx[mb + lane] : -1;
    __syncthreads();
    const int g0 = clampi(out_off[p], 0, n_out), g1 = clampi(out_off[p + 1], g0, n_out);
    if (g0 + lane < g1) {
        uint8_t code = SUBGC_GTG_NONE;
        if (lane < no) {
            if (row < 0) {
                code = SUBGC_GTG_NOROW;
            } else {
                const int want = obj_idx[q0 + lane];
                int first = -1;
                for (int k = 0; k < np; ++k)
                    if (p_idx[k] == want) { first = k; break; }
                if (first < 0) {
                    code = SUBGC_GTG_UNGROUNDED;
                } else {
                    const float* pb = mat_box + (mb + first) * 4;
                    const float* gb = obj_box + (int64_t)(q0 + lane) * 4;
                    const float ov = subgc_grounding_iou(make_float4(pb[0], pb[1], pb[2], pb[3]), make_float4(gb[0], gb[1], gb[2], gb[3]));
                    code = ov > iou_thresh ? SUBGC_GTG_HIT : SUBGC_GTG_MISS;
                }
            }
        }
        out[g0 + lane] = code;
    }
    for (int q = g0 + 64 + lane; q < g1; q += 64) out[q] = SUBGC_GTG_NONE;     // a slot longer than a wave: padding
}

}  // namespace

SUBGC_API int subgc_gt_grounding_material(const int32_t* node, int T1, const int32_t* n_words, int rows, const int32_t* row_img,
                                          const int32_t* box_off, int n_img, const float* boxes, int n_boxes, int32_t* mat_n, int32_t* mat_idx,
                                          float* mat_box, int ld_m, void* stream) {
    SUBGC_REQUIRE(rows >= 0 && n_img >= 0 && n_boxes >= 0, "gt_grounding_material: rows, n_img, n_boxes >= 0");
    SUBGC_REQUIRE(T1 >= 1, "gt_grounding_material: T1 >= 1 (got %d)", T1);
    SUBGC_REQUIRE(ld_m >= (T1 < kWords ? T1 : kWords), "gt_grounding_material: ld_m = %d is shorter than min(T1, %d) = %d", ld_m, kWords,
                  T1 < kWords ? T1 : kWords);
    if (rows == 0) return SUBGC_OK;
    SUBGC_REQUIRE(n_img >= 1, "gt_grounding_material: rows without an image");
    SUBGC_REQUIRE(node && n_words && row_img && box_off && mat_n && mat_idx && mat_box && (n_boxes == 0 || boxes), "gt_grounding_material: null pointer");
    hipStream_t s = (hipStream_t)stream;
    SUBGC_DEBUG_RANGE(row_img, 4, 1, rows, rows, 0, (int64_t)n_img - 1, -1, "gt_grounding_material: row_img (image of every forced row)", s);
    SUBGC_DEBUG_MONO("gt_grounding_material", "box_off (box rows of the images)", "position", box_off, n_img, n_boxes, s);
    SUBGC_DEBUG_RANGE(node, 4, rows, T1, T1, 0, n_boxes > 0 ? (int64_t)n_boxes - 1 : 0, -1, "gt_grounding_material: node (box row of every word position)", s);
    hipLaunchKernelGGL(gt_material_kernel, dim3(rows), dim3(64), 0, s, node, T1, n_words, rows, row_img, box_off, n_img, boxes, n_boxes, mat_n, mat_idx,
                       mat_box, ld_m);
    return subgc::check_launch("subgc_gt_grounding_material");
}

SUBGC_API int subgc_gt_grounding_score(const int32_t* mat_n, const int32_t* mat_idx, const float* mat_box, int ld_m, int rows,
                                       const int32_t* pair_cap, const int32_t* pair_row, int n_pairs, const int32_t* obj_off, int n_caps,
                                       const int32_t* obj_idx, const float* obj_box, int n_obj, float iou_thresh, const int32_t* out_off,
                                       uint8_t* out, int n_out, void* stream) {
    SUBGC_REQUIRE(rows >= 0 && n_pairs >= 0 && n_caps >= 0 && n_obj >= 0 && n_out >= 0, "gt_grounding_score: rows, n_pairs, n_caps, n_obj, n_out >= 0");
    SUBGC_REQUIRE(ld_m >= 1, "gt_grounding_score: ld_m >= 1 (got %d)", ld_m);
    if (n_pairs == 0) return SUBGC_OK;
    SUBGC_REQUIRE(n_caps >= 1, "gt_grounding_score: pairs without a reference caption");
    SUBGC_REQUIRE(pair_cap && pair_row && obj_off && out_off && (rows == 0 || (mat_n && mat_idx && mat_box)) && (n_obj == 0 || (obj_idx && obj_box)) &&
                      (n_out == 0 || out),
                  "gt_grounding_score: null pointer");
    hipStream_t s = (hipStream_t)stream;
    SUBGC_DEBUG_RANGE(pair_cap, 4, 1, n_pairs, n_pairs, 0, (int64_t)n_caps - 1, -1, "gt_grounding_score: pair_cap (reference caption of every pair)", s);
    SUBGC_DEBUG_RANGE(pair_row, 4, 1, n_pairs, n_pairs, (int64_t)INT32_MIN, (int64_t)rows - 1, (int64_t)INT32_MIN - 1, "gt_grounding_score: pair_row (forced row of every pair)", s);
    SUBGC_DEBUG_MONO("gt_grounding_score", "obj_off (CSR object offsets)", "position", obj_off, n_caps, n_obj, s);
    SUBGC_DEBUG_MONO("gt_grounding_score", "out_off (event offsets)", "position", out_off, n_pairs, n_out, s);
    hipLaunchKernelGGL(gt_score_kernel, dim3(n_pairs), dim3(64), 0, s, mat_n, mat_idx, mat_box, ld_m, rows, pair_cap, pair_row, obj_off, n_caps, obj_idx,
                       obj_box, n_obj, iou_thresh, out_off, out, n_out);
    return subgc::check_launch("subgc_gt_grounding_score");
}
