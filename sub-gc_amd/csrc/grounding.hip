// Grounding scores of a decode batch (include/subgc_grounding_hip.h): the {'clss','idx_in_sent','bbox'} lists of the chosen captions
// (misc/grd_utils.py:49-60) and the precision / recall events of FlickrGrdEval.grd_eval (misc/grounding/eval_grd_flickr30k_entities.py:
// 129-198) with the IoU of bbox_overlaps_batch (misc/grounding/tools/bbox_transform.py:194-220).  Two kernels of one wave per unit of
// work: a lane per word position (material), a lane per predicted word and then per annotated object (score).  Classes, lemmas and words
// are integer ids; the IoU is fp32 in the reference's operation order with FMA contraction off for the whole file and a correctly
// rounded division, so a hit (`> iou_thresh` on that fp32 value) is the reference's hit.  No atomics: every output has one writer.
#include "common.h"

#include "../../include/subgc_grounding_hip.h"

#pragma clang fp contract(off)

#include "caption.h"      // after the pragma: its functions are compiled without contraction here
#include "grounding_iou.h" // the IoU, shared with grounding_gt.hip

namespace {

constexpr int kWords = SUBGC_GRD_MAX_WORDS;
constexpr int kObj = SUBGC_GRD_MAX_OBJ;

// One wave per batch image; lane j = word position j.  The grounded words are compacted in word order by a ballot prefix count.
__global__ __launch_bounds__(64) void material_kernel(const void* __restrict__ tok, int tok64, int T, const uint8_t* __restrict__ bad, int bad_n, int rows,
                                                      const int32_t* __restrict__ seg, const int32_t* __restrict__ pick, int I,
                                                      const int32_t* __restrict__ node, int T1, const int32_t* __restrict__ n_words,
                                                      const int32_t* __restrict__ tok_class, int n_tok_class, const int32_t* __restrict__ box_off,
                                                      const float* __restrict__ boxes, int n_boxes, int32_t* __restrict__ mat_n,
                                                      int32_t* __restrict__ mat_cls, int32_t* __restrict__ mat_idx, float* __restrict__ mat_box, int ld_m) {
    const int i = blockIdx.x, lane = threadIdx.x;
    const int a = clampi(seg[i], 0, rows), b = clampi(seg[i + 1], a, rows);
    if (b <= a) {
        if (lane == 0) mat_n[i] = 0;
        return;
    }
    const int r = a + clampi(pick ? pick[i] : 0, 0, b - a - 1);
    int64_t v;
    int L = load_row(tok, tok64, T, r, bad, bad_n, lane, v);
    const int nw = n_words[i];
    L = L < nw ? L : nw;
    L = L < T1 ? L : T1;
    L = L < ld_m ? L : ld_m;
    int cls = -1;
    if (lane < L && v > 0 && v < n_tok_class) cls = tok_class[v];
    const unsigned long long m = __ballot(cls >= 0);
    if (lane == 0) mat_n[i] = __popcll(m);
    if (cls < 0) return;
    const int k = __popcll(m & ((1ull << lane) - 1ull));
    const int b0 = clampi(box_off[i], 0, n_boxes), b1 = clampi(box_off[i + 1], b0, n_boxes);
    const int64_t o = (int64_t)i * ld_m + k;
    mat_cls[o] = cls;
    mat_idx[o] = lane;
    float4 bx = make_float4(0.f, 0.f, 0.f, 0.f);
    if (b1 > b0) {
        const int64_t q = b0 + clampi(node[(int64_t)i * T1 + lane], 0, b1 - b0 - 1);
        bx = make_float4(boxes[q * 4], boxes[q * 4 + 1], boxes[q * 4 + 2], boxes[q * 4 + 3]);
    }
    mat_box[o * 4] = bx.x;
    mat_box[o * 4 + 1] = bx.y;
    mat_box[o * 4 + 2] = bx.z;
    mat_box[o * 4 + 3] = bx.w;
}

// One wave per (batch image, reference caption) pair.
__global__ __launch_bounds__(64) void score_kernel(const int32_t* __restrict__ mat_n, const int32_t* __restrict__ mat_cls, const float* __restrict__ mat_box,
                                                   int ld_m, int I, const int32_t* __restrict__ img_ref, int n_ref, const int32_t* __restrict__ pair_off,
                                                   int n_pairs, const int32_t* __restrict__ cap_off, int n_caps, const int32_t* __restrict__ obj_off,
                                                   const int32_t* __restrict__ obj_cls, const int32_t* __restrict__ obj_idx,
                                                   const float* __restrict__ obj_box, int n_obj, const int32_t* __restrict__ ex_off,
                                                   const int32_t* __restrict__ ex_lemma, int n_ex, const int32_t* __restrict__ class_lemma, int n_class,
                                                   float iou_thresh, const int32_t* __restrict__ prec_off, uint8_t* __restrict__ prec, int n_prec,
                                                   const int32_t* __restrict__ rec_off, uint8_t* __restrict__ rec, int n_rec) {
    __shared__ int p_cls[kWords];
    __shared__ int o_cls[kObj], o_idx[kObj];
    const int p = blockIdx.x, lane = threadIdx.x;
    // the pair's batch image: the last i with pair_off[i] <= p (a pair_off that is not monotone names some image; nothing is read out of range)
    int lo = 0, hi = I - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (pair_off[mid] <= p) lo = mid; else hi = mid - 1;
    }
    const int i = lo;
    const int j = clampi(img_ref[i], 0, n_ref - 1);
    const int c0 = clampi(cap_off[j], 0, n_caps - 1), c1 = clampi(cap_off[j + 1], c0, n_caps);
    const int s = clampi(c0 + (p - pair_off[i]), c0, c1 > c0 ? c1 - 1 : c0);
    const int q0 = clampi(obj_off[s], 0, n_obj), q1 = clampi(obj_off[s + 1], q0, n_obj);
    const int no = q1 - q0 < kObj ? q1 - q0 : kObj;
    const int e0 = clampi(ex_off[s], 0, n_ex), e1 = clampi(ex_off[s + 1], e0, n_ex);
    const int cap_m = ld_m < kWords ? ld_m : kWords;
    const int np = clampi(mat_n[i], 0, cap_m);
    const int64_t mb = (int64_t)i * ld_m;
    p_cls[lane] = lane < np ? mat_cls[mb + lane] : -1;
    o_cls[lane] = lane < no ? obj_cls[q0 + lane] : -2;
    o_idx[lane] = lane < no ? obj_idx[q0 + lane] : 0;
    __syncthreads();
    // precision: lane = predicted word
    const int f0 = clampi(prec_off[p], 0, n_prec), f1 = clampi(prec_off[p + 1], f0, n_prec);
    if (f0 + lane < f1) {
        uint8_t code = SUBGC_GRD_NONE;
        if (lane < np) {
            const int cls = p_cls[lane];
            int best = -1, best_idx = 0;
            for (int q = 0; q < no; ++q)
                if (o_cls[q] == cls && (best < 0 || o_idx[q] < best_idx)) { best = q; best_idx = o_idx[q]; }
            if (best >= 0) {
                const float* pb = mat_box + (mb + lane) * 4;
                const float* gb = obj_box + (int64_t)(q0 + best) * 4;
                const float ov = subgc_grounding_iou(make_float4(pb[0], pb[1], pb[2], pb[3]), make_float4(gb[0], gb[1], gb[2], gb[3]));
                code = ov > iou_thresh ? SUBGC_GRD_HIT : SUBGC_GRD_MISS;
            } else {
                const int lem = class_lemma[clampi(cls, 0, n_class - 1)];
                int x0 = e0, x1 = e1;                                       // first excluded lemma that is not below lem
                while (x0 < x1) {
                    const int mid = (x0 + x1) >> 1;
                    if (ex_lemma[mid] < lem) x0 = mid + 1; else x1 = mid;
                }
                code = (x0 < e1 && ex_lemma[x0] == lem) ? SUBGC_GRD_SKIP : SUBGC_GRD_HALLUCINATED;
            }
        }
        prec[f0 + lane] = code;
    }
    for (int q = f0 + 64 + lane; q < f1; q += 64) prec[q] = SUBGC_GRD_NONE;   // a slot longer than a wave: padding
    // recall: lane = annotated object
    const int g0 = clampi(rec_off[p], 0, n_rec), g1 = clampi(rec_off[p + 1], g0, n_rec);
    if (g0 + lane < g1) {
        uint8_t code = SUBGC_GRD_ABSENT;
        if (lane < no) {
            const int cls = o_cls[lane];
            int first = -1;
            for (int k = 0; k < np; ++k)
                if (p_cls[k] == cls) { first = k; break; }
            if (first >= 0) {
                const float* pb = mat_box + (mb + first) * 4;
                const float* gb = obj_box + (int64_t)(q0 + lane) * 4;
                const float ov = subgc_grounding_iou(make_float4(pb[0], pb[1], pb[2], pb[3]), make_float4(gb[0], gb[1], gb[2], gb[3]));
                code = ov > iou_thresh ? SUBGC_GRD_HIT : SUBGC_GRD_MISS;
            }
        } else {
            code = SUBGC_GRD_NONE;
        }
        rec[g0 + lane] = code;
    }
    for (int q = g0 + 64 + lane; q < g1; q += 64) rec[q] = SUBGC_GRD_NONE;
}

}  // namespace

SUBGC_API int subgc_grounding_material(const void* tok, int tok64, int T, const uint8_t* bad, int bad_n, int rows, const int32_t* seg,
                                       const int32_t* pick, int I, const int32_t* node, int T1, const int32_t* n_words, const int32_t* tok_class,
                                       int n_tok_class, const int32_t* box_off, const float* boxes, int n_boxes, int32_t* mat_n, int32_t* mat_cls,
                                       int32_t* mat_idx, float* mat_box, int ld_m, void* stream) {
    SUBGC_REQUIRE(rows >= 0 && I >= 0 && n_tok_class >= 0 && n_boxes >= 0 && (!bad || bad_n >= 1),
                  "grounding_material: rows, I, n_tok_class, n_boxes >= 0, bad_n >= 1 with a bad-endings table");
    SUBGC_REQUIRE(T >= 1 && T <= kWords, "grounding_material: token rows need 1 <= T <= %d (got %d)", kWords, T);
    SUBGC_REQUIRE(T1 >= 1, "grounding_material: T1 >= 1 (got %d)", T1);
    SUBGC_REQUIRE(ld_m >= (T < T1 ? T : T1), "grounding_material: ld_m = %d is shorter than min(T, T1) = %d", ld_m, T < T1 ? T : T1);
    if (I == 0) return SUBGC_OK;
    SUBGC_REQUIRE(seg && node && n_words && box_off && mat_n && mat_cls && mat_idx && mat_box && (rows == 0 || tok) && (n_tok_class == 0 || tok_class) &&
                      (n_boxes == 0 || boxes),
                  "grounding_material: null pointer");
    hipStream_t s = (hipStream_t)stream;
    SUBGC_DEBUG_MONO("grounding_material", "seg (row boundaries of the images)", "position", seg, I, rows, s);
    SUBGC_DEBUG_MONO("grounding_material", "box_off (box rows of the images)", "position", box_off, I, n_boxes, s);
    // a pick is image-local; 8192 rows per image is the ranking launch's own limit, so [0, rows) is the check that needs no second table
    SUBGC_DEBUG_RANGE(pick, 4, 1, I, I, 0, rows > 0 ? (int64_t)rows - 1 : 0, -1, "grounding_material: pick (chosen caption of every image)", s);
    SUBGC_DEBUG_RANGE(node, 4, I, T1, T1, 0, n_boxes > 0 ? (int64_t)n_boxes - 1 : 0, -1, "grounding_material: node (box row of every word position)", s);
    hipLaunchKernelGGL(material_kernel, dim3(I), dim3(64), 0, s, tok, tok64, T, bad, bad_n, rows, seg, pick, I, node, T1, n_words, tok_class, n_tok_class,
                       box_off, boxes, n_boxes, mat_n, mat_cls, mat_idx, mat_box, ld_m);
    return subgc::check_launch("subgc_grounding_material");
}

SUBGC_API int subgc_grounding_score(const int32_t* mat_n, const int32_t* mat_cls, const float* mat_box, int ld_m, int I, const int32_t* img_ref,
                                    int n_ref, const int32_t* pair_off, int n_pairs, const int32_t* cap_off, int n_caps, const int32_t* obj_off,
                                    const int32_t* obj_cls, const int32_t* obj_idx, const float* obj_box, int n_obj, const int32_t* ex_off,
                                    const int32_t* ex_lemma, int n_ex, const int32_t* class_lemma, int n_class, float iou_thresh,
                                    const int32_t* prec_off, uint8_t* prec, int n_prec, const int32_t* rec_off, uint8_t* rec, int n_rec,
                                    void* stream) {
    SUBGC_REQUIRE(I >= 0 && n_ref >= 0 && n_pairs >= 0 && n_caps >= 0 && n_obj >= 0 && n_ex >= 0 && n_class >= 0 && n_prec >= 0 && n_rec >= 0,
                  "grounding_score: I, n_ref, n_pairs, n_caps, n_obj, n_ex, n_class, n_prec, n_rec >= 0");
    SUBGC_REQUIRE(ld_m >= 1, "grounding_score: ld_m >= 1 (got %d)", ld_m);
    if (I == 0 || n_pairs == 0) return SUBGC_OK;
    SUBGC_REQUIRE(n_ref >= 1 && n_caps >= 1 && n_class >= 1, "grounding_score: pairs without a reference image, a reference caption or a class");
    SUBGC_REQUIRE(mat_n && mat_cls && mat_box && img_ref && pair_off && cap_off && obj_off && ex_off && class_lemma && prec_off && rec_off &&
                      (n_obj == 0 || (obj_cls && obj_idx && obj_box)) && (n_ex == 0 || ex_lemma) && (n_prec == 0 || prec) && (n_rec == 0 || rec),
                  "grounding_score: null pointer");
    hipStream_t s = (hipStream_t)stream;
    SUBGC_DEBUG_RANGE(img_ref, 4, 1, I, I, 0, (int64_t)n_ref - 1, -1, "grounding_score: img_ref (reference image of every batch image)", s);
    SUBGC_DEBUG_MONO("grounding_score", "pair_off (pairs of the batch images)", "position", pair_off, I, n_pairs, s);
    SUBGC_DEBUG_MONO("grounding_score", "cap_off (CSR caption offsets)", "position", cap_off, n_ref, n_caps, s);
    SUBGC_DEBUG_MONO("grounding_score", "obj_off (CSR object offsets)", "position", obj_off, n_caps, n_obj, s);
    SUBGC_DEBUG_MONO("grounding_score", "ex_off (CSR excluded-lemma offsets)", "position", ex_off, n_caps, n_ex, s);
    SUBGC_DEBUG_MONO("grounding_score", "prec_off (precision event offsets)", "position", prec_off, n_pairs, n_prec, s);
    SUBGC_DEBUG_MONO("grounding_score", "rec_off (recall event offsets)", "position", rec_off, n_pairs, n_rec, s);
    hipLaunchKernelGGL(score_kernel, dim3(n_pairs), dim3(64), 0, s, mat_n, mat_cls, mat_box, ld_m, I, img_ref, n_ref, pair_off, n_pairs, cap_off, n_caps,
                       obj_off, obj_cls, obj_idx, obj_box, n_obj, ex_off, ex_lemma, n_ex, class_lemma, n_class, iou_thresh, prec_off, prec, n_prec,
                       rec_off, rec, n_rec);
    return subgc::check_launch("subgc_grounding_score");
}
