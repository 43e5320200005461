// The input side of the controllability experiment (include/subgc_control_input_hip.h): dataloaders/dataloader_test_sct.py
// `DataLoader.__getitem__` :261-368 -- region boxes -> matched detection boxes -> the sub-graph rows of the `sct` decode.
//   :261-295  a Python triple loop (set x region x detection box) and a threshold / best-match filter  -> sct_match_kernel
//   :314-355  greedy extraction with numpy masks per set                                               -> sct_extract_greedy_kernel
//   :356-368  look-up of the precomputed sub-graph with the same seed set                              -> sct_gt_lookup_kernel
// One wave64 per region set everywhere: a detection box / node per lane, node sets as 64-bit masks (ballot), relations in chunks of
// 64 with a lane each.  Integer work apart from the IoU; no atomics on floats.
#include "common.h"

#include "../../include/subgc_control_input_hip.h"

#pragma clang fp contract(off)
#include "control_input_math.h"

namespace {

constexpr int MAX_CHUNKS = SUBGC_SCT_MAX_REL / 64;

// the image of region set s: the last b with set_off[b] <= s (images without sets are skipped); wave-uniform
__device__ __forceinline__ int image_of(const int64_t* __restrict__ set_off, int B, int s) {
    int lo = 0, hi = B;                                  // invariant: set_off[lo] <= s < set_off[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (set_off[mid] <= s) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ uint64_t below(int n) { return n >= 64 ? ~0ull : ((1ull << n) - 1ull); }

__global__ __launch_bounds__(64) void sct_match_kernel(const float* __restrict__ boxes, const float* __restrict__ img_wh, int B, int n_obj,
                                                       const float* __restrict__ regions, const int64_t* __restrict__ set_off, int R,
                                                       uint64_t* __restrict__ seed_mask, int32_t* __restrict__ match_idx,
                                                       float* __restrict__ match_iou, int32_t* __restrict__ status) {
    const int s = blockIdx.x, lane = threadIdx.x;
    const int b = image_of(set_off, B, s);
    // lane k: detection box k at image scale (:262-263)
    SubgcSctBox det = {0.f, 0.f, 0.f, 0.f};
    if (lane < n_obj) {
        const float4 d = *reinterpret_cast<const float4*>(boxes + ((int64_t)b * n_obj + lane) * 4);
        det = subgc_sct_scale(SubgcSctBox{d.x, d.y, d.z, d.w}, img_wh[2 * b], img_wh[2 * b + 1]);
    }
    const float* reg = regions + (int64_t)s * R * 5;
    // :271 valid rows = the FIRST count_nonzero(flag column) rows; lane j also keeps region j (R <= 64)
    SubgcSctBox mine = {0.f, 0.f, 0.f, 0.f};
    bool flag = false;
    if (lane < R) {
        mine = SubgcSctBox{reg[lane * 5], reg[lane * 5 + 1], reg[lane * 5 + 2], reg[lane * 5 + 3]};
        flag = reg[lane * 5 + 4] != 0.f;
    }
    const int valid = __popcll(__ballot(flag));
    int my_idx = -1;
    float my_iou = 0.f;
    for (int j = 0; j < valid; ++j) {                    // :274-284, wave-uniform trip count
        SubgcSctBox r;
        r.x1 = __shfl(mine.x1, j); r.y1 = __shfl(mine.y1, j); r.x2 = __shfl(mine.x2, j); r.y2 = __shfl(mine.y2, j);
        float v = lane < n_obj ? subgc_sct_iou(r, det) : 0.f;
        v = v > 0.f ? v : 0.f;                           // `this_iou > max_iou` from 0: nothing at or below 0, nothing unordered
        const float mx = wave_max(v);
        const uint64_t at = __ballot(mx > 0.f && v == mx);
        if (lane == j && at) {                           // strict `>`: the first box that reaches the maximum
            my_idx = __ffsll((unsigned long long)at) - 1;
            my_iou = mx;
        }
    }
    // :287-293 the filter
    const bool matched = my_idx >= 0;
    uint64_t keep = __ballot(matched && my_iou >= 0.5f);
    const uint64_t any = __ballot(matched);
    if (keep == 0) {
        const float best = wave_max(matched ? my_iou : 0.f);
        keep = __ballot(matched && my_iou >= best);
    }
    uint64_t seeds = 0;
    for (uint64_t m = keep; m; m &= m - 1) {             // wave-uniform
        const int l = __ffsll((unsigned long long)m) - 1;
        seeds |= 1ull << (__shfl(my_idx, l) & 63);
    }
    if (lane < R) {
        match_idx[(int64_t)s * R + lane] = my_idx;
        match_iou[(int64_t)s * R + lane] = my_iou;
    }
    if (lane == 0) {
        seed_mask[s] = seeds;
        status[s] = any ? SUBGC_SCT_OK : SUBGC_SCT_NO_OVERLAP;
    }
}

// np.argmax of every object_dist row: one wave per row, the first maximum
__global__ __launch_bounds__(64) void sct_class_kernel(const float* __restrict__ dist, int C, int32_t* __restrict__ cls) {
    const int64_t row = blockIdx.x;
    const int lane = threadIdx.x;
    const float* x = dist + row * C;
    float best = -INFINITY;
    int at = 0x7fffffff;
    for (int c = lane; c < C; c += 64) {
        const float v = x[c];
        if (v > best || at == 0x7fffffff) { best = v; at = c; }
    }
    const float mx = wave_max(best);                     // lanes past C hold -inf
    int cand = (at != 0x7fffffff && best == mx) ? at : 0x7fffffff;
#pragma unroll
    for (int o = 32; o; o >>= 1) cand = min(cand, __shfl_xor(cand, o));
    if (lane == 0) cls[row] = cand == 0x7fffffff ? 0 : cand;
}

__global__ __launch_bounds__(64) void sct_extract_greedy_kernel(const int32_t* __restrict__ cls, const int64_t* __restrict__ rel_ind,
                                                                const int64_t* __restrict__ rel_off, int B, int n_obj,
                                                                const int64_t* __restrict__ set_off, const uint64_t* __restrict__ seed_mask,
                                                                const int32_t* __restrict__ status, int obj_num, int rel_num,
                                                                int64_t* __restrict__ obj_ind, float* __restrict__ att_masks,
                                                                float* __restrict__ pool_mtx, int64_t* __restrict__ pred_ind,
                                                                int64_t* __restrict__ nrel_ind) {
    __shared__ unsigned int s_nodes[2];                  // endpoints of the kept relations, as a 64-bit node mask
    __shared__ int s_sel[64];                            // kept node ids in ascending order
    const int s = blockIdx.x, lane = threadIdx.x;
    const int b = image_of(set_off, B, s);
    const bool ok = status[s] == SUBGC_SCT_OK;
    if (lane < 2) s_nodes[lane] = 0u;
    __syncthreads();
    // :316-325 the seeds and every node of a seed's class
    const uint64_t seeds = ok ? (seed_mask[s] & below(n_obj)) : 0ull;
    const int my_cls = lane < n_obj ? cls[(int64_t)b * n_obj + lane] : -1;
    bool in = false;
    for (uint64_t m = seeds; m; m &= m - 1) {
        const int c = __shfl(my_cls, __ffsll((unsigned long long)m) - 1);
        in = in || (lane < n_obj && my_cls == c);
    }
    const uint64_t nodes0 = __ballot(in);
    // :328-336 relations touching those nodes; their endpoints join
    const int64_t k0 = rel_off[b];
    const int nk = ok ? (int)min((int64_t)(rel_num - 1), max((int64_t)0, rel_off[b + 1] - k0)) : 0;
    const int chunks = (nk + 63) >> 6;                   // <= MAX_CHUNKS (rel_num <= SUBGC_SCT_MAX_REL)
    uint64_t kept[MAX_CHUNKS];
#pragma unroll
    for (int ch = 0; ch < MAX_CHUNKS; ++ch) {
        kept[ch] = 0;
        if (ch < chunks) {
            const int r = ch * 64 + lane;
            bool k = false;
            if (r < nk) {
                const int64_t e0 = rel_ind[(k0 + r) * 2], e1 = rel_ind[(k0 + r) * 2 + 1];
                const bool v0 = e0 >= 0 && e0 < n_obj, v1 = e1 >= 0 && e1 < n_obj;
                k = (v0 && ((nodes0 >> e0) & 1)) || (v1 && ((nodes0 >> e1) & 1));
                if (k) {
                    if (v0) atomicOr(&s_nodes[e0 >> 5], 1u << (e0 & 31));
                    if (v1) atomicOr(&s_nodes[e1 >> 5], 1u << (e1 & 31));
                }
            }
            kept[ch] = __ballot(k);
        }
    }
    __syncthreads();
    const uint64_t nodes = nodes0 | ((uint64_t)s_nodes[0] | ((uint64_t)s_nodes[1] << 32));
    const int n_nodes = __popcll(nodes);
    if ((nodes >> lane) & 1) s_sel[__popcll(nodes & below(lane))] = lane;
    __syncthreads();
    // :346-349 whole rows
    for (int i = lane; i < obj_num; i += 64) {
        obj_ind[(int64_t)s * obj_num + i] = i < n_nodes ? s_sel[i] : obj_num - 1;
        att_masks[(int64_t)s * obj_num + i] = i < n_nodes ? 1.f : 0.f;
    }
    if (pool_mtx) {
        float* pm = pool_mtx + (int64_t)s * obj_num * obj_num;
        for (int q = lane; q < obj_num * obj_num; q += 64) {
            const int r = q / obj_num, c = q - r * obj_num;
            pm[q] = (r == c && r < n_nodes) ? 1.f : 0.f;
        }
    }
    // :351-355 kept relation rows ascending, their endpoints renumbered (:340-343) in relation order
    int64_t* pr = pred_ind + (int64_t)s * rel_num;
    int64_t* nr = nrel_ind + (int64_t)s * rel_num * 2;
    int before = 0;
#pragma unroll
    for (int ch = 0; ch < MAX_CHUNKS; ++ch) {
        if (ch < chunks) {
            const int r = ch * 64 + lane;
            if ((kept[ch] >> lane) & 1) {
                const int at = before + __popcll(kept[ch] & below(lane));          // < nk <= rel_num - 1
                const int64_t e0 = rel_ind[(k0 + r) * 2], e1 = rel_ind[(k0 + r) * 2 + 1];
                pr[at] = r;
                // an endpoint outside the nodes (refused on the host, reported by debug bounds mode) reads as the dummy node
                nr[2 * at] = (e0 >= 0 && e0 < n_obj) ? __popcll(nodes & below((int)e0)) : obj_num - 1;
                nr[2 * at + 1] = (e1 >= 0 && e1 < n_obj) ? __popcll(nodes & below((int)e1)) : obj_num - 1;
            }
            before += __popcll(kept[ch]);
        }
    }
    for (int i = before + lane; i < rel_num; i += 64) {
        pr[i] = rel_num - 1;
        nr[2 * i] = obj_num - 1;
        nr[2 * i + 1] = obj_num - 1;
    }
}

__global__ __launch_bounds__(64) void sct_gt_lookup_kernel(const int64_t* __restrict__ gt_seed, const int64_t* __restrict__ gt_seed_off,
                                                           int n_seed, int B, int n_obj, const int64_t* __restrict__ set_off,
                                                           const uint64_t* __restrict__ seed_mask, int32_t* __restrict__ choice,
                                                           int32_t* __restrict__ status) {
    const int s = blockIdx.x, lane = threadIdx.x;
    const int b = image_of(set_off, B, s);
    const int st = status[s];
    const uint64_t want = seed_mask[s];
    int found = -1;
    for (int j = 0; j < SUBGC_SCT_GT_LISTS; ++j) {       // :360-366, the first equal list
        int64_t a = gt_seed_off[b * SUBGC_SCT_GT_LISTS + j], e = gt_seed_off[b * SUBGC_SCT_GT_LISTS + j + 1];
        a = max((int64_t)0, a);
        e = min((int64_t)n_seed, e);
        uint64_t m = 0;
        bool bad = false;
        for (int64_t i = a + lane; i < e; i += 64) {
            const int64_t v = gt_seed[i];
            if (v >= 0 && v < n_obj) m |= 1ull << v; else bad = true;
        }
#pragma unroll
        for (int o = 32; o; o >>= 1) m |= (uint64_t)__shfl_xor((unsigned long long)m, o);
        const bool any_bad = __ballot(bad) != 0;
        if (found < 0 && !any_bad && m == want) found = j;
    }
    if (lane == 0) {
        choice[s] = st == SUBGC_SCT_OK ? found : -1;
        if (st == SUBGC_SCT_OK && found < 0) status[s] = SUBGC_SCT_NO_GT;
    }
}

}  // namespace

SUBGC_API int subgc_sct_match(const float* boxes, const float* img_wh, int B, int n_obj, const float* regions, const int64_t* set_off,
                              int n_sets, int R, uint64_t* seed_mask, int32_t* match_idx, float* match_iou, int32_t* status, void* stream) {
    SUBGC_REQUIRE(n_obj >= 1 && n_obj <= SUBGC_SCT_MAX_OBJ, "sct_match: 1 <= n_obj <= %d detection boxes per image, one lane each (got %d)",
                  SUBGC_SCT_MAX_OBJ, n_obj);
    SUBGC_REQUIRE(R >= 1 && R <= SUBGC_SCT_MAX_REGIONS, "sct_match: 1 <= R <= %d region rows per set (got %d)", SUBGC_SCT_MAX_REGIONS, R);
    SUBGC_REQUIRE(B >= 0 && n_sets >= 0, "sct_match: negative size (B = %d, n_sets = %d)", B, n_sets);
    if (n_sets == 0) return SUBGC_OK;
    SUBGC_REQUIRE(B >= 1, "sct_match: %d region sets without an image", n_sets);
    SUBGC_REQUIRE(boxes && img_wh && regions && set_off && seed_mask && match_idx && match_iou && status, "sct_match: null pointer");
    SUBGC_DEBUG_RANGE(set_off, 8, 1, (int64_t)B + 1, (int64_t)B + 1, 0, n_sets, -1, "sct_match: set_off", stream);
    hipLaunchKernelGGL(sct_match_kernel, dim3(n_sets), dim3(64), 0, (hipStream_t)stream, boxes, img_wh, B, n_obj, regions, set_off, R, seed_mask,
                       match_idx, match_iou, status);
    return subgc::check_launch("subgc_sct_match");
}

SUBGC_API int subgc_sct_extract_greedy(const float* object_dist, int C, const int64_t* rel_ind, const int64_t* rel_off, int B, int n_obj,
                                       const int64_t* set_off, const uint64_t* seed_mask, const int32_t* status, int n_sets, int obj_num,
                                       int rel_num, int32_t* object_cls, int64_t* gpn_obj_ind, float* att_masks, float* gpn_pool_mtx,
                                       int64_t* gpn_pred_ind, int64_t* gpn_nrel_ind, void* stream) {
    SUBGC_REQUIRE(n_obj >= 1 && n_obj <= SUBGC_SCT_MAX_OBJ, "sct_extract_greedy: 1 <= n_obj <= %d nodes per image, one lane each (got %d)",
                  SUBGC_SCT_MAX_OBJ, n_obj);
    SUBGC_REQUIRE(obj_num >= n_obj + 1, "sct_extract_greedy: obj_num = %d leaves no dummy node behind n_obj = %d nodes", obj_num, n_obj);
    SUBGC_REQUIRE(rel_num >= 2 && rel_num <= SUBGC_SCT_MAX_REL, "sct_extract_greedy: 2 <= rel_num <= %d (got %d)", SUBGC_SCT_MAX_REL, rel_num);
    SUBGC_REQUIRE(C >= 1, "sct_extract_greedy: C >= 1 classes (got %d)", C);
    SUBGC_REQUIRE(B >= 0 && n_sets >= 0, "sct_extract_greedy: negative size (B = %d, n_sets = %d)", B, n_sets);
    if (B == 0 && n_sets == 0) return SUBGC_OK;
    SUBGC_REQUIRE(B >= 1, "sct_extract_greedy: %d region sets without an image", n_sets);
    SUBGC_REQUIRE(object_dist && object_cls, "sct_extract_greedy: null pointer");
    hipLaunchKernelGGL(sct_class_kernel, dim3((unsigned)((int64_t)B * n_obj)), dim3(64), 0, (hipStream_t)stream, object_dist, C, object_cls);
    if (int rc = subgc::check_launch("subgc_sct_extract_greedy (classes)")) return rc;
    if (n_sets == 0) return SUBGC_OK;
    SUBGC_REQUIRE(rel_off && set_off && seed_mask && status && gpn_obj_ind && att_masks && gpn_pred_ind && gpn_nrel_ind,
                  "sct_extract_greedy: null pointer");
    SUBGC_DEBUG_RANGE(set_off, 8, 1, (int64_t)B + 1, (int64_t)B + 1, 0, n_sets, -1, "sct_extract_greedy: set_off", stream);
    hipLaunchKernelGGL(sct_extract_greedy_kernel, dim3(n_sets), dim3(64), 0, (hipStream_t)stream, object_cls, rel_ind, rel_off, B, n_obj, set_off,
                       seed_mask, status, obj_num, rel_num, gpn_obj_ind, att_masks, gpn_pool_mtx, gpn_pred_ind, gpn_nrel_ind);
    return subgc::check_launch("subgc_sct_extract_greedy");
}

SUBGC_API int subgc_sct_gt_lookup(const int64_t* gt_seed, const int64_t* gt_seed_off, int n_seed, int B, int n_obj, const int64_t* set_off,
                                  const uint64_t* seed_mask, int n_sets, int32_t* choice, int32_t* status, void* stream) {
    SUBGC_REQUIRE(n_obj >= 1 && n_obj <= SUBGC_SCT_MAX_OBJ, "sct_gt_lookup: 1 <= n_obj <= %d nodes per image (got %d)", SUBGC_SCT_MAX_OBJ, n_obj);
    SUBGC_REQUIRE(B >= 0 && n_sets >= 0 && n_seed >= 0, "sct_gt_lookup: negative size (B = %d, n_sets = %d, n_seed = %d)", B, n_sets, n_seed);
    if (n_sets == 0) return SUBGC_OK;
    SUBGC_REQUIRE(B >= 1, "sct_gt_lookup: %d region sets without an image", n_sets);
    SUBGC_REQUIRE(gt_seed_off && set_off && seed_mask && choice && status && (gt_seed || n_seed == 0), "sct_gt_lookup: null pointer");
    SUBGC_DEBUG_RANGE(set_off, 8, 1, (int64_t)B + 1, (int64_t)B + 1, 0, n_sets, -1, "sct_gt_lookup: set_off", stream);
    hipLaunchKernelGGL(sct_gt_lookup_kernel, dim3(n_sets), dim3(64), 0, (hipStream_t)stream, gt_seed, gt_seed_off, n_seed, B, n_obj, set_off,
                       seed_mask, choice, status);
    return subgc::check_launch("subgc_sct_gt_lookup");
}
