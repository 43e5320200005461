// The IoU of the grounding evaluators, shared by grounding.hip (subgc_grounding_score) and grounding_gt.hip (subgc_gt_grounding_score) so
// that the two kernels agree bit for bit.  Include it AFTER `#pragma clang fp contract(off)`: every operation is rounded on its own.
#pragma once
#include <hip/hip_runtime.h>

// bbox_overlaps_batch for one predicted box p and one ground-truth box g (bbox_transform.py:194-220), every operation rounded on its own
__device__ __forceinline__ float subgc_grounding_iou(const float4 p, const float4 g) {
    const float gx = (g.z - g.x) + 1.f, gy = (g.w - g.y) + 1.f;
    const float ga = gx * gy;
    const float px = (p.z - p.x) + 1.f, py = (p.w - p.y) + 1.f;
    const float pa = px * py;
    float iw = (fminf(p.z, g.z) - fmaxf(p.x, g.x)) + 1.f;
    iw = iw < 0.f ? 0.f : iw;
    float ih = (fminf(p.w, g.w) - fmaxf(p.y, g.y)) + 1.f;
    ih = ih < 0.f ? 0.f : ih;
    const float inter = iw * ih;
    const float ua = (pa + ga) - inter;
    float ov = __fdiv_rn(inter, ua);
    if (gx == 1.f && gy == 1.f) ov = 0.f;
    if (px == 1.f && py == 1.f) ov = -1.f;
    return ov;
}
