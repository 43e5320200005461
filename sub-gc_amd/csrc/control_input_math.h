// The arithmetic of the sct loader's box matching (dataloaders/dataloader_test_sct.py:207-228,263), shared by control_input.hip and the
// stand-alone host check (tools/sct_host_check.cpp) so that the two agree bit for bit.  Include it AFTER `#pragma clang fp contract(off)`
// (host: -ffp-contract=off): every operation is rounded on its own.  NOT the grounding evaluators' IoU (grounding_iou.h): the loader's
// formula has no degenerate-box rules and takes the region first.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SUBGC_SCT_HD __host__ __device__ __forceinline__
#else
#define SUBGC_SCT_HD inline
#endif

struct SubgcSctBox { float x1, y1, x2, y2; };

// :263 `boxes * max(w, h) / 592` on an fp32 array: one rounded product, one correctly rounded division
SUBGC_SCT_HD float subgc_sct_div(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(a, b);
#else
    return a / b;
#endif
}
SUBGC_SCT_HD SubgcSctBox subgc_sct_scale(SubgcSctBox d, float w, float h) {
    const float m = w > h ? w : h;                       // python max(w, h): the first of two equals, the same number
    SubgcSctBox o;
    o.x1 = subgc_sct_div(d.x1 * m, 592.f);
    o.y1 = subgc_sct_div(d.y1 * m, 592.f);
    o.x2 = subgc_sct_div(d.x2 * m, 592.f);
    o.y2 = subgc_sct_div(d.y2 * m, 592.f);
    return o;
}

// :207-228 bb_intersection_over_union(region, detection box) as numpy >= 2 evaluates it on two fp32 rows
SUBGC_SCT_HD float subgc_sct_iou(SubgcSctBox a, SubgcSctBox b) {
    const float xA = a.x1 > b.x1 ? a.x1 : b.x1;
    const float yA = a.y1 > b.y1 ? a.y1 : b.y1;
    const float xB = a.x2 < b.x2 ? a.x2 : b.x2;
    const float yB = a.y2 < b.y2 ? a.y2 : b.y2;
    float iw = (xB - xA) + 1.f;
    iw = iw > 0.f ? iw : 0.f;                            // max(0, x): 0 unless x > 0
    float ih = (yB - yA) + 1.f;
    ih = ih > 0.f ? ih : 0.f;
    const float inter = iw * ih;
    const float areaA = ((a.x2 - a.x1) + 1.f) * ((a.y2 - a.y1) + 1.f);
    const float areaB = ((b.x2 - b.x1) + 1.f) * ((b.y2 - b.y1) + 1.f);
    return subgc_sct_div(inter, (areaA + areaB) - inter);
}
