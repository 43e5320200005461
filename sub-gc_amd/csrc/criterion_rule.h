// The criterion fused on the decoder's rows, written once: loss = sum_q term(q) / den forward, and backward through the log-softmax
// dlogits[r, c] = g_r (exp(logp[r, c] - lse[r]) - true_dist[r, c]).  A RULE, fixed at compile time, supplies what the three criteria
// differ in -- a run-time "smoothing = 0, reward = 1" form would change the instruction sequences and the bits of the sums:
//   NllRule       decoder.hip       LanguageModelCriterion   weight m           true_dist 1 / 0      term -lp m
//   SmoothRule    criterion.hip     LabelSmoothing           weight m           true_dist conf / e   term (H - conf lp - e (slp - lp)) m
//   RewardRule    selfcritical.hip  RewardCriterion          weight reward m    true_dist 1 / 0      term -lp reward m
// Each entry point stays in its own file and instantiates the two kernels with its rule.  No floating-point contraction pragma here.
#pragma once
#include "rowwise.h"

namespace {

struct NllRule {
    __device__ __forceinline__ float weight(float m, int s, int t) const { return m; }
    __device__ __forceinline__ float hit() const { return 1.f; }
    __device__ __forceinline__ float miss() const { return 0.f; }
    __device__ __forceinline__ float term(float lpw, float m, int q, int s, int t) const { return -(lpw) * m; }
    __device__ __forceinline__ void unseen(float& num, float den_all, float den_seen) const {}
};

// the smoothed target distribution of one call: true_dist[c] = c == w ? conf : e, and H = sum_c true_dist[c] log true_dist[c]
struct Smooth { float conf, e, H; };
struct SmoothRule {
    Smooth sm_;
    const float* __restrict__ slp;                      // [S * T] the sum of the row's log-probabilities (row_lse_sum); forward only
    __device__ __forceinline__ float weight(float m, int s, int t) const { return m; }
    __device__ __forceinline__ float hit() const { return sm_.conf; }
    __device__ __forceinline__ float miss() const { return sm_.e; }
    __device__ __forceinline__ float term(float lpw, float m, int q, int s, int t) const {
        return (sm_.H - sm_.conf * lpw - sm_.e * (slp[q] - lpw)) * m;
    }
    // rows this call does not see: the mask-0 tail (nothing) and the reference's zero rows (m H each)
    __device__ __forceinline__ void unseen(float& num, float den_all, float den_seen) const { num += sm_.H * (den_all - den_seen); }
};

struct RewardRule {
    const float* __restrict__ reward;                   // [S, T] view
    int64_t r_stride;
    __device__ __forceinline__ float weight(float m, int s, int t) const { return reward[(int64_t)s * r_stride + t] * m; }
    __device__ __forceinline__ float hit() const { return 1.f; }
    __device__ __forceinline__ float miss() const { return 0.f; }
    __device__ __forceinline__ float term(float lpw, float m, int q, int s, int t) const {
        return -(lpw) * reward[(int64_t)s * r_stride + t] * m;
    }
    __device__ __forceinline__ void unseen(float& num, float den_all, float den_seen) const {}
};

// forward, one workgroup of WIDTH threads (the width fixes the order in which block_sum adds).  lse != NULL: `logp` holds RAW logits
// and lse[q] their row log-sum-exp.  den_override: the criterion's denominator over rows this call does not see (packed decoder).
template <class Rule, int WIDTH>
__global__ __launch_bounds__(WIDTH) void criterion_fwd_kernel(const float* __restrict__ logp, const int64_t* __restrict__ target,
                                                              int64_t t_stride, const float* __restrict__ mask, int64_t m_stride, Rule rule,
                                                              float* __restrict__ loss, float* __restrict__ scratch2, int S, int T, int V,
                                                              const float* __restrict__ den_override, const float* __restrict__ lse) {
    __shared__ float sm[16];
    float num = 0.f, den = 0.f;
    for (int q = threadIdx.x; q < S * T; q += blockDim.x) {
        const int s = q / T, t = q % T;
        const float m = mask[(int64_t)s * m_stride + t];
        int64_t w = target[(int64_t)s * t_stride + t];
        w = w < 0 ? 0 : (w >= V ? V - 1 : w);
        const float lpw = logp[(int64_t)q * V + w] - (lse ? lse[q] : 0.f);
        num += rule.term(lpw, m, q, s, t);
        den += m;
    }
    num = block_sum(num, sm);
    den = block_sum(den, sm);
    if (den_override) {
        rule.unseen(num, den_override[0], den);
        den = den_override[0];
    }
    if (threadIdx.x == 0) { scratch2[0] = num; scratch2[1] = den; loss[0] = num / den; }
}

// backward, one workgroup per row; rows that are masked or inactive get zeros.
// b16: d(logits) is a GEMM operand only (weight gradient and d(hidden)): written bf16, half the bytes of the largest tensor
// lse != NULL: `logp` holds RAW logits and lse[r] their row log-sum-exp (subgc_row_lse_f32): exp(x - lse) is the same number
// vec: V % 4 == 0 and 16-byte aligned rows on both sides -> four columns per lane (16-byte loads, 8/16-byte stores)
template <class Rule>
__global__ __launch_bounds__(256) void criterion_logsoftmax_bwd_kernel(const float* __restrict__ logp, const int64_t* __restrict__ target,
                                                                       int64_t t_stride, const float* __restrict__ mask, int64_t m_stride,
                                                                       Rule rule, const float* __restrict__ scratch2,
                                                                       const float* __restrict__ dloss, void* __restrict__ dlogits, int64_t ldo,
                                                                       int T, int V, const int32_t* __restrict__ active, int b16,
                                                                       const float* __restrict__ lse, int vec) {
    const int r = blockIdx.x, s = r / T, t = r % T;
    const float m = mask[(int64_t)s * m_stride + t];
    const int64_t d = (int64_t)r * ldo;
    if (m == 0.f || (active && !active[r])) {
        if (vec) { const float z[4] = {0.f, 0.f, 0.f, 0.f}; for (int c = threadIdx.x * 4; c < V; c += blockDim.x * 4) subgc_store_act<4>(dlogits, d + c, z, b16); }
        else for (int c = threadIdx.x; c < V; c += blockDim.x) store_one(dlogits, d + c, 0.f, b16);
        return;
    }
    int64_t w = target[(int64_t)s * t_stride + t];
    w = w < 0 ? 0 : (w >= V ? V - 1 : w);
    const float g = dloss[0] * rule.weight(m, s, t) / scratch2[1];
    const float* lp = logp + (int64_t)r * V;
    const float sub = lse ? lse[r] : 0.f;
    const float hit = rule.hit(), miss = rule.miss();
    if (vec) {
        for (int c = threadIdx.x * 4; c < V; c += blockDim.x * 4) {
            const float4 x = *reinterpret_cast<const float4*>(lp + c);
            const int wi = (int)w - c;
            const float o[4] = {g * (expf(x.x - sub) - (wi == 0 ? hit : miss)), g * (expf(x.y - sub) - (wi == 1 ? hit : miss)),
                                g * (expf(x.z - sub) - (wi == 2 ? hit : miss)), g * (expf(x.w - sub) - (wi == 3 ? hit : miss))};
            subgc_store_act<4>(dlogits, d + c, o, b16);
        }
        return;
    }
    for (int c = threadIdx.x; c < V; c += blockDim.x) store_one(dlogits, d + c, g * (expf(lp[c] - sub) - (c == (int)w ? hit : miss)), b16);
}

// the launch of the backward for an entry point that has checked its arguments; `who` is its name in a launch error
template <class Rule>
int criterion_logsoftmax_bwd_launch(const char* who, const float* logp, const int64_t* target, int64_t t_stride, const float* mask,
                                    int64_t m_stride, Rule rule, const float* scratch2, const float* dloss, void* dlogits, int64_t ld_out, int S,
                                    int T, int V, const int32_t* active, int out_bf16, const float* lse, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    subgc::ProfScope prof(SUBGC_FAM_SOFTMAX, s, 4.0 * S * T * (double)V * 2);
    const int vec = V % 4 == 0 && ld_out % 4 == 0 && (reinterpret_cast<uintptr_t>(logp) & 15) == 0 &&
                    (reinterpret_cast<uintptr_t>(dlogits) & (out_bf16 ? 7 : 15)) == 0;
    hipLaunchKernelGGL(criterion_logsoftmax_bwd_kernel<Rule>, dim3(S * T), dim3(256), 0, s, logp, target, t_stride, mask, m_stride, rule,
                       scratch2, dloss, dlogits, ld_out, T, V, active, out_bf16, lse, vec);
    return subgc::check_launch(who);
}

}  // namespace
