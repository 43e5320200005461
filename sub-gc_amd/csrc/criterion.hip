// Label-smoothed language loss (`--label_smoothing`, opts.py:105): LabelSmoothing of misc/utils.py:126-156 in closed form.
// Entry points and arithmetic: include/subgc_criterion_hip.h.  The loss and its backward through the log-softmax are the criterion
// kernels of criterion_rule.h with SmoothRule; the row pass (lse and the sum of the row's log-probabilities from one read) uses the row
// helpers of rowwise.h.  Only the dense d(logp) of the two-step backward is a kernel of this file's own: every element is written, where
// the plain criterion's (decoder.hip) fills with zeros and writes one element per row.  With smoothing == 0 the model never comes here.
#include "common.h"
#include "bf16_util.h"
#include "criterion_rule.h"

#include "../../include/subgc_criterion_hip.h"

#include <cmath>

namespace {

Smooth make_smooth(double s, int V) {
    const double conf = 1.0 - s, e = V > 1 ? s / (double)(V - 1) : 0.0;
    const double H = (conf > 0.0 ? conf * std::log(conf) : 0.0) + (s > 0.0 ? s * std::log(e) : 0.0);      // 0 log 0 = 0 at both ends
    return Smooth{(float)conf, (float)e, (float)H};
}

// one workgroup per row, PER x 256 >= V: lse (raw logits) and the sum of the row's log-probabilities from ONE read
template <int PER>
__global__ __launch_bounds__(256) void row_lse_sum_kernel(const float* __restrict__ x, int64_t ldx, int rows, int V,
                                                          float* __restrict__ lse_out, float* __restrict__ slp_out) {
    __shared__ float sm[16];
    const int r = blockIdx.x;
    const float* p = x + (int64_t)r * ldx;
    float v[PER];
    row_load<PER>(p, V, v);
    float lse = 0.f;
    if (lse_out) lse = row_lse<PER>(v, V, sm, RowPlain{});                // block-uniform; log_softmax_kernel's lse, bit for bit
    float slp = 0.f;
#pragma unroll
    for (int j = 0; j < PER; ++j) slp += (threadIdx.x + j * 256 < V) ? v[j] - lse : 0.f;      // per element: no sum x - V lse
    slp = block_sum(slp, sm);
    if (threadIdx.x == 0) {
        if (lse_out) lse_out[r] = lse;
        slp_out[r] = slp;
    }
}

// dense d(logp): one workgroup per row, every element written
__global__ __launch_bounds__(256) void smoothed_nll_bwd_kernel(const int64_t* __restrict__ target, int64_t t_stride,
                                                               const float* __restrict__ mask, int64_t m_stride,
                                                               const float* __restrict__ scratch2, const float* __restrict__ dloss, Smooth sm_,
                                                               float* __restrict__ dlogp, int T, int V) {
    const int r = blockIdx.x, s = r / T, t = r % T;
    int64_t w = target[(int64_t)s * t_stride + t];
    w = w < 0 ? 0 : (w >= V ? V - 1 : w);
    const float g = dloss[0] * mask[(int64_t)s * m_stride + t] / scratch2[1];
    float* d = dlogp + (int64_t)r * V;
    for (int c = threadIdx.x; c < V; c += blockDim.x) d[c] = -g * (c == (int)w ? sm_.conf : sm_.e);
}

}  // namespace

// `smoothing` first: the one argument a caller can get wrong without any tensor at hand
#define SUBGC_REQUIRE_SMOOTHING(who, s, V)                                                                              \
    do {                                                                                                                \
        SUBGC_REQUIRE((s) >= 0.0 && (s) <= 1.0, who ": smoothing %g is outside [0, 1]", (double)(s));                   \
        SUBGC_REQUIRE((V) != 1 || (s) == 0.0, who ": smoothing %g needs more than one column", (double)(s));            \
    } while (0)

SUBGC_API int subgc_row_lse_sum_f32(const float* x, int64_t ldx, int rows, int V, float* lse, float* slp, void* stream) {
    SUBGC_REQUIRE(rows >= 0 && V > 0 && ldx >= V, "row_lse_sum: bad sizes");
    if (rows == 0) return SUBGC_OK;
    SUBGC_REQUIRE(x && slp, "row_lse_sum: null pointer");
    SUBGC_REQUIRE(V <= 256 * 64, "row_lse_sum: at most %d columns", 256 * 64);
    hipStream_t s = (hipStream_t)stream;
    subgc::ProfScope prof(SUBGC_FAM_SOFTMAX, s, 4.0 * rows * (double)V);
    const int per = (V + 255) / 256;
#define LAUNCH(P) hipLaunchKernelGGL(row_lse_sum_kernel<P>, dim3(rows), dim3(256), 0, s, x, ldx, rows, V, lse, slp)
    SUBGC_DISPATCH_PER(per, LAUNCH);
#undef LAUNCH
    return subgc::check_launch("subgc_row_lse_sum_f32");
}

SUBGC_API int subgc_smoothed_nll_fwd(const float* logp, const int64_t* target, int64_t t_stride, const float* mask, int64_t m_stride,
                                     const float* slp, double smoothing, float* loss, float* scratch2, int S, int T, int V,
                                     const float* den_override, const float* lse, void* stream) {
    SUBGC_REQUIRE_SMOOTHING("smoothed_nll_fwd", smoothing, V);
    SUBGC_REQUIRE(S > 0 && T > 0 && V > 0, "smoothed_nll_fwd: bad sizes");
    SUBGC_REQUIRE(logp && target && mask && slp && loss && scratch2, "smoothed_nll_fwd: null pointer");
    SUBGC_DEBUG_RANGE(target, 8, S, T, t_stride, 0, V - 1, -1, "smoothed_nll_fwd: target (word ids)", stream);
    hipLaunchKernelGGL((criterion_fwd_kernel<SmoothRule, 1024>), dim3(1), dim3(1024), 0, (hipStream_t)stream, logp, target, t_stride, mask,
                       m_stride, SmoothRule{make_smooth(smoothing, V), slp}, loss, scratch2, S, T, V, den_override, lse);
    return subgc::check_launch("subgc_smoothed_nll_fwd");
}

SUBGC_API int subgc_smoothed_nll_bwd(const int64_t* target, int64_t t_stride, const float* mask, int64_t m_stride, const float* scratch2,
                                     const float* dloss, double smoothing, float* dlogp, int S, int T, int V, void* stream) {
    SUBGC_REQUIRE_SMOOTHING("smoothed_nll_bwd", smoothing, V);
    SUBGC_REQUIRE(S > 0 && T > 0 && V > 0, "smoothed_nll_bwd: bad sizes");
    SUBGC_REQUIRE(target && mask && scratch2 && dloss && dlogp, "smoothed_nll_bwd: null pointer");
    SUBGC_DEBUG_RANGE(target, 8, S, T, t_stride, 0, V - 1, -1, "smoothed_nll_bwd: target (word ids)", stream);
    hipLaunchKernelGGL(smoothed_nll_bwd_kernel, dim3(S * T), dim3(256), 0, (hipStream_t)stream, target, t_stride, mask, m_stride, scratch2,
                       dloss, make_smooth(smoothing, V), dlogp, T, V);
    return subgc::check_launch("subgc_smoothed_nll_bwd");
}

SUBGC_API int subgc_smoothed_logsoftmax_bwd(const float* logp, const int64_t* target, int64_t t_stride, const float* mask, int64_t m_stride,
                                            const float* scratch2, const float* dloss, double smoothing, void* dlogits, int64_t ld_out, int S,
                                            int T, int V, const int32_t* active, int out_bf16, const float* lse, void* stream) {
    SUBGC_REQUIRE_SMOOTHING("smoothed_logsoftmax_bwd", smoothing, V);
    SUBGC_REQUIRE(S > 0 && T > 0 && V > 0 && ld_out >= V, "smoothed_logsoftmax_bwd: bad sizes");
    SUBGC_REQUIRE(logp && target && mask && scratch2 && dloss && dlogits, "smoothed_logsoftmax_bwd: null pointer");
    SUBGC_DEBUG_RANGE(target, 8, S, T, t_stride, 0, V - 1, -1, "smoothed_logsoftmax_bwd: target (word ids)", stream);
    return criterion_logsoftmax_bwd_launch("subgc_smoothed_logsoftmax_bwd", logp, target, t_stride, mask, m_stride,
                                           SmoothRule{make_smooth(smoothing, V), nullptr}, scratch2, dloss, dlogits, ld_out, S, T, V, active,
                                           out_bf16, lse, stream);
}
