// Label-smoothed language loss (`--label_smoothing`, opts.py:105): LabelSmoothing of misc/utils.py:126-156 in closed form.
// Entry points and arithmetic: include/subgc_criterion_hip.h.  The kernels are the smoothed twins of log_softmax_kernel, nll_fwd_kernel,
// nll_bwd_kernel and nll_logsoftmax_bwd_kernel in decoder.hip (wave64, 256 lanes per row, the row held in registers between its single
// read and the sums); those stay as they are, and with smoothing == 0 the model never comes here.
#include "common.h"
#include "bf16_util.h"

#include "../../include/subgc_criterion_hip.h"

#include <cmath>

namespace {

// the smoothed target distribution of one call: true_dist[c] = c == w ? conf : e, and H = sum_c true_dist[c] log true_dist[c]
struct Smooth { float conf, e, H; };

Smooth make_smooth(double s, int V) {
    const double conf = 1.0 - s, e = V > 1 ? s / (double)(V - 1) : 0.0;
    const double H = (conf > 0.0 ? conf * std::log(conf) : 0.0) + (s > 0.0 ? s * std::log(e) : 0.0);      // 0 log 0 = 0 at both ends
    return Smooth{(float)conf, (float)e, (float)H};
}

__device__ __forceinline__ void store_one(void* base, int64_t i, float v, int b16) {
    if (b16) static_cast<uint16_t*>(base)[i] = (uint16_t)subgc_f2bf(v);
    else static_cast<float*>(base)[i] = v;
}

// one workgroup per row, PER x 256 >= V: lse (raw logits) and the sum of the row's log-probabilities from ONE read
template <int PER>
__global__ __launch_bounds__(256) void row_lse_sum_kernel(const float* __restrict__ x, int64_t ldx, int rows, int V,
                                                          float* __restrict__ lse_out, float* __restrict__ slp_out) {
    __shared__ float sm[16];
    const int r = blockIdx.x;
    const float* p = x + (int64_t)r * ldx;
    float v[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int c = threadIdx.x + j * 256;
        v[j] = c < V ? p[c] : -INFINITY;
    }
    float lse = 0.f;
    if (lse_out) {                                                        // block-uniform: the same steps as log_softmax_kernel
        float mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < PER; ++j) mx = fmaxf(mx, v[j]);
        mx = block_max(mx, sm);
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < PER; ++j) sum += (threadIdx.x + j * 256 < V) ? expf(v[j] - mx) : 0.f;
        sum = block_sum(sum, sm);
        lse = mx + logf(sum);
    }
    float slp = 0.f;
#pragma unroll
    for (int j = 0; j < PER; ++j) slp += (threadIdx.x + j * 256 < V) ? v[j] - lse : 0.f;      // per element: no sum x - V lse
    slp = block_sum(slp, sm);
    if (threadIdx.x == 0) {
        if (lse_out) lse_out[r] = lse;
        slp_out[r] = slp;
    }
}

__global__ __launch_bounds__(1024) void smoothed_nll_fwd_kernel(const float* __restrict__ logp, const int64_t* __restrict__ target,
                                                                int64_t t_stride, const float* __restrict__ mask, int64_t m_stride,
                                                                const float* __restrict__ slp, Smooth sm_, float* __restrict__ loss,
                                                                float* __restrict__ scratch2, int S, int T, int V,
                                                                const float* __restrict__ den_override, const float* __restrict__ lse) {
    __shared__ float sm[16];
    float num = 0.f, den = 0.f;
    for (int q = threadIdx.x; q < S * T; q += blockDim.x) {
        const int s = q / T, t = q % T;
        const float m = mask[(int64_t)s * m_stride + t];
        int64_t w = target[(int64_t)s * t_stride + t];
        w = w < 0 ? 0 : (w >= V ? V - 1 : w);
        const float lpw = logp[(int64_t)q * V + w] - (lse ? lse[q] : 0.f);
        num += (sm_.H - sm_.conf * lpw - sm_.e * (slp[q] - lpw)) * m;
        den += m;
    }
    num = block_sum(num, sm);
    den = block_sum(den, sm);
    if (den_override) {                                // rows this call does not see: the mask-0 tail (nothing) and the reference's zero rows (m H each)
        num += sm_.H * (den_override[0] - den);
        den = den_override[0];
    }
    if (threadIdx.x == 0) { scratch2[0] = num; scratch2[1] = den; loss[0] = num / den; }
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

// fused through the log-softmax: dlogits[r, c] = g (exp(logp[r, c] - lse[r]) - true_dist[r, c]); masked or inactive rows get zeros.
// b16 / lse / vec as in nll_logsoftmax_bwd_kernel: bf16 output for a GEMM-operand-only gradient, raw logits + lse, four columns per lane.
__global__ __launch_bounds__(256) void smoothed_logsoftmax_bwd_kernel(const float* __restrict__ logp, const int64_t* __restrict__ target,
                                                                      int64_t t_stride, const float* __restrict__ mask, int64_t m_stride,
                                                                      const float* __restrict__ scratch2, const float* __restrict__ dloss,
                                                                      Smooth sm_, void* __restrict__ dlogits, int64_t ldo, int T, int V,
                                                                      const int32_t* __restrict__ active, int b16, const float* __restrict__ lse,
                                                                      int vec) {
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
    const float g = dloss[0] * m / scratch2[1];
    const float* lp = logp + (int64_t)r * V;
    const float sub = lse ? lse[r] : 0.f;
    const float conf = sm_.conf, e = sm_.e;
    if (vec) {
        for (int c = threadIdx.x * 4; c < V; c += blockDim.x * 4) {
            const float4 x = *reinterpret_cast<const float4*>(lp + c);
            const int wi = (int)w - c;
            const float o[4] = {g * (expf(x.x - sub) - (wi == 0 ? conf : e)), g * (expf(x.y - sub) - (wi == 1 ? conf : e)),
                                g * (expf(x.z - sub) - (wi == 2 ? conf : e)), g * (expf(x.w - sub) - (wi == 3 ? conf : e))};
            subgc_store_act<4>(dlogits, d + c, o, b16);
        }
        return;
    }
    for (int c = threadIdx.x; c < V; c += blockDim.x) store_one(dlogits, d + c, g * (expf(lp[c] - sub) - (c == (int)w ? conf : e)), b16);
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
    if (per <= 4) hipLaunchKernelGGL(row_lse_sum_kernel<4>, dim3(rows), dim3(256), 0, s, x, ldx, rows, V, lse, slp);
    else if (per <= 16) hipLaunchKernelGGL(row_lse_sum_kernel<16>, dim3(rows), dim3(256), 0, s, x, ldx, rows, V, lse, slp);
    else if (per <= 40) hipLaunchKernelGGL(row_lse_sum_kernel<40>, dim3(rows), dim3(256), 0, s, x, ldx, rows, V, lse, slp);
    else hipLaunchKernelGGL(row_lse_sum_kernel<64>, dim3(rows), dim3(256), 0, s, x, ldx, rows, V, lse, slp);
    return subgc::check_launch("subgc_row_lse_sum_f32");
}

SUBGC_API int subgc_smoothed_nll_fwd(const float* logp, const int64_t* target, int64_t t_stride, const float* mask, int64_t m_stride,
                                     const float* slp, double smoothing, float* loss, float* scratch2, int S, int T, int V,
                                     const float* den_override, const float* lse, void* stream) {
    SUBGC_REQUIRE_SMOOTHING("smoothed_nll_fwd", smoothing, V);
    SUBGC_REQUIRE(S > 0 && T > 0 && V > 0, "smoothed_nll_fwd: bad sizes");
    SUBGC_REQUIRE(logp && target && mask && slp && loss && scratch2, "smoothed_nll_fwd: null pointer");
    SUBGC_DEBUG_RANGE(target, 8, S, T, t_stride, 0, V - 1, -1, "smoothed_nll_fwd: target (word ids)", stream);
    hipLaunchKernelGGL(smoothed_nll_fwd_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, logp, target, t_stride, mask, m_stride, slp,
                       make_smooth(smoothing, V), loss, scratch2, S, T, V, den_override, lse);
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
    hipStream_t s = (hipStream_t)stream;
    subgc::ProfScope prof(SUBGC_FAM_SOFTMAX, s, 4.0 * S * T * (double)V * 2);
    const int vec = V % 4 == 0 && ld_out % 4 == 0 && (reinterpret_cast<uintptr_t>(logp) & 15) == 0 &&
                    (reinterpret_cast<uintptr_t>(dlogits) & (out_bf16 ? 7 : 15)) == 0;
    hipLaunchKernelGGL(smoothed_logsoftmax_bwd_kernel, dim3(S * T), dim3(256), 0, s, logp, target, t_stride, mask, m_stride, scratch2, dloss,
                       make_smooth(smoothing, V), dlogits, ld_out, T, V, active, out_bf16, lse, vec);
    return subgc::check_launch("subgc_smoothed_logsoftmax_bwd");
}
