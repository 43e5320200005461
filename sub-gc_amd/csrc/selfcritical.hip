// Self-critical sequence training: RewardCriterion of misc/utils.py:89-109, the token choice of its rollout (AttModel.py:295-316 plus the
// sample_max = 0 branch of the upstream project) and the reward of a rollout (opts.py:149-152).  Entry points and arithmetic:
// include/subgc_selfcritical_hip.h.  The criterion on the decoder's rows is criterion_rule.h with RewardRule; the greedy half of
// sc_pick_kernel and its token filing are the row helpers of rowwise.h that decode_pick_kernel uses, and its sampling half follows
// multinomial_kernel in sched_sampling.hip (the row staged in LDS, contiguous chunks per lane).
#include "common.h"
#include "bf16_util.h"
#include "criterion_rule.h"

#include "../../include/subgc_metrics_hip.h"
#include "../../include/subgc_selfcritical_hip.h"

#include <cmath>

namespace {

// One workgroup per row, the row (<= 256 * PER logits) loaded into registers once.  Rows below n_sample draw, the others take the arg-max:
// blockIdx.x < n_sample is workgroup-uniform, like every other branch here.  Dynamic LDS: V floats when the launch has sampling rows.
template <int PER>
__global__ __launch_bounds__(256) void sc_pick_kernel(const float* __restrict__ logits, int64_t ld, int n_sample, int V, float temp,
                                                      const float* __restrict__ u, int t, int64_t* __restrict__ seq,
                                                      float* __restrict__ seqlp, int T, int64_t* __restrict__ next_tok,
                                                      int32_t* __restrict__ unfinished, int32_t* __restrict__ n_unfinished,
                                                      const int32_t* __restrict__ prev_count, int raw) {
    if (prev_count && *prev_count == 0) return;   // the reference has left its loop (AttModel.py:318-319)
    extern __shared__ float ex[];                 // [V] exp(x / temp - max) of a sampling row
    __shared__ float sv[16];
    __shared__ int si[16];
    __shared__ float smf[16];
    __shared__ float s_z;
    __shared__ int s_pick;
    const int tid = threadIdx.x, r = blockIdx.x;
    const float* p = logits + (int64_t)r * ld;
    float x[PER];
    row_load<PER>(p, V, x);
    int it; float lp;
    if (r >= n_sample) {
        row_greedy<PER>(x, V, raw, sv, si, smf, it, lp);
    } else {
        const float mx = row_max<PER>(x, smf, RowTempered{temp});
        float sum = 0.f;                          // row_sum_exp spelled out: each term is also staged in LDS for the CDF
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int c = tid + j * 256;
            if (c < V) { const float e = expf(x[j] / temp - mx); ex[c] = e; sum += e; }
        }
        if (tid == 0) s_pick = 0;
        sum = block_sum(sum, smf);                // (barriers inside: ex[] and s_pick are complete afterwards)
        const float lse = mx + logf(sum);
        // the CDF in column order: lane i owns columns [i * CH, (i + 1) * CH)
        const int CH = (V + 255) >> 8;
        const int lo = min(V, tid * CH), hi = min(V, lo + CH);
        float tot = 0.f;
        for (int c = lo; c < hi; ++c) tot += ex[c];
        const float base = block_scan_excl(tot, smf);
        if (tid == 255) s_z = base + tot;         // the mass of the whole row as the scan sums it: cdf_{V-1} = 1
        __syncthreads();
        const float z = s_z, uu = u ? u[r] : 0.f;
        int cnt = 0;
        float run = 0.f;
        for (int c = lo; c < hi; ++c) {
            run += ex[c];
            cnt += uu >= (base + run) / z;
        }
        if (cnt) atomicAdd(&s_pick, cnt);         // integer LDS adds: the order does not matter
        __syncthreads();
        it = min(s_pick, V - 1);
        lp = p[it] / temp - lse;                  // one element read again (the registers cannot be indexed by a run-time column)
    }
    if (tid == 0) file_token(r, t, T, t == 0 || unfinished[r], it, lp, seq, seqlp, next_tok, unfinished, n_unfinished);
}

// one thread per rollout row (2 S of them): the scored row; the sampled half also writes its replay labels and its criterion mask
__global__ __launch_bounds__(256) void sc_prepare_kernel(const int64_t* __restrict__ seq2, int S, int T, int64_t eos_id,
                                                         int64_t* __restrict__ labels, float* __restrict__ mask,
                                                         int64_t* __restrict__ score_rows) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= 2 * S) return;
    const int64_t* src = seq2 + (int64_t)r * T;
    if (score_rows) {
        int64_t* dst = score_rows + (int64_t)r * (T + 1);
        bool ended = false;
        for (int t = 0; t < T; ++t) {
            const int64_t w = src[t];
            if (eos_id > 0) {
                if (ended) dst[t] = 0;
                else if (w == 0) { dst[t] = eos_id; ended = true; }
                else dst[t] = w;
            } else {
                dst[t] = w;
            }
        }
        dst[T] = 0;
    }
    if (r < S) {
        if (labels) {
            int64_t* lab = labels + (int64_t)r * (T + 2);
            lab[0] = 0;
            for (int t = 0; t < T; ++t) lab[t + 1] = src[t];
            lab[T + 1] = 0;
        }
        if (mask) {
            float* m = mask + (int64_t)r * (T + 1);
            m[0] = 1.f;
            for (int t = 1; t < T; ++t) m[t] = src[t - 1] > 0 ? 1.f : 0.f;
            m[T] = 0.f;
        }
    }
}

// one workgroup: scores, rewards and the mean reward; fp64 throughout, the mean summed lane by lane and then over the lanes in order
__global__ __launch_bounds__(256) void sc_reward_kernel(const double* __restrict__ row_d, int ld_d, int S, int T1, double w_cider, double w_bleu,
                                                        float* __restrict__ reward, float* __restrict__ mean_reward,
                                                        double* __restrict__ scores) {
    __shared__ double part[256];
    double acc = 0.0;
    for (int s = threadIdx.x; s < S; s += 256) {
        const double* a = row_d + (int64_t)s * ld_d;
        const double* b = row_d + (int64_t)(S + s) * ld_d;
        const double sa = w_cider * a[SUBGC_ACC_CIDER] + w_bleu * a[SUBGC_ACC_BLEU + 3];
        const double sb = w_cider * b[SUBGC_ACC_CIDER] + w_bleu * b[SUBGC_ACC_BLEU + 3];
        scores[s] = sa;
        scores[S + s] = sb;
        const float rw = (float)(sa - sb);
        for (int t = 0; t < T1; ++t) reward[(int64_t)s * T1 + t] = rw;
        acc += (double)rw;
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double sum = 0.0;
        for (int i = 0; i < 256; ++i) sum += part[i];
        mean_reward[0] = (float)(sum / (double)S);
    }
}

// RewardCriterion.forward on gathered log-probabilities; one workgroup
__global__ __launch_bounds__(256) void reward_nll_fwd_kernel(const float* __restrict__ input, const int64_t* __restrict__ seq,
                                                             const float* __restrict__ reward, const float* __restrict__ gpn,
                                                             float* __restrict__ loss, float* __restrict__ scratch2, int S, int T) {
    __shared__ float sm[16];
    float num = 0.f, den = 0.f;
    for (int q = threadIdx.x; q < S * T; q += blockDim.x) {
        const int s = q / T, t = q % T;
        const float m = (t == 0 || seq[q - 1] > 0) ? 1.f : 0.f;
        const float rw = reward[q];
        float term = -input[q] * rw;
        if (gpn) term += gpn[s] * expf(rw);
        num += term * m;
        den += m;
    }
    num = block_sum(num, sm);
    den = block_sum(den, sm);
    if (threadIdx.x == 0) { scratch2[0] = num; scratch2[1] = den; loss[0] = num / den; }
}

// its backward: one thread per sentence walks the T steps (dinput) and sums exp(reward) m in fp64 (dgpn)
__global__ __launch_bounds__(256) void reward_nll_bwd_kernel(const int64_t* __restrict__ seq, const float* __restrict__ reward,
                                                             const float* __restrict__ gpn, const float* __restrict__ scratch2,
                                                             const float* __restrict__ dloss, float* __restrict__ dinput,
                                                             float* __restrict__ dgpn, int S, int T) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const float den = scratch2[1], dl = dloss[0];
    double acc = 0.0;
    for (int t = 0; t < T; ++t) {
        const int64_t q = (int64_t)s * T + t;
        const float m = (t == 0 || seq[q - 1] > 0) ? 1.f : 0.f;
        const float rw = reward[q];
        dinput[q] = -(dl * (rw * m) / den);
        if (gpn && m != 0.f) acc += exp((double)rw);
    }
    if (gpn && dgpn) dgpn[s] = (float)((double)dl * acc / (double)den);
}

}  // namespace

SUBGC_API int subgc_sc_pick(const float* logits, int64_t ld, int n, int n_sample, int V, float temp, const float* u, int t, int64_t* seq,
                            float* seqlp, int T, int64_t* next_tok, int32_t* unfinished, int32_t* n_unfinished,
                            const int32_t* prev_count, int raw_logits, void* stream) {
    SUBGC_REQUIRE(n >= 0 && V > 0 && t >= 0 && t < T, "sc_pick: bad sizes");
    SUBGC_REQUIRE(n_sample >= 0 && n_sample <= n, "sc_pick: n_sample = %d of n = %d rows; the sampling rows are the first n_sample", n_sample, n);
    SUBGC_REQUIRE(V <= 256 * 64 && ld >= V, "sc_pick: at most %d columns, ld >= V", 256 * 64);
    SUBGC_REQUIRE(n_sample == 0 || temp > 0.f, "sc_pick: temperature must be positive");
    if (n == 0) return SUBGC_OK;
    SUBGC_REQUIRE(logits && seq && seqlp && next_tok && unfinished, "sc_pick: null pointer");
    const size_t lds = n_sample > 0 ? (size_t)V * sizeof(float) : 0;
    const size_t lds_static = 512;                // the kernel's own __shared__ arrays (< 256 bytes) count against the same 64 KiB default
    const int per = (V + 255) / 256;
#define LAUNCH(P)                                                                                                                     \
    do {                                                                                                                              \
        if (int rc = subgc::raise_lds_cached((const void*)sc_pick_kernel<P>, lds ? lds + lds_static : 0, "sc_pick")) return rc;       \
        hipLaunchKernelGGL(sc_pick_kernel<P>, dim3(n), dim3(256), lds, (hipStream_t)stream, logits, ld, n_sample, V, temp, u, t, seq, \
                           seqlp, T, next_tok, unfinished, n_unfinished, prev_count, raw_logits);                                     \
    } while (0)
    SUBGC_DISPATCH_PER(per, LAUNCH);
#undef LAUNCH
    return subgc::check_launch("subgc_sc_pick");
}

SUBGC_API int subgc_sc_prepare(const int64_t* seq2, int S, int T, int V, int64_t eos_id, int64_t* labels, float* mask,
                               int64_t* score_rows, void* stream) {
    SUBGC_REQUIRE(S > 0 && T > 0 && V > 0 && eos_id >= 0, "sc_prepare: bad sizes");
    SUBGC_REQUIRE(seq2, "sc_prepare: null pointer");
    SUBGC_DEBUG_RANGE(seq2, 8, 2 * (int64_t)S, T, T, 0, V - 1, -1, "sc_prepare: seq2 (word ids)", stream);
    hipLaunchKernelGGL(sc_prepare_kernel, dim3((2 * S + 255) / 256), dim3(256), 0, (hipStream_t)stream, seq2, S, T, eos_id, labels, mask,
                       score_rows);
    return subgc::check_launch("subgc_sc_prepare");
}

SUBGC_API int subgc_sc_reward(const double* row_d, int ld_d, int S, int T1, double w_cider, double w_bleu, float* reward,
                              float* mean_reward, double* scores, void* stream) {
    SUBGC_REQUIRE(std::isfinite(w_cider) && std::isfinite(w_bleu), "sc_reward: the reward weights (cider %g, bleu %g) must be finite", w_cider,
                  w_bleu);
    SUBGC_REQUIRE(S > 0 && T1 > 0 && ld_d >= SUBGC_ACC_ROW_F64, "sc_reward: bad sizes");
    SUBGC_REQUIRE(row_d && reward && mean_reward && scores, "sc_reward: null pointer");
    hipLaunchKernelGGL(sc_reward_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, row_d, ld_d, S, T1, w_cider, w_bleu, reward, mean_reward,
                       scores);
    return subgc::check_launch("subgc_sc_reward");
}

SUBGC_API int subgc_reward_nll_fwd(const float* input, const int64_t* seq, const float* reward, const float* gpn_loss, float* loss,
                                   float* scratch2, int S, int T, void* stream) {
    SUBGC_REQUIRE(S > 0 && T > 0, "reward_nll_fwd: bad sizes");
    SUBGC_REQUIRE(input && seq && reward && loss && scratch2, "reward_nll_fwd: null pointer");
    hipLaunchKernelGGL(reward_nll_fwd_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, input, seq, reward, gpn_loss, loss, scratch2, S, T);
    return subgc::check_launch("subgc_reward_nll_fwd");
}

SUBGC_API int subgc_reward_nll_bwd(const int64_t* seq, const float* reward, const float* gpn_loss, const float* scratch2,
                                   const float* dloss, float* dinput, float* dgpn, int S, int T, void* stream) {
    SUBGC_REQUIRE(S > 0 && T > 0, "reward_nll_bwd: bad sizes");
    SUBGC_REQUIRE(seq && reward && scratch2 && dloss && dinput, "reward_nll_bwd: null pointer");
    SUBGC_REQUIRE(!gpn_loss || dgpn, "reward_nll_bwd: gpn_loss given without a place for its gradient");
    hipLaunchKernelGGL(reward_nll_bwd_kernel, dim3((S + 255) / 256), dim3(256), 0, (hipStream_t)stream, seq, reward, gpn_loss, scratch2, dloss,
                       dinput, dgpn, S, T);
    return subgc::check_launch("subgc_reward_nll_bwd");
}

SUBGC_API int subgc_reward_logits_fwd(const float* logp, const int64_t* target, int64_t t_stride, const float* mask, int64_t m_stride,
                                      const float* reward, int64_t r_stride, float* loss, float* scratch2, int S, int T, int V,
                                      const float* den_override, const float* lse, void* stream) {
    SUBGC_REQUIRE(S > 0 && T > 0 && V > 0, "reward_logits_fwd: bad sizes");
    SUBGC_REQUIRE(logp && target && mask && reward && loss && scratch2, "reward_logits_fwd: null pointer");
    SUBGC_DEBUG_RANGE(target, 8, S, T, t_stride, 0, V - 1, -1, "reward_logits_fwd: target (word ids)", stream);
    hipLaunchKernelGGL((criterion_fwd_kernel<RewardRule, 256>), dim3(1), dim3(256), 0, (hipStream_t)stream, logp, target, t_stride, mask,
                       m_stride, RewardRule{reward, r_stride}, loss, scratch2, S, T, V, den_override, lse);
    return subgc::check_launch("subgc_reward_logits_fwd");
}

SUBGC_API int subgc_reward_logsoftmax_bwd(const float* logp, const int64_t* target, int64_t t_stride, const float* mask, int64_t m_stride,
                                          const float* reward, int64_t r_stride, const float* scratch2, const float* dloss, void* dlogits,
                                          int64_t ld_out, int S, int T, int V, const int32_t* active, int out_bf16, const float* lse,
                                          void* stream) {
    SUBGC_REQUIRE(S > 0 && T > 0 && V > 0 && ld_out >= V, "reward_logsoftmax_bwd: bad sizes");
    SUBGC_REQUIRE(logp && target && mask && reward && scratch2 && dloss && dlogits, "reward_logsoftmax_bwd: null pointer");
    SUBGC_DEBUG_RANGE(target, 8, S, T, t_stride, 0, V - 1, -1, "reward_logsoftmax_bwd: target (word ids)", stream);
    return criterion_logsoftmax_bwd_launch("subgc_reward_logsoftmax_bwd", logp, target, t_stride, mask, m_stride, RewardRule{reward, r_stride},
                                           scratch2, dloss, dlogits, ld_out, S, T, V, active, out_bf16, lse, stream);
}
