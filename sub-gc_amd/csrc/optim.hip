// The optimizer step over one flat fp32 bucket: the squared gradient norm (subgc_sumsq_f32) and the fused global-norm clip + update
// sweep that consumes it (subgc_clip_optim_step), for every rule misc/utils.py:223-239 (build_optimizer) can construct: Adam, AdamW,
// SGD (plain / momentum / Nesterov), RMSprop, Adagrad.  The sweep reads the clip coefficient from the caller's sum(g^2) accumulator,
// applies grad_scale first, runs as a float4 sweep with a scalar form for unaligned buckets, writes the bf16 weight snapshot in the same
// pass, and has a `_zero` form that leaves the gradient zeroed (optimizer.zero_grad() folded in).  The update rule is a template
// parameter; each follows the single-tensor code path of the torch class build_optimizer constructs, operation by operation.
//
// Parameters torch would SKIP (their .grad is None: the reference's dead GCN units and unused class embeddings) are not touched:
// the caller hands a device table of live [lo, hi) element ranges; every element outside them keeps its weight and its state
// (the `_zero` form still zeroes its gradient).  Without a table (live = NULL: parallel.FlatAdam) every element is swept.  The sweep is
// purely elementwise: no atomics, nothing for deterministic mode to do (the norm's fixed-order form is det_sumsq, det.hip).
#include "common.h"
#include "bf16_util.h"

#include <algorithm>
#include <cmath>

namespace {

inline int ew_grid(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 8192)); }

__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ g, int64_t n, float* __restrict__ out) {
    __shared__ float sm[16];
    float acc = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) acc += g[i] * g[i];
    acc = block_sum(acc, sm);
    if (threadIdx.x == 0) unsafeAtomicAdd(out, acc);
}
// float4 forms (n % 4 == 0, 16-byte aligned buffers: the flat parameter bucket always is): 1 KB per wave instruction
__global__ __launch_bounds__(256) void sumsq_vec_kernel(const float4* __restrict__ g, int64_t n4, float* __restrict__ out) {
    __shared__ float sm[16];
    float acc = 0.f;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i + 3 * stride < n4; i += 4 * stride) {              // four loads in flight per thread: a quarter of the workgroups keeps the bytes in flight
        const float4 x0 = g[i], x1 = g[i + stride], x2 = g[i + 2 * stride], x3 = g[i + 3 * stride];
        acc += x0.x * x0.x + x0.y * x0.y + x0.z * x0.z + x0.w * x0.w;
        acc += x1.x * x1.x + x1.y * x1.y + x1.z * x1.z + x1.w * x1.w;
        acc += x2.x * x2.x + x2.y * x2.y + x2.z * x2.z + x2.w * x2.w;
        acc += x3.x * x3.x + x3.y * x3.y + x3.z * x3.z + x3.w * x3.w;
    }
    for (; i < n4; i += stride) {
        const float4 x = g[i];
        acc += x.x * x.x + x.y * x.y + x.z * x.z + x.w * x.w;
    }
    acc = block_sum(acc, sm);
    if (threadIdx.x == 0) unsafeAtomicAdd(out, acc);
}

struct OptimHyper {
    float lr, a, b, eps, wd;
    float c1, c2;       // ADAM / ADAMW: lr / (1 - beta1^t), sqrt(1 - beta2^t); SGD: 1 - dampening; ADAGRAD: lr / (1 + (t - 1) lr_decay)
    float decay;        // ADAMW: 1 - lr * weight_decay
    int nesterov, first;
};

// one element: p, its state s1 (exp_avg | momentum_buffer | square_avg | sum) and s2 (exp_avg_sq), gi = the scaled, clipped gradient
template <int RULE>
__device__ __forceinline__ void optim_elem(float& p, float gi, float& s1, float& s2, const OptimHyper& h) {
    if constexpr (RULE == SUBGC_OPTIM_ADAM) {                 // torch/optim/adam.py, L2 decay in the gradient.  Every multiply-add is fused
        if (h.wd != 0.f) gi = fmaf(h.wd, p, gi);              // by hand: the bits then do not depend on which products the compiler would
        const float mi = fmaf(1.f - h.a, gi, h.a * s1);       // contract in a given instantiation (scalar / float4, ZERO or not; a
        const float vi = fmaf(gi, (1.f - h.b) * gi, h.b * s2); // near-cancelling g coef + wd p turns an ulp there into 4e-6 of p)
        s1 = mi; s2 = vi;
        const float denom = sqrtf(vi) / h.c2 + h.eps;
        p = fmaf(-h.c1, mi / denom, p);
    } else if constexpr (RULE == SUBGC_OPTIM_ADAMW) {        // adam.py _single_tensor_adam, decoupled_weight_decay: p *= 1 - lr wd first
        if (h.wd != 0.f) p = p * h.decay;
        const float w1 = 1.f - h.a;                           // exp_avg.lerp_(grad, 1 - beta1) (ATen's two-sided lerp)
        s1 = w1 < 0.5f ? s1 + w1 * (gi - s1) : gi - (gi - s1) * (1.f - w1);
        s2 = s2 * h.b + (1.f - h.b) * (gi * gi);              // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
        const float denom = sqrtf(s2) / h.c2 + h.eps;
        p = p + (-h.c1) * (s1 / denom);                       // param.addcdiv_(exp_avg, denom, value=-step_size)
    } else if constexpr (RULE == SUBGC_OPTIM_SGD) {          // sgd.py _single_tensor_sgd
        if (h.wd != 0.f) gi = gi + h.wd * p;
        if (h.a != 0.f) {
            s1 = h.first ? gi : s1 * h.a + h.c1 * gi;         // the first step's buffer IS the gradient (grad.clone())
            gi = h.nesterov ? gi + h.a * s1 : s1;
        }
        p = p + (-h.lr) * gi;
    } else if constexpr (RULE == SUBGC_OPTIM_RMSPROP) {      // rmsprop.py _single_tensor_rmsprop (momentum 0, centered False)
        if (h.wd != 0.f) gi = gi + h.wd * p;
        s1 = s1 * h.a + (1.f - h.a) * (gi * gi);
        const float avg = sqrtf(s1) + h.eps;
        p = p + (-h.lr) * (gi / avg);
    } else {                                                  // adagrad.py _single_tensor_adagrad (dense)
        if (h.wd != 0.f) gi = gi + h.wd * p;
        s1 = s1 + gi * gi;
        const float sd = sqrtf(s1) + h.eps;
        p = p + (-h.c1) * (gi / sd);
    }
}

constexpr bool uses_s2(int rule) { return rule == SUBGC_OPTIM_ADAM || rule == SUBGC_OPTIM_ADAMW; }

// liveness of element e under the sorted bound list live[0..nb) ([lo0, hi0, lo1, hi1, ...]): `r` counts the bounds <= e, `nxt` caches
// live[r]; a thread's elements only increase, so the cursor only moves forward (a handful of steps over the whole sweep)
__device__ __forceinline__ bool live_at(int64_t e, const int64_t* __restrict__ live, int nb, int& r, int64_t& nxt) {
    while (e >= nxt) {
        ++r;
        nxt = r < nb ? live[r] : INT64_MAX;
    }
    return live == nullptr || (r & 1);
}

__device__ __forceinline__ float clip_coef(const float* __restrict__ sumsq, float max_norm, float gscale) {
    // misc/utils.py:193: coef = clip / max(total_norm, clip); gscale (1/world after a SUM all-reduce) is applied first
    return gscale * (max_norm > 0.f ? max_norm / fmaxf(sqrtf(sumsq[0]) * gscale, max_norm) : 1.f);
}

template <int RULE, bool ZERO>
__global__ __launch_bounds__(256) void clip_optim_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ s1,
                                                         float* __restrict__ s2, int64_t n, const int64_t* __restrict__ live, int nb,
                                                         const float* __restrict__ sumsq, float max_norm, float gscale, OptimHyper h,
                                                         uint16_t* __restrict__ p16) {
    const float coef = clip_coef(sumsq, max_norm, gscale);
    const bool st1 = RULE != SUBGC_OPTIM_SGD || h.a != 0.f;
    int r = 0;
    int64_t nxt = nb > 0 ? live[0] : INT64_MAX;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        if (!live_at(i, live, nb, r, nxt)) {
            if (ZERO) g[i] = 0.f;
            continue;
        }
        float gi = g[i] * coef;
        g[i] = ZERO ? 0.f : gi;
        float pi = p[i], a = st1 ? s1[i] : 0.f, b = uses_s2(RULE) ? s2[i] : 0.f;
        optim_elem<RULE>(pi, gi, a, b, h);
        p[i] = pi;
        if (st1) s1[i] = a;
        if (uses_s2(RULE)) s2[i] = b;
        if (p16) p16[i] = (uint16_t)subgc_f2bf(pi);
    }
}

// float4 form (n % 4 == 0, 16-byte aligned buffers: the flat parameter bucket always is).  Live bounds need no alignment: a float4 that
// straddles one updates its live elements only and stores the others back unchanged.
template <int RULE, bool ZERO>
__global__ __launch_bounds__(256) void clip_optim_vec_kernel(float4* __restrict__ p, float4* __restrict__ g, float4* __restrict__ s1,
                                                             float4* __restrict__ s2, int64_t n4, const int64_t* __restrict__ live, int nb,
                                                             const float* __restrict__ sumsq, float max_norm, float gscale, OptimHyper h,
                                                             uint16_t* __restrict__ p16) {
    const float coef = clip_coef(sumsq, max_norm, gscale);
    const bool st1 = RULE != SUBGC_OPTIM_SGD || h.a != 0.f;
    int r = 0;
    int64_t nxt = nb > 0 ? live[0] : INT64_MAX;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        unsigned on = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) on |= (unsigned)live_at(4 * i + e, live, nb, r, nxt) << e;
        if (on == 0) {
            if (ZERO) g[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            continue;
        }
        const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
        float4 P = p[i], G = g[i], A = st1 ? s1[i] : zero4, B = uses_s2(RULE) ? s2[i] : zero4;
        float* pp = &P.x; float* gg = &G.x; float* aa = &A.x; float* bb = &B.x;
#pragma unroll
        for (int e = 0; e < 4; ++e) {                                          // same arithmetic, element by element, as clip_optim_kernel
            if (!((on >> e) & 1u)) {
                if (ZERO) gg[e] = 0.f;
                continue;
            }
            const float gi = gg[e] * coef;
            gg[e] = ZERO ? 0.f : gi;
            optim_elem<RULE>(pp[e], gi, aa[e], bb[e], h);
        }
        g[i] = G; p[i] = P;
        if (st1) s1[i] = A;
        if (uses_s2(RULE)) s2[i] = B;
        if (p16) *reinterpret_cast<uint2*>(p16 + 4 * i) = subgc_pack4(P.x, P.y, P.z, P.w);
    }
}

template <int RULE, bool ZERO>
int launch_rule(float* p, float* g, float* s1, float* s2, int64_t n, const int64_t* live, int nb, const float* sumsq, float max_norm,
                float grad_scale, const OptimHyper& h, uint16_t* p16, hipStream_t stream) {
    auto al = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    if (n % 4 == 0 && al(p) && al(g) && al(s1) && al(s2) && (reinterpret_cast<uintptr_t>(p16) & 7) == 0) {
        hipLaunchKernelGGL((clip_optim_vec_kernel<RULE, ZERO>), dim3(ew_grid(n / 4)), dim3(256), 0, stream, reinterpret_cast<float4*>(p),
                           reinterpret_cast<float4*>(g), reinterpret_cast<float4*>(s1), reinterpret_cast<float4*>(s2), n / 4, live, nb, sumsq,
                           max_norm, grad_scale, h, p16);
    } else {
        hipLaunchKernelGGL((clip_optim_kernel<RULE, ZERO>), dim3(ew_grid(n)), dim3(256), 0, stream, p, g, s1, s2, n, live, nb, sumsq, max_norm,
                           grad_scale, h, p16);
    }
    return subgc::check_launch("subgc_clip_optim_step");
}

template <bool ZERO>
int clip_optim_launch(int rule, float* p, float* g, float* s1, float* s2, int64_t n, const int64_t* live, int n_live, const float* sumsq,
                      float max_norm, float grad_scale, float lr, float h0, float h1, float eps, float weight_decay, int step, int flags,
                      uint16_t* p_bf16, void* stream) {
    SUBGC_REQUIRE(rule >= SUBGC_OPTIM_ADAM && rule <= SUBGC_OPTIM_ADAGRAD, "clip_optim_step: unknown rule %d", rule);
    SUBGC_REQUIRE(n >= 0 && step >= 1 && grad_scale > 0.f && n_live >= 0 && n_live <= (1 << 28), "clip_optim_step: bad arguments");
    SUBGC_REQUIRE(std::isfinite(lr) && lr >= 0.f && eps >= 0.f && weight_decay >= 0.f && max_norm >= 0.f && (flags & ~3) == 0,
                  "clip_optim_step: bad hyperparameters (lr, eps, weight_decay, max_norm >= 0; flags in {0..3})");
    const bool adam = rule == SUBGC_OPTIM_ADAM || rule == SUBGC_OPTIM_ADAMW;
    if (adam) SUBGC_REQUIRE(h0 >= 0.f && h0 < 1.f && h1 >= 0.f && h1 < 1.f, "clip_optim_step: Adam betas must lie in [0, 1)");
    if (rule == SUBGC_OPTIM_SGD) {
        SUBGC_REQUIRE(h0 >= 0.f && std::isfinite(h1), "clip_optim_step: SGD momentum must be >= 0");
        SUBGC_REQUIRE(!(flags & 1) || (h0 > 0.f && h1 == 0.f), "clip_optim_step: Nesterov momentum requires a momentum and zero dampening");
    }
    if (rule == SUBGC_OPTIM_RMSPROP) SUBGC_REQUIRE(h0 >= 0.f && h0 <= 1.f, "clip_optim_step: RMSprop alpha must lie in [0, 1]");
    if (rule == SUBGC_OPTIM_ADAGRAD) SUBGC_REQUIRE(h0 >= 0.f, "clip_optim_step: Adagrad lr_decay must be >= 0");
    SUBGC_REQUIRE((flags & 1) == 0 || rule == SUBGC_OPTIM_SGD, "clip_optim_step: the Nesterov flag is an SGD option");
    if (n == 0) return SUBGC_OK;
    const bool st1 = rule != SUBGC_OPTIM_SGD || h0 != 0.f;
    SUBGC_REQUIRE(p && g && sumsq && (!st1 || s1) && (!adam || s2) && (n_live == 0 || live),
                  "clip_optim_step: null pointer (s1 for every rule but momentum-free SGD, s2 for Adam / AdamW, live when n_live > 0)");
    OptimHyper h{};
    h.lr = lr; h.a = h0; h.b = h1; h.eps = eps; h.wd = weight_decay;
    h.nesterov = flags & 1; h.first = (flags >> 1) & 1;
    if (adam) {                                   // bias corrections, in fp32
        const float bc1 = 1.f - powf(h0, (float)step), bc2 = 1.f - powf(h1, (float)step);
        h.c1 = lr / bc1; h.c2 = sqrtf(bc2);
        h.decay = (float)(1.0 - (double)lr * (double)weight_decay);
    } else if (rule == SUBGC_OPTIM_SGD) {
        h.c1 = (float)(1.0 - (double)h1);
    } else if (rule == SUBGC_OPTIM_ADAGRAD) {
        h.c1 = (float)((double)lr / (1.0 + (double)(step - 1) * (double)h0));
    }
    const int nb = 2 * n_live;
    if (!st1) s1 = nullptr;
    if (!adam) s2 = nullptr;
    hipStream_t s = (hipStream_t)stream;
    switch (rule) {
        case SUBGC_OPTIM_ADAM: return launch_rule<SUBGC_OPTIM_ADAM, ZERO>(p, g, s1, s2, n, live, nb, sumsq, max_norm, grad_scale, h, p_bf16, s);
        case SUBGC_OPTIM_ADAMW: return launch_rule<SUBGC_OPTIM_ADAMW, ZERO>(p, g, s1, s2, n, live, nb, sumsq, max_norm, grad_scale, h, p_bf16, s);
        case SUBGC_OPTIM_SGD: return launch_rule<SUBGC_OPTIM_SGD, ZERO>(p, g, s1, s2, n, live, nb, sumsq, max_norm, grad_scale, h, p_bf16, s);
        case SUBGC_OPTIM_RMSPROP: return launch_rule<SUBGC_OPTIM_RMSPROP, ZERO>(p, g, s1, s2, n, live, nb, sumsq, max_norm, grad_scale, h, p_bf16, s);
        default: return launch_rule<SUBGC_OPTIM_ADAGRAD, ZERO>(p, g, s1, s2, n, live, nb, sumsq, max_norm, grad_scale, h, p_bf16, s);
    }
}

}  // namespace

SUBGC_API int subgc_sumsq_f32(const float* g, int64_t n, float* sumsq, void* stream) {
    SUBGC_REQUIRE(n >= 0, "sumsq: bad size");
    SUBGC_REQUIRE(!subgc::deterministic(), "sumsq: adds with float atomics; in deterministic mode call subgc_sumsq_f32_ws");
    if (n == 0) return SUBGC_OK;
    SUBGC_REQUIRE(g && sumsq, "sumsq: null pointer");
    if (n % 4 == 0 && (reinterpret_cast<uintptr_t>(g) & 15) == 0) {
        // one same-address float atomic per workgroup: 2048 of them queue memory-side for ~20 us (a 13 MB slice took 35 us), 512 do not
        hipLaunchKernelGGL(sumsq_vec_kernel, dim3(std::min(ew_grid(n / 4), 512)), dim3(256), 0, (hipStream_t)stream,
                           reinterpret_cast<const float4*>(g), n / 4, sumsq);
        return subgc::check_launch("subgc_sumsq_f32");
    }
    hipLaunchKernelGGL(sumsq_kernel, dim3(std::min(ew_grid(n), 1024)), dim3(256), 0, (hipStream_t)stream, g, n, sumsq);
    return subgc::check_launch("subgc_sumsq_f32");
}
SUBGC_API int subgc_sumsq_f32_ws(const float* g, int64_t n, float* sumsq, void* workspace, size_t ws_bytes, void* stream) {
    if (!subgc::deterministic()) return subgc_sumsq_f32(g, n, sumsq, stream);
    SUBGC_REQUIRE(n >= 0, "sumsq_ws: bad size");
    if (n == 0) return SUBGC_OK;
    SUBGC_REQUIRE(g && sumsq, "sumsq_ws: null pointer");
    return subgc::det_sumsq(g, n, sumsq, workspace, ws_bytes, (hipStream_t)stream);
}

SUBGC_API int subgc_clip_optim_step(int rule, float* p, float* g, float* s1, float* s2, int64_t n, const int64_t* live, int n_live,
                                    const float* sumsq, float max_norm, float grad_scale, float lr, float h0, float h1, float eps,
                                    float weight_decay, int step, int flags, uint16_t* p_bf16, void* stream) {
    return clip_optim_launch<false>(rule, p, g, s1, s2, n, live, n_live, sumsq, max_norm, grad_scale, lr, h0, h1, eps, weight_decay, step,
                                    flags, p_bf16, stream);
}
SUBGC_API int subgc_clip_optim_step_zero(int rule, float* p, float* g, float* s1, float* s2, int64_t n, const int64_t* live, int n_live,
                                         const float* sumsq, float max_norm, float grad_scale, float lr, float h0, float h1, float eps,
                                         float weight_decay, int step, int flags, uint16_t* p_bf16, void* stream) {
    return clip_optim_launch<true>(rule, p, g, s1, s2, n, live, n_live, sumsq, max_norm, grad_scale, lr, h0, h1, eps, weight_decay, step,
                                   flags, p_bf16, stream);
}
