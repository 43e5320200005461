// Forced decode (include/subgc_forced_hip.h): the token filing of a decode step that FOLLOWS a given token (AttModel.py:295-316 with `it`
// given) and the per-caption log-likelihood after the loop.  forced_pick_kernel files the given token with the pick kernels' file_token
// (rowwise.h) behind its own test for a row that has ended; its log-sum-exp takes the chunk-then-scan order of sc_pick_kernel's sampling
// half (the row staged in LDS, a contiguous chunk per lane, an inclusive scan over the 256 chunk sums), not the strided order of row_lse,
// so its seqlp agrees with the greedy kernels' to rounding and not to the bit.  No atomics: every output has one writer.
#include "common.h"
#include "rowwise.h"

#include "../../include/subgc_forced_hip.h"

namespace {

// One workgroup of 256 per row.  Every branch is workgroup-uniform (live, raw), so the block reductions run on full waves.
// Dynamic LDS: V floats when raw (the row, read once).
__global__ __launch_bounds__(256) void forced_pick_kernel(const float* __restrict__ logits, int64_t ld, int V, const int64_t* __restrict__ forced,
                                                          int64_t ld_f, int t, int64_t* __restrict__ seq, float* __restrict__ seqlp, int T,
                                                          int64_t* __restrict__ next_tok, int32_t* __restrict__ unfinished,
                                                          int32_t* __restrict__ n_unfinished, const int32_t* __restrict__ prev_count, int raw) {
    if (prev_count && *prev_count == 0) return;   // no row was unfinished after the previous step (AttModel.py:318-319)
    extern __shared__ float xs[];                 // [V] the row
    __shared__ float smf[16];
    __shared__ float s_z;
    const int tid = threadIdx.x, r = blockIdx.x;
    const bool live = t == 0 || unfinished[r] != 0;
    __syncthreads();                              // every thread has read unfinished[r] before thread 0 writes it
    const int64_t o = (int64_t)r * T + t;
    if (!live) {
        if (tid == 0) { seq[o] = 0; seqlp[o] = 0.f; next_tok[r] = 0; unfinished[r] = 0; }
        return;
    }
    const int64_t given = forced[(int64_t)r * ld_f + t];
    const int tok = given < 0 ? 0 : (given >= V ? V - 1 : (int)given);
    const float* p = logits + (int64_t)r * ld;
    float lp;
    if (raw) {
        float mx = -INFINITY;
        for (int c = tid; c < V; c += 256) {
            const float x = p[c];
            xs[c] = x;
            mx = fmaxf(mx, x);
        }
        mx = block_max(mx, smf);                  // (barriers inside: xs[] is complete afterwards)
        const int CH = (V + 255) >> 8;
        const int lo = min(V, tid * CH), hi = min(V, lo + CH);
        float tot = 0.f;
        for (int c = lo; c < hi; ++c) tot += expf(xs[c] - mx);
        const float run = block_scan_incl(tot, smf);
        if (tid == 255) s_z = run;
        __syncthreads();
        lp = (xs[tok] - mx) - logf(s_z);
    } else {
        lp = p[tok];
    }
    if (tid == 0) file_token(r, t, T, live, tok, lp, seq, seqlp, next_tok, unfinished, n_unfinished);
}

// one thread per row: the live steps are a prefix (step 0, then as long as the previous token is a word)
__global__ __launch_bounds__(256) void forced_finish_kernel(const int64_t* __restrict__ seq, const float* __restrict__ seqlp, int T, int n, int Tf,
                                                            double* __restrict__ ll, int32_t* __restrict__ n_tok) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const int64_t* s = seq + (int64_t)r * T;
    const float* l = seqlp + (int64_t)r * T;
    double sum = 0.0;
    int cnt = 0;
    for (int t = 0; t < Tf; ++t) {
        if (t > 0 && s[t - 1] <= 0) break;
        sum += (double)l[t];
        ++cnt;
    }
    ll[r] = sum;
    n_tok[r] = cnt;
}

}  // namespace

SUBGC_API int subgc_forced_pick(const float* logits, int64_t ld, int n, int V, const int64_t* forced, int64_t ld_f, int Tf, int t, int64_t* seq,
                                float* seqlp, int T, int64_t* next_tok, int32_t* unfinished, int32_t* n_unfinished, const int32_t* prev_count,
                                int raw_logits, void* stream) {
    SUBGC_REQUIRE(n >= 0 && V > 0, "forced_pick: n >= 0 rows of V > 0 columns (got n = %d, V = %d)", n, V);
    SUBGC_REQUIRE(V <= SUBGC_FORCED_MAX_V && ld >= V, "forced_pick: at most %d columns and ld >= V (got V = %d, ld = %lld)", SUBGC_FORCED_MAX_V, V,
                  (long long)ld);
    SUBGC_REQUIRE(Tf >= 1 && Tf <= SUBGC_FORCED_MAX_T, "forced_pick: 1 <= Tf <= %d forced steps (got %d)", SUBGC_FORCED_MAX_T, Tf);
    SUBGC_REQUIRE(t >= 0 && t < Tf, "forced_pick: step t = %d is outside the forced rows' 0 .. Tf - 1 = %d", t, Tf - 1);
    SUBGC_REQUIRE(ld_f >= Tf && T >= Tf, "forced_pick: ld_f = %lld and T = %d must cover Tf = %d", (long long)ld_f, T, Tf);
    if (n == 0) return SUBGC_OK;
    SUBGC_REQUIRE(logits && forced && seq && seqlp && next_tok && unfinished, "forced_pick: null pointer");
    hipStream_t s = (hipStream_t)stream;
    SUBGC_DEBUG_RANGE(forced + t, 8, n, 1, ld_f, 0, (int64_t)V - 1, -1, "forced_pick: forced (the given word ids of this step)", s);
    const size_t lds = raw_logits ? (size_t)V * sizeof(float) : 0;
    const size_t lds_static = 512;                // the kernel's own __shared__ arrays count against the same 64 KiB default
    if (int rc = subgc::raise_lds_cached((const void*)forced_pick_kernel, lds ? lds + lds_static : 0, "forced_pick")) return rc;
    hipLaunchKernelGGL(forced_pick_kernel, dim3(n), dim3(256), lds, s, logits, ld, V, forced, ld_f, t, seq, seqlp, T, next_tok, unfinished,
                       n_unfinished, prev_count, raw_logits);
    return subgc::check_launch("subgc_forced_pick");
}

SUBGC_API int subgc_forced_finish(const int64_t* seq, const float* seqlp, int T, int n, int Tf, double* ll, int32_t* n_tok, void* stream) {
    SUBGC_REQUIRE(n >= 0 && Tf >= 1 && T >= Tf, "forced_finish: n >= 0 rows, 1 <= Tf <= T (got n = %d, Tf = %d, T = %d)", n, Tf, T);
    SUBGC_REQUIRE(Tf <= SUBGC_FORCED_MAX_T, "forced_finish: 1 <= Tf <= %d forced steps (got %d)", SUBGC_FORCED_MAX_T, Tf);
    if (n == 0) return SUBGC_OK;
    SUBGC_REQUIRE(seq && seqlp && ll && n_tok, "forced_finish: null pointer");
    hipLaunchKernelGGL(forced_finish_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, seq, seqlp, T, n, Tf, ll, n_tok);
    return subgc::check_launch("subgc_forced_finish");
}
