// Decode rules (include/subgc_decode_rules_hip.h): the log-softmax of a logits row and, on it, block_trigrams, the UNK penalty, the
// repeat ban and the bad-ending ban of one step of the non-beam token loop -- one row pass, in place, in front of the unchanged pick
// kernels.  The row is staged in LDS (one read, one write); its log-sum-exp takes forced_pick_kernel's chunk-then-scan order; the
// history (<= 64 tokens) and the bad-ending list (<= 64 ids) sit in LDS beside it and wave 0 finds the trigram matches, one lane per
// start position.  No atomics: every column and every counter has one writer.
#include "common.h"
#include "rowwise.h"

#include "../../include/subgc_decode_rules_hip.h"

#pragma clang fp contract(off)

namespace {

// a thread's part of the first arg-max of a row: its columns arrive in ascending order, so `>` keeps the first of equal values
struct Best {
    float v = -INFINITY;
    int i = 0x7fffffff;
    __device__ __forceinline__ void see(float x, int c) {
        if (x > v || i == 0x7fffffff) { v = x; i = c; }
    }
};

// One workgroup of 256 per row.  Every branch around a barrier is workgroup-uniform (flags, t, stats, prev_count).
// Dynamic LDS: V floats (the row).
__global__ __launch_bounds__(256) void decode_rules_kernel(float* __restrict__ logits, int64_t ld, int V, const int64_t* __restrict__ seq, int T,
                                                           int t, int flags, float pen, const int32_t* __restrict__ bad_ids, int n_bad,
                                                           int32_t* __restrict__ stats, const int32_t* __restrict__ prev_count) {
    if (prev_count && *prev_count == 0) return;   // no row was unfinished after the previous step (AttModel.py:318-319)
    extern __shared__ float xs[];                 // [V] the row
    __shared__ float smf[16];
    __shared__ float s_z;
    __shared__ float sv[4];
    __shared__ int si[4];
    __shared__ long long s_h[SUBGC_RULES_MAX_T];  // the history, as filed
    __shared__ int s_col[SUBGC_RULES_MAX_T];      // the column a match at start j counts for, else -1
    __shared__ int s_bad[SUBGC_RULES_MAX_BAD];
    __shared__ int s_tri;                         // a trigram penalty was applied
    const int tid = threadIdx.x, r = blockIdx.x;
    float* p = logits + (int64_t)r * ld;
    if (tid < t) s_h[tid] = seq[(int64_t)r * T + tid];
    if (tid < SUBGC_RULES_MAX_T) s_col[tid] = -1;
    if ((flags & SUBGC_RULE_BAD_END) && tid < n_bad) s_bad[tid] = bad_ids[tid];
    if (tid == 0) s_tri = 0;
    float mx = -INFINITY;
    constexpr int U = 8;                          // U loads of a thread are requested before the first is used
    for (int c0 = tid; c0 < V; c0 += 256 * U) {
        float x[U];
#pragma unroll
        for (int u = 0; u < U; ++u) x[u] = c0 + u * 256 < V ? p[c0 + u * 256] : -INFINITY;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (c0 + u * 256 < V) xs[c0 + u * 256] = x[u];
            mx = fmaxf(mx, x[u]);
        }
    }
    mx = block_max(mx, smf);                      // (barriers inside: xs[], s_h[], s_col[] and s_bad[] are complete afterwards)
    const int CH = (V + 255) >> 8;
    const int lo = min(V, tid * CH), hi = min(V, lo + CH);
    float tot = 0.f;
    for (int c = lo; c < hi; ++c) tot += expf(xs[c] - mx);
    const float run = block_scan_incl(tot, smf);
    if (tid == 255) s_z = run;
    // the trigram matches: lane j of wave 0 owns start j
    if ((flags & SUBGC_RULE_TRIGRAMS) && t >= 3 && tid <= t - 3) {
        const long long c = s_h[tid + 2];
        if (s_h[tid] == s_h[t - 2] && s_h[tid + 1] == s_h[t - 1] && c >= 0 && c < V) s_col[tid] = (int)c;
    }
    __syncthreads();                              // s_z, s_col[]; every chunk sum has read xs[]
    const float lz = logf(s_z);
    Best b0;                                      // the first arg-max of the log-softmax row, taken as it is written
    for (int c = tid; c < V; c += 256) {
        const float lp = (xs[c] - mx) - lz;
        xs[c] = lp;
        b0.see(lp, c);
    }
    __syncthreads();
    if (stats) block_argmax(b0.v, b0.i, sv, si);
    // 1. block_trigrams: the first lane of a column counts the column's matches in ascending j and owns its write
    if ((flags & SUBGC_RULE_TRIGRAMS) && t >= 3 && tid <= t - 3) {
        const int col = s_col[tid];
        if (col >= 0) {
            int cnt = 0, first = 1;
            for (int j = 0; j <= t - 3; ++j) {
                if (s_col[j] == col) { ++cnt; if (j < tid) first = 0; }
            }
            if (first) {
                const float add = (float)cnt * pen;
                xs[col] = xs[col] + add;
                s_tri = 1;                        // (every writer stores the same value)
            }
        }
    }
    __syncthreads();
    // 2.-4.: one lane, in the contract's order
    if (tid == 0) {
        int rep = 0, bad = 0;
        if (flags & SUBGC_RULE_UNK) xs[V - 1] = xs[V - 1] - 1000.0f;
        if (t >= 1) {
            const long long last = s_h[t - 1];
            if ((flags & SUBGC_RULE_REPEAT) && last >= 0 && last < V) { xs[(int)last] = -INFINITY; rep = 1; }
            if (flags & SUBGC_RULE_BAD_END) {
                for (int i = 0; i < n_bad; ++i) bad |= (long long)s_bad[i] == last;
                if (bad) xs[0] = -INFINITY;
            }
        }
        if (stats) {
            int32_t* st = stats + (int64_t)r * 4;
            if (s_tri) st[SUBGC_RULE_STAT_TRIGRAM] = st[SUBGC_RULE_STAT_TRIGRAM] + 1;
            if (rep) st[SUBGC_RULE_STAT_REPEAT] = st[SUBGC_RULE_STAT_REPEAT] + 1;
            if (bad) st[SUBGC_RULE_STAT_BAD_END] = st[SUBGC_RULE_STAT_BAD_END] + 1;
        }
    }
    __syncthreads();
    Best b1;                                      // ... and of the ruled row, taken as it leaves
    for (int c = tid; c < V; c += 256) {
        const float v = xs[c];
        p[c] = v;
        b1.see(v, c);
    }
    if (stats) {
        block_argmax(b1.v, b1.i, sv, si);
        if (tid == 0 && b1.i != b0.i) {
            int32_t* st = stats + (int64_t)r * 4;
            st[SUBGC_RULE_STAT_CHANGED] = st[SUBGC_RULE_STAT_CHANGED] + 1;
        }
    }
}

}  // namespace

SUBGC_API int subgc_decode_rules(float* logits, int64_t ld, int n, int V, const int64_t* seq, int T, int t, int flags, float trigram_pen,
                                 const int32_t* bad_ids, int n_bad, int32_t* stats, const int32_t* prev_count, void* stream) {
    SUBGC_REQUIRE(n >= 0, "decode_rules: n >= 0 rows (got n = %d)", n);
    SUBGC_REQUIRE(V <= SUBGC_RULES_MAX_V, "decode_rules: at most %d columns (got V = %d)", SUBGC_RULES_MAX_V, V);
    SUBGC_REQUIRE(V >= SUBGC_RULES_MIN_V, "decode_rules: at least %d columns (got V = %d)", SUBGC_RULES_MIN_V, V);
    SUBGC_REQUIRE(T >= 1 && T <= SUBGC_RULES_MAX_T, "decode_rules: 1 <= T <= %d steps of history (got T = %d)", SUBGC_RULES_MAX_T, T);
    SUBGC_REQUIRE(t >= 0 && t < T, "decode_rules: step t = %d is outside 0 .. T - 1 = %d", t, T - 1);
    SUBGC_REQUIRE(n_bad >= 0 && n_bad <= SUBGC_RULES_MAX_BAD, "decode_rules: 0 <= n_bad <= %d bad-ending ids (got n_bad = %d)",
                  SUBGC_RULES_MAX_BAD, n_bad);
    SUBGC_REQUIRE(ld >= V, "decode_rules: ld >= V (got ld = %lld, V = %d)", (long long)ld, V);
    SUBGC_REQUIRE((flags & ~SUBGC_RULE_ALL) == 0, "decode_rules: unknown flag bits (got flags = %d, known: %d)", flags, SUBGC_RULE_ALL);
    SUBGC_REQUIRE(!(trigram_pen > 0.f) && trigram_pen == trigram_pen, "decode_rules: trigram_pen <= 0 (got %g)", (double)trigram_pen);
    if (n == 0) return SUBGC_OK;
    SUBGC_REQUIRE(logits && seq, "decode_rules: null pointer");
    SUBGC_REQUIRE(!(flags & SUBGC_RULE_BAD_END) || n_bad == 0 || bad_ids, "decode_rules: n_bad = %d ids but bad_ids is null", n_bad);
    hipStream_t s = (hipStream_t)stream;
    if (t > 0) SUBGC_DEBUG_RANGE(seq, 8, n, t, T, 0, (int64_t)V - 1, -1, "decode_rules: seq (the history tokens of the rows)", s);
    const size_t lds = (size_t)V * sizeof(float);
    const size_t lds_static = 2048;               // the kernel's own __shared__ arrays count against the same 64 KiB default
    if (int rc = subgc::raise_lds_cached((const void*)decode_rules_kernel, lds + lds_static, "decode_rules")) return rc;
    hipLaunchKernelGGL(decode_rules_kernel, dim3(n), dim3(256), lds, s, logits, ld, V, seq, T, t, flags, trigram_pen, bad_ids, n_bad, stats,
                       prev_count);
    return subgc::check_launch("subgc_decode_rules");
}
