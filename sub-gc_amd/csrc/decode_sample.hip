// Sampling token choice of one decode step for ANY the_k, with an optional nucleus (top-p) cut: subgc_decode_sample.
// subgc_decode_pick (decoder.hip) keeps its top-k in per-thread arrays and finds them by k dependent workgroup arg-max passes, which
// stops at k = 8.  Here the k leading logits of a row are found by a radix select, sorted in LDS and walked by a fixed-order scan:
//   order     (float32 logit descending, column ascending) -- a total order, written as ONE 48-bit integer per logit:
//             (order-preserving key of the float << 16) | (0xFFFF - column); columns < 16384.  x -> x/temp - lse is monotone, so this
//             is a valid top-k order of the tempered log-probs, and a stable descending sort of the same floats reproduces it exactly.
//   select    the L-th largest composite by an MSB-first radix select: six 8-bit rounds at most, 256-bin LDS histogram (integer LDS
//             adds), the bin that holds rank L found by a block scan over the bins in descending order.  Composites are distinct, so
//             exactly L logits survive; the rounds stop as soon as the whole bin is wanted (no tie straddles the cut: <= 4 rounds).
//   sort      the survivors are compacted into LDS (slot order is arbitrary, the sort removes it) and sorted by a bitonic network.
//   scan      thread t owns the contiguous chunk [t*per, (t+1)*per) of the sorted prefix: chunk sums, an exclusive block scan over
//             the 256 chunk sums, then the running sums inside the chunk -- the same additions in the same order on every launch.
//   nucleus   top_p < 1: only the leading 256 (then x8, ... up to k) are selected and sorted; the level is accepted when the
//             summed mass reaches top_p inside it.  Caption distributions are peaked: the first level almost always decides.
//   whole row k == V, top_p == 1 (plain temperature sampling): the normaliser is the row's whole mass, summed from the registers in a
//             fixed order, so the same escalation applies: a level is accepted when the draw lands inside it.
//   two launches  the dynamic LDS bounds the workgroups per CU, and a 16384-entry prefix (128 KiB) leaves room for one.  An escalating
//             call whose last level exceeds 2048 entries is therefore TWO launches: the first runs the levels up to 2048 with 16 KiB and
//             marks a row it could not decide (next_tok = -1, a vector store like every other result); the second, with the LDS of the
//             last level, returns at once for every decided row and runs the remaining levels for the others.  A level's outcome
//             does not depend on the levels before it, so the result equals the one-launch form bit for bit.
// No float atomics, nothing depends on scheduling: equal inputs give equal bits.  No synchronisation, no allocation: capturable.
#include "common.h"
#include "rowwise.h"

#include <climits>

namespace {

__device__ __forceinline__ uint32_t order_key(float x) {         // a < b  <=>  order_key(a) < order_key(b); -0 counts as +0
    uint32_t b = __float_as_uint(x);
    if (b == 0x80000000u) b = 0u;
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }
__device__ __forceinline__ unsigned long long composite(float x, int c) {
    return ((unsigned long long)order_key(x) << 16) | (unsigned long long)(0xFFFF - c);
}

// One 256-thread workgroup per row; the row (<= 256*PER logits) is loaded into registers once, like decode_pick_kernel<PER>.
// Dynamic LDS: 8 bytes x the power of two >= the longest prefix this launch may sort (see "two launches" above).
template <int PER>
__global__ __launch_bounds__(256) void decode_sample_kernel(const float* __restrict__ logits, int64_t ld, int V, int k, float top_p, float temp,
                                                            const float* __restrict__ u, int t, int64_t* __restrict__ seq,
                                                            float* __restrict__ seqlp, int T, int64_t* __restrict__ next_tok,
                                                            int32_t* __restrict__ unfinished, int32_t* __restrict__ n_unfinished,
                                                            const int32_t* __restrict__ prev_count, int first_level, int last_level,
                                                            int resume) {
    if (prev_count && *prev_count == 0) return;   // the reference has left its loop (AttModel.py:318-319)
    if (resume && next_tok[blockIdx.x] != -1) return;             // second launch: the first one decided this row
    extern __shared__ unsigned long long buf[];   // the sorted prefix
    __shared__ int hist[256];
    __shared__ int smi[8];
    __shared__ float smf[16];
    __shared__ int s_digit, s_krem, s_all, s_cnt, s_first, s_pick;
    __shared__ float s_z;
    const int tid = threadIdx.x, r = blockIdx.x;
    const float* p = logits + (int64_t)r * ld;
    float x[PER];
    row_load<PER>(p, V, x);
    // v = log_softmax(x / temp) = x / temp - lse; the registers keep the raw logits (the radix select orders those).  row_lse with
    // RowTempered spelled out: through the helper this kernel's launches measured 1-3 % slower (profiles/r18_row_refactor_ab.txt)
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < PER; ++j) mx = fmaxf(mx, x[j] / temp);
    mx = block_max(mx, smf);
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < PER; ++j) sum += (tid + j * 256 < V) ? expf(x[j] / temp - mx) : 0.f;
    sum = block_sum(sum, smf);
    const float lse = mx + logf(sum);
    auto mass = [&](unsigned long long e) { return expf(key_value((uint32_t)(e >> 16)) / temp - lse); };

    // plain temperature sampling over the whole row: the kept mass is the row's own (1 up to rounding), known before anything is sorted
    const bool whole = k == V && top_p == 1.f;
    float zrow = 0.f;
    if (whole) {
#pragma unroll
        for (int j = 0; j < PER; ++j) zrow += (tid + j * 256 < V) ? expf(x[j] / temp - lse) : 0.f;
        zrow = block_sum(zrow, smf);
    }
    const float uu = u ? u[r] : 0.f;
    int L = (top_p < 1.f || whole) ? min(k, first_level) : k;        // length of the sorted prefix of this level; every branch below is workgroup-uniform
    int m, lo, hi;
    float base;
    for (;;) {
        // ---- threshold: the L-th largest composite (0: every logit survives)
        unsigned long long thr = 0ull;
        if (L < V) {
            int krem = L;
            for (int rd = 0; rd < 6; ++rd) {
                const int shift = 40 - 8 * rd;
                hist[tid] = 0;
                __syncthreads();
#pragma unroll
                for (int j = 0; j < PER; ++j) {
                    const int c = tid + j * 256;
                    const unsigned long long e = composite(x[j], c);
                    if (c < V && ((e ^ thr) >> (shift + 8)) == 0ull) atomicAdd(&hist[(int)(e >> shift) & 255], 1);
                }
                __syncthreads();
                const int h = hist[255 - tid];                    // bins in descending order
                const int inc = block_scan_incl(h, smi);
                const int exc = inc - h;
                if (exc < krem && krem <= inc) { s_digit = 255 - tid; s_krem = krem - exc; s_all = (krem - exc == h); }
                __syncthreads();
                thr |= (unsigned long long)s_digit << shift;
                krem = s_krem;
                if (s_all) break;                                 // the whole bin is wanted: the undecided low bits stay 0
            }
        }
        // ---- compact the L survivors, pad to a power of two with 0 (below every composite), sort descending
        int P = 1;
        while (P < L) P <<= 1;
        if (tid == 0) { s_cnt = 0; s_first = INT_MAX; s_pick = 0; }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int c = tid + j * 256;
            const unsigned long long e = composite(x[j], c);
            if (c < V && e >= thr) {
                const int slot = atomicAdd(&s_cnt, 1);
                if (slot < P) buf[slot] = e;
            }
        }
        for (int i = L + tid; i < P; i += 256) buf[i] = 0ull;
        for (int size = 2; size <= P; size <<= 1)
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                __syncthreads();
                for (int i = tid; i < (P >> 1); i += 256) {
                    const int a = 2 * i - (i & (stride - 1)), b = a + stride;
                    const unsigned long long ea = buf[a], eb = buf[b];
                    if ((ea < eb) == ((a & size) == 0)) { buf[a] = eb; buf[b] = ea; }
                }
            }
        __syncthreads();
        // ---- c_j = summed exp(v) of the leading j + 1, in a fixed order
        const int per = (L + 255) >> 8;
        lo = min(L, tid * per);
        hi = min(L, lo + per);
        float tot = 0.f;
        for (int j = lo; j < hi; ++j) tot += mass(buf[j]);
        base = block_scan_excl(tot, smf);
        if (whole) {                                              // the draw against the row's mass: decided when it lands inside this level
            int cnt = 0;
            float run = 0.f;
            for (int j = lo; j < hi; ++j) {
                run += mass(buf[j]);
                cnt += uu >= (base + run) / zrow;
            }
            if (cnt) atomicAdd(&s_pick, cnt);
            __syncthreads();
            if (s_pick >= L && L < k) {
                L = (int)min((int64_t)k, (int64_t)L * 8);
                if (L > last_level) { if (tid == 0) next_tok[r] = -1; return; }      // left to the second launch
                __syncthreads();
                continue;
            }
            m = L;
            break;
        }
        if (top_p < 1.f) {                                        // the shortest prefix whose mass reaches top_p
            float run = 0.f;
            for (int j = lo; j < hi; ++j) {
                run += mass(buf[j]);
                if (base + run >= top_p) { atomicMin(&s_first, j); break; }
            }
        }
        __syncthreads();
        const int first = s_first;
        if (first == INT_MAX && L < k) {                          // not reached inside this level: sort a longer prefix
            L = (int)min((int64_t)k, (int64_t)L * 8);
            if (L > last_level) { if (tid == 0) next_tok[r] = -1; return; }          // left to the second launch
            __syncthreads();
            continue;
        }
        m = first == INT_MAX ? L : first + 1;                     // top_p == 1, or the k leading never reach top_p: m = k
        break;
    }
    // ---- renormalise over the m kept, inverse CDF in that order: pick = #{j < m : u >= c_j / c_{m-1}}
    if (!whole) {
        if (lo <= m - 1 && m - 1 < hi) {
            float run = 0.f;
            for (int j = lo; j <= m - 1; ++j) run += mass(buf[j]);
            s_z = base + run;
        }
        __syncthreads();
        const float z = s_z;
        int cnt = 0;
        float run = 0.f;
        for (int j = lo; j < min(hi, m); ++j) {
            run += mass(buf[j]);
            cnt += uu >= (base + run) / z;
        }
        if (cnt) atomicAdd(&s_pick, cnt);
        __syncthreads();
    }
    if (tid == 0) {
        const unsigned long long e = buf[min(s_pick, m - 1)];
        const int it = 0xFFFF - (int)(e & 0xFFFFull);
        const float lp = key_value((uint32_t)(e >> 16)) / temp - lse;    // un-renormalised: the reference gathers from the scattered row
        file_token(r, t, T, t == 0 || unfinished[r], it, lp, seq, seqlp, next_tok, unfinished, n_unfinished);
    }
}

}  // namespace

SUBGC_API int subgc_decode_sample(const float* logits, int64_t ld, int n, int V, int k, float top_p, float temp, const float* u, int t,
                                  int64_t* seq, float* seqlp, int T, int64_t* next_tok, int32_t* unfinished, int32_t* n_unfinished,
                                  const int32_t* prev_count, int raw_logits, void* stream) {
    (void)raw_logits;                             // log_softmax(x / temp) is shift-invariant: normalised and raw rows give the same result
    SUBGC_REQUIRE(n >= 0 && V > 0 && k >= 1 && k <= V && t >= 0 && t < T, "decode_sample: bad sizes");
    SUBGC_REQUIRE(top_p > 0.f && top_p <= 1.f, "decode_sample: top_p must lie in (0, 1]");
    SUBGC_REQUIRE(temp > 0.f, "decode_sample: temperature must be positive");
    SUBGC_REQUIRE(V <= 256 * 64 && ld >= V, "decode_sample: at most %d columns, ld >= V", 256 * 64);
    if (n == 0) return SUBGC_OK;
    SUBGC_REQUIRE(logits && seq && seqlp && next_tok && unfinished, "decode_sample: null pointer");
    int P = 2;
    while (P < k) P <<= 1;
    // levels 256, 2048, 16384 (each capped at k); an escalating call whose last level is beyond kSplit entries runs as two launches
    constexpr int kFirst = 256, kSplit = 2048;
    const bool split = (top_p < 1.f || k == V) && P > kSplit;
    const int per = (V + 255) / 256;
#define LAUNCH(PER_, ENTRIES_, FIRST_, LAST_, RESUME_)                                                                                 \
    do {                                                                                                                               \
        const size_t lds = (size_t)(ENTRIES_) * sizeof(unsigned long long);                                                            \
        if (int rc = subgc::raise_lds_cached((const void*)decode_sample_kernel<PER_>, lds, "decode_sample")) return rc;                \
        hipLaunchKernelGGL(decode_sample_kernel<PER_>, dim3(n), dim3(256), lds, (hipStream_t)stream, logits, ld, V, k, top_p, temp, u, t, seq, \
                           seqlp, T, next_tok, unfinished, n_unfinished, prev_count, FIRST_, LAST_, RESUME_);                          \
    } while (0)
#define LAUNCHES(PER_)                                                                                                                 \
    do {                                                                                                                               \
        if (split) {                                                                                                                   \
            LAUNCH(PER_, kSplit, kFirst, kSplit, 0);                                                                                   \
            LAUNCH(PER_, P, kSplit * 8, INT_MAX, 1);                                                                                   \
        } else {                                                                                                                       \
            LAUNCH(PER_, P, kFirst, INT_MAX, 0);                                                                                       \
        }                                                                                                                              \
    } while (0)
    SUBGC_DISPATCH_PER(per, LAUNCHES);
#undef LAUNCHES
#undef LAUNCH
    return subgc::check_launch("subgc_decode_sample");
}
