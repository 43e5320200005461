// What the kernels that give one workgroup of 256 threads one row of logits agree on, written once: the row in registers, its max /
// sum exp / log-sum-exp, the first arg-max, the fixed-order block scans, the greedy choice and the filing of a chosen token.  Users:
// decoder.hip (log_softmax, decode_pick), criterion.hip (row_lse_sum), decode_sample.hip, selfcritical.hip (sc_pick), forced.hip and
// beam.hip.  Device functions only, all inlined.  NO floating-point contraction pragma here: every file that includes this header
// compiles under the compiler's default and these functions with it.
#pragma once
#include "common.h"
#include "bf16_util.h"

#include <type_traits>

// ---- the PER ladder: a row of V columns sits in PER registers per thread, PER x 256 >= V (callers refuse V > 256 * 64).
// LAUNCH(P) is the caller's launch of its kernel<P>; `per` is (V + 255) / 256.
#define SUBGC_DISPATCH_PER(per, LAUNCH) \
    do {                                \
        if (per <= 4) LAUNCH(4);        \
        else if (per <= 16) LAUNCH(16); \
        else if (per <= 40) LAUNCH(40); \
        else LAUNCH(64);                \
    } while (0)

__device__ __forceinline__ void store_one(void* base, int64_t i, float v, int b16) {
    if (b16) static_cast<uint16_t*>(base)[i] = (uint16_t)subgc_f2bf(v);
    else static_cast<float*>(base)[i] = v;
}

// first arg-max over the workgroup: (value descending, index ascending), a total order; sv, si: >= 4 entries
__device__ __forceinline__ void block_argmax(float& v, int& i, float* sv, int* si) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o, 64);
        const int oi = __shfl_xor(i, o, 64);
        if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { sv[w] = v; si[w] = i; }
    __syncthreads();
    v = sv[0]; i = si[0];
    for (int k = 1; k < nw; ++k)
        if (sv[k] > v || (sv[k] == v && si[k] < i)) { v = sv[k]; i = si[k]; }
}

// scans over the 256 threads in thread order: a fixed tree per wave, then the totals of the waves in front added in wave order and the
// thread's own part (inclusive: its tree value, exclusive: its left neighbour's) added last; sm: >= 4 elements
template <class T>
__device__ __forceinline__ void wave_scan_incl(T& v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
}
template <class T>
__device__ __forceinline__ T waves_in_front(T v, T* sm) {       // v: the thread's inclusive wave scan
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 63) sm[w] = v;
    __syncthreads();
    T base = T(0);
    for (int i = 0; i < w; ++i) base += sm[i];
    return base;
}
template <class T>
__device__ __forceinline__ T block_scan_incl(T v, T* sm) {
    wave_scan_incl(v);
    if constexpr (std::is_integral<T>::value) {
        // integers: the order is free, and adding the wave totals onto v is the loop decode_sample's radix select was timed with (through
        // waves_in_front its launches measured 1-3 % slower, profiles/r18_row_refactor_ab.txt)
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
        __syncthreads();
        if (lane == 63) sm[w] = v;
        __syncthreads();
        for (int i = 0; i < w; ++i) v += sm[i];
        return v;
    } else {
        return waves_in_front(v, sm) + v;
    }
}
template <class T>
__device__ __forceinline__ T block_scan_excl(T v, T* sm) {
    wave_scan_incl(v);
    T exc = __shfl_up(v, 1, 64);
    if ((threadIdx.x & 63) == 0) exc = T(0);
    return waves_in_front(v, sm) + exc;
}

// ---- the row in registers: thread i holds columns i, i + 256, ...; a column past V holds -inf
template <int PER>
__device__ __forceinline__ void row_load(const float* __restrict__ p, int V, float (&x)[PER]) {
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int c = threadIdx.x + j * 256;
        x[j] = c < V ? p[c] : -INFINITY;
    }
}

// how a register becomes the number that is summed: as it is, or divided by the temperature at every use
struct RowPlain {
    __device__ __forceinline__ float operator()(float v) const { return v; }
};
struct RowTempered {
    float temp;
    __device__ __forceinline__ float operator()(float v) const { return v / temp; }
};

// max_c f(x_c), sum_c exp(f(x_c) - mx) and their log-sum-exp over the workgroup; sm: >= 16 floats
template <int PER, class F>
__device__ __forceinline__ float row_max(const float (&x)[PER], float* sm, F f) {
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < PER; ++j) mx = fmaxf(mx, f(x[j]));
    return block_max(mx, sm);
}
template <int PER, class F>
__device__ __forceinline__ float row_sum_exp(const float (&x)[PER], int V, float mx, float* sm, F f) {
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < PER; ++j) sum += (threadIdx.x + j * 256 < V) ? expf(f(x[j]) - mx) : 0.f;
    return block_sum(sum, sm);
}
template <int PER, class F>
__device__ __forceinline__ float row_lse(const float (&x)[PER], int V, float* sm, F f) {
    const float mx = row_max<PER>(x, sm, f);
    return mx + logf(row_sum_exp<PER>(x, V, mx, sm, f));
}

// the greedy choice: the first arg-max of the row and its log-probability -- the value itself on log-softmaxed rows, and on raw logits
// log_softmax(x)[argmax] = -log sum exp(x - max)
template <int PER>
__device__ __forceinline__ void row_greedy(const float (&x)[PER], int V, int raw, float* sv, int* si, float* smf, int& it, float& lp) {
    float bv = -INFINITY; int bi = 0x7fffffff;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int c = threadIdx.x + j * 256;
        if (c < V && (x[j] > bv || bi == 0x7fffffff)) { bv = x[j]; bi = c; }
    }
    block_argmax(bv, bi, sv, si);
    it = bi; lp = bv;
    if (raw) lp = -logf(row_sum_exp<PER>(x, V, bv, smf, RowPlain{}));
}

// Filing the token `it` chosen for row r at step t (AttModel.py:295-316); ONE thread of the row's workgroup calls it.  live: the row was
// unfinished before this step (t == 0 || unfinished[r]).  n_unfinished is a FLAG, not a count: every consumer only tests it against
// zero, and one same-address device atomic per row is what decode_pick once spent its time on (2560 rows x ~15 ns of memory-side
// serialisation = 38 of its 43 us).
__device__ __forceinline__ void file_token(int r, int t, int T, bool live, int it, float lp, int64_t* __restrict__ seq,
                                           float* __restrict__ seqlp, int64_t* __restrict__ next_tok, int32_t* __restrict__ unfinished,
                                           int32_t* __restrict__ n_unfinished) {
    const int unf = live && it > 0;
    unfinished[r] = unf;
    const int64_t w = unf ? it : 0;
    seq[(int64_t)r * T + t] = w;
    seqlp[(int64_t)r * T + t] = lp;
    next_tok[r] = w;
    if (unf && n_unfinished) *n_unfinished = 1;
}
