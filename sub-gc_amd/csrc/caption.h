// What the metric kernels (consensus, diversity, accuracy, grounding, controllability) agree on, written once: how a token row becomes a
// caption, how its n-grams become 64-bit keys, and the CIDEr / BLEU pieces that more than one family spells.  Device functions only, all
// inlined.  NO floating-point contraction pragma here: accuracy.hip, grounding.hip, controllability.hip and consensus_bleu.hip turn
// contraction off for the whole file and include this header AFTER that pragma, consensus.hip and diversity.hip keep the compiler's
// default -- every file gets these functions under its own setting.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ int64_t tok_at(const void* __restrict__ tok, int tok64, int64_t i) {
    return tok64 ? static_cast<const int64_t*>(tok)[i] : (int64_t)static_cast<const int32_t*>(tok)[i];
}

// One WAVE (all 64 lanes) reads row r of tok [rows, T], T <= 64: -> the caption's length = the ids before the first id <= 0, at most T
// and at most `cap` (negative: no cap), then -- bad != NULL -- minus its trailing words w with bad[w] != 0 unless every word is one
// (misc/utils.py:74-80).  v = the lane's raw id; a 16-bit word is (uint32_t)v & 0xffffu where lane < length.
__device__ __forceinline__ int load_row(const void* __restrict__ tok, int tok64, int T, int64_t r, const uint8_t* __restrict__ bad, int bad_n,
                                        int lane, int64_t& v, int cap = -1) {
    v = lane < T ? (tok64 ? static_cast<const int64_t*>(tok)[r * T + lane] : (int64_t)static_cast<const int32_t*>(tok)[r * T + lane]) : 0;
    const unsigned long long stop = ~__ballot(v > 0);
    int L = stop ? __ffsll((long long)stop) - 1 : 64;
    if (L > T) L = T;
    if (cap >= 0 && cap < L) L = cap;
    if (bad) {
        const unsigned long long good = __ballot(lane < L && !(v > 0 && v < bad_n && bad[(v > 0 && v < bad_n) ? v : 0]));
        if (good) L = 64 - __clzll((long long)good);                        // a caption of nothing but such words stays whole
    }
    return L;
}

// An n-gram of order 1 .. 4 is ONE 64-bit key: word j in bits 63-16j .. 48-16j, missing words zero (0 is never a word inside a
// sentence), so keys of different orders never coincide.  order = 0 .. 3; w[p .. p + order] are 16-bit words.
__device__ __forceinline__ uint64_t ngram_key(const uint32_t* w, int p, int order) {
    uint64_t key = (uint64_t)w[p] << 48;
    if (order >= 1) key |= (uint64_t)w[p + 1] << 32;
    if (order >= 2) key |= (uint64_t)w[p + 2] << 16;
    if (order >= 3) key |= (uint64_t)w[p + 3];
    return key;
}
__device__ __forceinline__ int key_order(uint64_t k) {                     // 0 .. 3 for a 1- .. 4-gram: the last non-zero 16-bit lane
    return (k & 0xffffull) ? 3 : ((k & 0xffff0000ull) ? 2 : ((k & 0xffff00000000ull) ? 1 : 0));
}

// -> how often the key gk[g] occurs in gk[lo .. hi); before = how many of those lie in front of g (0: g is the key's first occurrence)
__device__ __forceinline__ int count_key(const uint64_t* gk, int lo, int hi, int g, int& before) {
    const uint64_t key = gk[g];
    int c = 0;
    before = 0;
    for (int j = lo; j < hi; ++j) {
        const bool same = gk[j] == key;
        c += same;
        before += same && j < g;
    }
    return c;
}

// CIDEr's sim() numerators of one (hypothesis, reference) pair (cider_scorer.py:139-147): one thread walks the reference's cooked list
// rk / rw [base .. base + nb) (sorted keys, tf-idf weights) once -- addresses do not depend on the comparisons, so the loads pipeline -- while a cursor
// advances through the hypothesis's hk / hw [na]; a matching key adds min(w_hyp, w_ref) * w_ref to its order's sum in ascending key order.
__device__ __forceinline__ void cider_walk(const uint64_t* hk, const double* hw, int na, const uint64_t* __restrict__ rk,
                                           const double* __restrict__ rw, int64_t base, int nb, double (&v)[4]) {
    double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0;
    int ia = 0;
    uint64_t ck = na > 0 ? hk[0] : ~0ull;
#pragma unroll 4
    for (int ib = 0; ib < nb; ++ib) {
        const uint64_t key = rk[base + ib];
        const double w = rw[base + ib];
        while (ck < key) {
            ++ia;
            ck = ia < na ? hk[ia] : ~0ull;
        }
        if (ck == key && ia < na) {
            const double term = fmin(hw[ia], w) * w;
            const int o = key_order(key);
            v0 += o == 0 ? term : 0.0;
            v1 += o == 1 ? term : 0.0;
            v2 += o == 2 ? term : 0.0;
            v3 += o == 3 ? term : 0.0;
        }
    }
    v[0] = v0; v[1] = v1; v[2] = v2; v[3] = v3;
}
// ... and their finish (:149-154): each order over the product of the two norms, where neither is zero, times the length factor g
__device__ __forceinline__ void cider_finish(double (&v)[4], const double (&hn)[4], const double (&rn)[4], double g) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (hn[k] != 0.0 && rn[k] != 0.0) v[k] /= hn[k] * rn[k];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] *= g;
}

// What the two consensus methods (consensus.hip: 'cider', consensus_bleu.hip: 'bleu') do around their pair score, for a workgroup of 256
// that every thread enters.  The captions of image i's first k neighbour images, listed in neighbour order (consensus_reranking.py:
// 155-157): caps[0 .. count) = corpus caption indices, at most max_caps of them; pre: k + 1 ints of scratch.  -> count.  A neighbour
// index out of range is clamped (debug bounds mode reports it instead).  The caller synchronises before it reads caps.
__device__ __forceinline__ int neighbour_captions(const int32_t* __restrict__ nn, int nn_ld, int i, int k, const int32_t* __restrict__ cap_off,
                                                  int n_img, int max_caps, int32_t* pre, int32_t* caps, int t) {
    int b0 = 0, bn = 0;
    if (t < k) {
        int img = nn[(int64_t)i * nn_ld + t];
        img = img < 0 ? 0 : (img >= n_img ? n_img - 1 : img);
        b0 = cap_off[img];
        bn = cap_off[img + 1] - b0;
        if (bn < 0) bn = 0;
        pre[t + 1] = bn;
    }
    if (t == 0) pre[0] = 0;
    __syncthreads();
    if (t == 0)
        for (int q = 1; q <= k; ++q) pre[q] += pre[q - 1];
    __syncthreads();
    if (t < k) {
        const int p = pre[t];
        for (int q = 0; q < bn && p + q < max_caps; ++q) caps[p + q] = b0 + q;
    }
    return pre[k] < max_caps ? pre[k] : max_caps;
}
// The pair scores sc[0 .. nc) (all >= 0; sc holds the next power of two) sorted descending in place, then the first min(m, nc) added in
// that order by thread 0, as `b_s_arr.sort(reverse=True); sum(b_s_arr[:m])` does (:168-169) -> the sum (thread 0 only).  Additions
// only: nothing here can contract.
__device__ __forceinline__ double sum_top_desc(double* sc, int nc, int m, int t) {
    int n2 = 1;
    while (n2 < nc) n2 <<= 1;
    for (int j = nc + t; j < n2; j += 256) sc[j] = -1.0;                   // below every score
    __syncthreads();
    for (int size = 2; size <= n2; size <<= 1) {                            // bitonic, descending
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int q = t; q < n2; q += 256) {
                const int p = q ^ stride;
                if (p > q) {
                    const double x = sc[q], y = sc[p];
                    const bool down = (q & size) == 0;
                    if (down ? x < y : x > y) { sc[q] = y; sc[p] = x; }
                }
            }
            __syncthreads();
        }
    }
    double acc = 0.0;
    if (t == 0) {
        const int mm = m < nc ? m : nc;
#pragma unroll 8
        for (int q = 0; q < mm; ++q) acc += sc[q];
    }
    return acc;
}

// BLEU's "closest" reference length (bleu_scorer.py:76-77 `min((abs(l - testlen), l) for l in reflen)[1]`): over len[0 .. n) without
// entry `skip` (negative: none), the length nearest to testlen, the shorter on a tie; 0 without a candidate
__device__ __forceinline__ int closest_len(const int* len, int n, int skip, int testlen) {
    int best_d = 1 << 30, reflen = 0;
    for (int r = 0; r < n; ++r) {
        if (r == skip) continue;
        const int l = len[r], d = l > testlen ? l - testlen : testlen - l;
        if (d < best_d || (d == best_d && l < reflen)) { best_d = d; reflen = l; }
    }
    return reflen;
}
