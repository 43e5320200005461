// Consensus re-ranking, method 'bleu' (include/subgc_consensus_hip.h; misc/consensus_reranking/concensus_reranking_utils/
// consensus_reranking.py:152-169 with calculate_bleu_sentence, bleu_score_util.py:15-61, as the pair score): every candidate caption of
// every image against the captions of the image's k nearest training images by the m-RNN sentence-level n-gram F-score, the m largest
// pair scores summed.  The id map, the 64-bit n-gram keys, the caption rule, the neighbour lists and the descending sum are those of
// consensus.hip (caption.h); the order of the sums is subgc_consensus_rank.  Counts are integers and matching is exact key comparison;
// the only floating point is the F-score of <= 4 orders per pair and the sums, fp64, in the reference's operation order with FMA
// contraction off for the whole file -- a fused `a * b + c` skips the product's rounding -- and IEEE division (the build has no
// fast-math flag: `/` on doubles is the correctly rounded v_div_scale / v_div_fmas / v_div_fixup sequence).  No atomics on floats.
#include "common.h"

#include <cmath>

#include "../../include/subgc_consensus_hip.h"

#pragma clang fp contract(off)

#include "caption.h"      // after the pragma: its functions are compiled without contraction here

namespace {

constexpr int kMaxCaps = 2048;      // neighbour captions per image
constexpr int kMaxK = 256;          // neighbour images per image
constexpr int kRowWords = 64;       // words of a candidate row (the decode's T)
constexpr int kMaxWords = 256;      // words of a corpus caption

// One wave per sentence: the <= 4 L n-gram keys, each DISTINCT key once with its count, in ascending key order (rank by counting, as
// consensus.hip's cook_kernel) -- `Counter(ngrams(sentence, o))` of bleu_score_util.py:33-34 for o = 1 .. 4 in one list.  Sentence s:
// CSR mode (woff != NULL) words tok[woff[s] .. woff[s+1]), all non-zero; row mode: row s of tok [S, T] by caption.h's load_row, capped
// at row_len[s] words.  Its list lands at keys / counts [4 * first word index ...].
template <int MAXW>
__global__ __launch_bounds__(64) void bleu_cook_kernel(const void* __restrict__ tok, int tok64, const int32_t* __restrict__ woff, int T,
                                                       const int32_t* __restrict__ row_len, const uint8_t* __restrict__ bad, int bad_n,
                                                       uint64_t* __restrict__ keys, int32_t* __restrict__ counts, int32_t* __restrict__ cnt,
                                                       int32_t* __restrict__ wlen) {
    constexpr int MAXK = 4 * MAXW;
    __shared__ uint32_t tk[MAXW];
    __shared__ uint64_t gk[MAXK];
    __shared__ int32_t tf[MAXK];                                           // > 0: first occurrence of its key, the key's count; 0: a repeat
    const int s = blockIdx.x, lane = threadIdx.x;
    const int32_t* t32 = static_cast<const int32_t*>(tok);
    const int64_t* t64 = static_cast<const int64_t*>(tok);
    int64_t start;
    int L;
    if (woff) {
        start = woff[s];
        L = woff[s + 1] - woff[s];
        L = L < 0 ? 0 : (L > MAXW ? MAXW : L);
        for (int p = lane; p < L; p += 64) tk[p] = (uint32_t)(tok64 ? t64[start + p] : (int64_t)t32[start + p]) & 0xffffu;
    } else {                                                                // T <= 64 (checked by the entry point): one word per lane
        start = (int64_t)s * T;
        int64_t v;
        L = load_row(tok, tok64, T, s, bad, bad_n, lane, v, row_len ? row_len[s] : -1);
        if (lane < L) tk[lane] = (uint32_t)v & 0xffffu;
    }
    __syncthreads();
    int nk = 0;
    for (int o = 0; o < 4; ++o) {
        const int c = L - o;
        if (c <= 0) break;
        for (int p = lane; p < c; p += 64) gk[nk + p] = ngram_key(tk, p, o);
        nk += c;
    }
    __syncthreads();
    for (int i = lane; i < nk; i += 64) {
        int before;
        const int eq = count_key(gk, 0, nk, i, before);
        tf[i] = before == 0 ? eq : 0;
    }
    __syncthreads();
    const int64_t base = 4 * start;                                         // nk <= 4 L: the list stays inside the sentence's 4 L slots
    int mine = 0;
    for (int i = lane; i < nk; i += 64) {
        const int f = tf[i];
        if (f == 0) continue;
        const uint64_t ki = gk[i];
        int u = 0;
        for (int j = 0; j < nk; ++j) u += tf[j] > 0 && gk[j] < ki;          // distinct keys below this one: its place
        keys[base + u] = ki;
        counts[base + u] = f;
        ++mine;
    }
    for (int d = 32; d > 0; d >>= 1) mine += __shfl_xor(mine, d);           // an integer count, all 64 lanes
    if (lane == 0) {
        cnt[s] = mine;
        wlen[s] = L;
    }
}

// The clipped matches of one (candidate, caption) pair, all four orders in one merge walk: the thread reads the caption's list
// rk / rc [base .. base + nb) once while a cursor advances through the candidate's hk / hc [na] in LDS; a key both hold adds
// min(count_t, count_r) to its order's sum (bleu_score_util.py:36-41: `min(count, ref_counts[ngram])` over the candidate's n-grams).
__device__ __forceinline__ void bleu_walk(const uint64_t* hk, const int32_t* hc, int na, const uint64_t* __restrict__ rk,
                                          const int32_t* __restrict__ rc, int64_t base, int nb, int (&acc)[4]) {
    int a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    int ia = 0;
    uint64_t ck = na > 0 ? hk[0] : ~0ull;
#pragma unroll 4
    for (int ib = 0; ib < nb; ++ib) {
        const uint64_t key = rk[base + ib];
        const int c = rc[base + ib];
        while (ck < key) {
            ++ia;
            ck = ia < na ? hk[ia] : ~0ull;
        }
        if (ck == key && ia < na) {
            const int h = hc[ia];
            const int term = h < c ? h : c;
            const int o = key_order(key);
            a0 += o == 0 ? term : 0;
            a1 += o == 1 ? term : 0;
            a2 += o == 2 ? term : 0;
            a3 += o == 3 ? term : 0;
        }
    }
    acc[0] = a0; acc[1] = a1; acc[2] = a2; acc[3] = a3;
}

// bleu_score_util.py:43-58 on the counts: hl / rl = the words of the candidate / the caption (both >= n here).  Every line below is one
// fp64 operation of the reference, in its order; the sum is left to right.
__device__ __forceinline__ double bleu_fscore(const int (&acc)[4], int hl, int rl, int n, double fpr) {
    double sum = 0.0;                                                       // 0.0 + f_1 is f_1 exactly
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        if (o >= n) break;
        double f = 0.0;
        if (acc[o] != 0) {
            const double pre = (double)acc[o] / (double)(hl - o);          // target_num = len(t) - o + 1, o counted from 1
            const double rec = (double)acc[o] / (double)(rl - o);
            const double num = ((fpr + 1.0) * pre) * rec;
            const double den = rec + fpr * pre;
            f = num / den;
        }
        sum = sum + f;
    }
    return sum / (double)n;
}

// One workgroup per (candidate c, image i).  The candidate's key / count list sits in LDS (<= 250 keys for 64 words); the captions of
// the image's first k neighbour images are listed in neighbour order; thread t scores captions t, t + 256, ...; the pair scores are
// sorted descending in LDS and the first min(m, count) are added in that order by one thread (caption.h, shared with the 'cider' method).
__global__ __launch_bounds__(256) void bleu_score_kernel(const uint64_t* __restrict__ ckeys, const int32_t* __restrict__ ccounts,
                                                         const int32_t* __restrict__ ccnt, const int32_t* __restrict__ cwlen, int cstride,
                                                         const int32_t* __restrict__ seg, int top_k, const int32_t* __restrict__ nn, int nn_ld,
                                                         int k, const int32_t* __restrict__ cap_off, int n_img, const int32_t* __restrict__ nwoff,
                                                         const uint64_t* __restrict__ nkeys, const int32_t* __restrict__ ncounts,
                                                         const int32_t* __restrict__ ncnt, const int32_t* __restrict__ nwlen, int n, double fpr,
                                                         int m, int max_caps, double* __restrict__ sim, double* __restrict__ pair_out,
                                                         int64_t pair_ld) {
    __shared__ uint64_t hk[4 * kRowWords];
    __shared__ int32_t hc[4 * kRowWords];
    __shared__ double sc[kMaxCaps];
    __shared__ int32_t caps[kMaxCaps];
    __shared__ int32_t pre[kMaxK + 1];
    const int c = blockIdx.x, i = blockIdx.y, t = threadIdx.x;
    const int a = seg[i];
    int rows = seg[i + 1] - a;
    if (top_k > 0 && rows > top_k) rows = top_k;
    if (c >= rows) return;
    const int row = a + c;
    int na = ccnt[row];
    na = na < 0 ? 0 : (na > 4 * kRowWords ? 4 * kRowWords : na);
    if (na > cstride) na = cstride;
    for (int q = t; q < na; q += 256) {
        hk[q] = ckeys[(int64_t)row * cstride + q];
        hc[q] = ccounts[(int64_t)row * cstride + q];
    }
    const int nc = neighbour_captions(nn, nn_ld, i, k, cap_off, n_img, max_caps, pre, caps, t);
    const int hl = cwlen[row];
    __syncthreads();
    for (int j = t; j < nc; j += 256) {
        const int s = caps[j];
        const int rl = nwlen[s];
        double score = 0.0;
        if (n <= hl && n <= rl) {                                           // :27, on n itself: shorter sentences score 0 in every order
            const int nb = ncnt[s];
            int acc[4];
            bleu_walk(hk, hc, na, nkeys, ncounts, 4 * (int64_t)nwoff[s], nb, acc);
            score = bleu_fscore(acc, hl, rl, n, fpr);
        }
        sc[j] = score;
        if (pair_out) pair_out[(int64_t)row * pair_ld + j] = score;
    }
    const double acc = sum_top_desc(sc, nc, m, t);
    if (t == 0) sim[row] = acc;
}

}  // namespace

SUBGC_API int subgc_consensus_bleu_cook(const void* tok, int tok64, const int32_t* woff, int T, const int32_t* row_len, const uint8_t* bad,
                                        int bad_n, int S, int max_words, uint64_t* keys, int32_t* counts, int32_t* cnt, int32_t* wlen,
                                        void* stream) {
    SUBGC_REQUIRE(S >= 0 && (!bad || bad_n >= 1), "consensus_bleu_cook: S >= 0, bad_n >= 1 with a bad-endings table");
    SUBGC_REQUIRE(max_words >= 0 && max_words <= kMaxWords, "consensus_bleu_cook: a sentence holds at most %d words (got max_words = %d)",
                  kMaxWords, max_words);
    if (!woff) SUBGC_REQUIRE(T >= 1 && T <= kRowWords, "consensus_bleu_cook: token rows need 1 <= T <= %d (got %d)", kRowWords, T);
    if (S == 0) return SUBGC_OK;
    SUBGC_REQUIRE(tok && keys && counts && cnt && wlen, "consensus_bleu_cook: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (woff) {
        SUBGC_DEBUG_RANGE(woff, 4, 1, (int64_t)S + 1, (int64_t)S + 1, 0, (int64_t)1 << 29, -1, "consensus_bleu_cook: woff (CSR word offsets)", s);
        if (max_words > kRowWords)
            hipLaunchKernelGGL(bleu_cook_kernel<kMaxWords>, dim3(S), dim3(64), 0, s, tok, tok64, woff, T, row_len, bad, bad_n, keys, counts, cnt,
                               wlen);
        else
            hipLaunchKernelGGL(bleu_cook_kernel<kRowWords>, dim3(S), dim3(64), 0, s, tok, tok64, woff, T, row_len, bad, bad_n, keys, counts, cnt,
                               wlen);
    } else {
        hipLaunchKernelGGL(bleu_cook_kernel<kRowWords>, dim3(S), dim3(64), 0, s, tok, tok64, woff, T, row_len, bad, bad_n, keys, counts, cnt, wlen);
    }
    return subgc::check_launch("subgc_consensus_bleu_cook");
}

SUBGC_API int subgc_consensus_bleu_score(const uint64_t* ckeys, const int32_t* ccounts, const int32_t* ccnt, const int32_t* cwlen, int T,
                                         const int32_t* seg, int I, int max_cand, int top_k, const int32_t* nn, int nn_ld, int k,
                                         const int32_t* cap_off, int n_img, int n_caps, const int32_t* nwoff, const uint64_t* nkeys,
                                         const int32_t* ncounts, const int32_t* ncnt, const int32_t* nwlen, int n, double fpr, int m,
                                         int max_caps, double* sim, double* pair_out, int64_t pair_ld, void* stream) {
    SUBGC_REQUIRE(I >= 0 && max_cand >= 0 && top_k >= 0, "consensus_bleu_score: I, max_cand, top_k >= 0");
    SUBGC_REQUIRE(T >= 1 && T <= kRowWords, "consensus_bleu_score: 1 <= T <= %d (got %d)", kRowWords, T);
    SUBGC_REQUIRE(n >= 1 && n <= 4, "consensus_bleu_score: 1 <= n <= 4 n-gram orders (got %d)", n);
    SUBGC_REQUIRE(std::isfinite(fpr) && fpr >= 0.0, "consensus_bleu_score: fpr finite and >= 0 (got %g)", fpr);
    SUBGC_REQUIRE(m >= 1, "consensus_bleu_score: m >= 1 (got %d): the m largest pair scores are summed", m);
    SUBGC_REQUIRE(k >= 1 && k <= kMaxK, "consensus_bleu_score: 1 <= k <= %d neighbour images (got %d)", kMaxK, k);
    SUBGC_REQUIRE(k <= nn_ld, "consensus_bleu_score: k = %d is larger than the neighbour lists (%d entries per image)", k, nn_ld);
    SUBGC_REQUIRE(max_caps >= 0 && max_caps <= kMaxCaps, "consensus_bleu_score: at most %d neighbour captions per image (got %d)", kMaxCaps,
                  max_caps);
    SUBGC_REQUIRE(n_img >= 1 && n_caps >= 0, "consensus_bleu_score: n_img >= 1, n_caps >= 0");
    SUBGC_REQUIRE(!pair_out || pair_ld >= max_caps, "consensus_bleu_score: pair_ld shorter than max_caps");
    if (I == 0 || max_cand == 0) return SUBGC_OK;
    SUBGC_REQUIRE(ckeys && ccounts && ccnt && cwlen && seg && nn && cap_off && nwoff && nkeys && ncounts && ncnt && nwlen && sim,
                  "consensus_bleu_score: null pointer");
    hipStream_t s = (hipStream_t)stream;
    SUBGC_DEBUG_RANGE(nn, 4, I, k, nn_ld, 0, (int64_t)n_img - 1, -1, "consensus_bleu_score: nn (neighbour image indices)", s);
    SUBGC_DEBUG_RANGE(cap_off, 4, 1, (int64_t)n_img + 1, (int64_t)n_img + 1, 0, n_caps, -1, "consensus_bleu_score: cap_off (CSR caption offsets)", s);
    const int cand = top_k > 0 && top_k < max_cand ? top_k : max_cand;
    hipLaunchKernelGGL(bleu_score_kernel, dim3(cand, I), dim3(256), 0, s, ckeys, ccounts, ccnt, cwlen, 4 * T, seg, top_k, nn, nn_ld, k, cap_off,
                       n_img, nwoff, nkeys, ncounts, ncnt, nwlen, n, fpr, m, max_caps, sim, pair_out, pair_ld);
    return subgc::check_launch("subgc_consensus_bleu_score");
}
