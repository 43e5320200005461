// Consensus re-ranking, method 'cider' (misc/consensus_reranking/concensus_reranking_utils/consensus_reranking.py:152-174 with
// CiderScorer.compute_cider_sen_pair, external/coco_caption_patch_mRNN_cr/cider_scorer_compute_sentence.py:187-264) for a whole decode
// batch: every candidate caption of every image against the captions of the image's k nearest training images, the m largest pair
// scores summed, the candidates ordered by that sum.  Words are 16-bit ids (1 .. 65535; 0 never inside a sentence), an n-gram of order
// 1 .. 4 is ONE 64-bit key (caption.h, which also holds the caption rule of a token row and the pair walk), so all matching is exact
// integer comparison -- no hashing.  Arithmetic is fp64 with a summation order fixed by the inputs alone: no float
// atomics, equal inputs give equal bits.  log(df), log(#images) and the Gaussian length factor come from the host (numpy, the reference's
// own expressions); the device adds, multiplies, takes min, divides and takes square roots.
#include "common.h"
#include "caption.h"

namespace {

constexpr int kMaxCaps = 2048;      // neighbour captions per image (60 neighbours x up to ~7 captions, with slack)
constexpr int kMaxK = 256;          // neighbour images per image
constexpr int kRowWords = 64;       // words of a candidate row (the decode's T)
constexpr int kMaxWords = 256;      // words of a corpus caption

// One wave per sentence ("cook", precook + counts2vec, cider_scorer_compute_sentence.py:15-30,188-212): the <= 4 L n-gram keys, each
// DISTINCT key once with tf = its count, in ascending key order (rank by counting: n is ~74 for a 20-word caption), weight
// tf * (ref_len - log df) with log df found by binary search in the corpus's sorted unique keys (absent: df = 0 -> log 1 = 0), the four
// norms (summed in key order by one lane each) and the length = the number of BIGRAMS, max(L - 1, 0) (:209-210).
// Sentence s: CSR mode (woff != NULL) words tok[woff[s] .. woff[s+1]), all non-zero; row mode: row s of tok [S, T] by caption.h's
// load_row, capped at row_len[s] words (row_len NULL or negative: no cap).  Its list lands at keys / wts [4 * first word index ...].
template <int MAXW>
__global__ __launch_bounds__(64) void cook_kernel(const void* __restrict__ tok, int tok64, const int32_t* __restrict__ woff, int T,
                                                  const int32_t* __restrict__ row_len, const uint8_t* __restrict__ bad, int bad_n,
                                                  const uint64_t* __restrict__ ukeys, const double* __restrict__ ulogdf, int64_t U,
                                                  double ref_len, uint64_t* __restrict__ keys, double* __restrict__ wts,
                                                  int32_t* __restrict__ cnt, int32_t* __restrict__ blen, double* __restrict__ norm) {
    constexpr int MAXK = 4 * MAXW;
    __shared__ uint32_t tk[MAXW];
    __shared__ uint64_t gk[MAXK];
    __shared__ int32_t tf[MAXK];                                           // > 0: first occurrence of its key, the key's count; 0: a repeat
    __shared__ uint64_t ok[MAXK];
    __shared__ double ow[MAXK];
    __shared__ int nu_sh;
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
    if (lane == 0) nu_sh = 0;
    __syncthreads();
    int nk = 0;
    for (int o = 0; o < 4; ++o) {
        const int c = L - o;
        if (c <= 0) break;
        for (int p = lane; p < c; p += 64) gk[nk + p] = ngram_key(tk, p, o);
        nk += c;
    }
    __syncthreads();
    int mine = 0;
    for (int i = lane; i < nk; i += 64) {
        int before;
        const int eq = count_key(gk, 0, nk, i, before);
        tf[i] = before == 0 ? eq : 0;
        mine += before == 0;
    }
    if (mine) atomicAdd(&nu_sh, mine);                                      // an integer count: the result does not depend on the order
    __syncthreads();
    const int nu = nu_sh;
    for (int i = lane; i < nk; i += 64) {
        const int f = tf[i];
        if (f == 0) continue;
        const uint64_t ki = gk[i];
        int u = 0;
        for (int j = 0; j < nk; ++j) u += tf[j] > 0 && gk[j] < ki;
        int64_t lo = 0, hi = U;                                             // first position with ukeys[pos] >= ki
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (ukeys[mid] < ki) lo = mid + 1; else hi = mid;
        }
        const double ldf = (lo < U && ukeys[lo] == ki) ? ulogdf[lo] : 0.0;
        ok[u] = ki;
        ow[u] = (double)f * (ref_len - ldf);
    }
    __syncthreads();
    const int64_t base = 4 * start;
    for (int u = lane; u < nu; u += 64) {
        keys[base + u] = ok[u];
        wts[base + u] = ow[u];
    }
    if (lane < 4) {
        double acc = 0.0;
        for (int u = 0; u < nu; ++u)
            if (key_order(ok[u]) == lane) acc += ow[u] * ow[u];
        norm[(int64_t)s * 4 + lane] = sqrt(acc);
    }
    if (lane == 0) {
        cnt[s] = nu;
        blen[s] = L > 0 ? L - 1 : 0;
    }
}

// One workgroup per (candidate c, image i).  The candidate's cooked list sits in LDS; the captions of the image's first k neighbour
// images are listed in neighbour order (consensus_reranking.py:155-157); thread t scores captions t, t + 256, ... by
// caption.h's cider_walk and cider_finish, all four orders in the one pass (sim(), cider_scorer_compute_sentence.py:225-240).  The pair scores are sorted descending in LDS and the first min(m, count) are added in
// that order by one thread, as `b_s_arr.sort(reverse=True); sum(b_s_arr[:m])` does (:168-169).
__global__ __launch_bounds__(256) void score_kernel(const uint64_t* __restrict__ ckeys, const double* __restrict__ cw,
                                                    const int32_t* __restrict__ ccnt, const int32_t* __restrict__ clen,
                                                    const double* __restrict__ cnorm, int cstride, const int32_t* __restrict__ seg, int top_k,
                                                    const int32_t* __restrict__ nn, int nn_ld, int k, const int32_t* __restrict__ cap_off,
                                                    int n_img, const int32_t* __restrict__ nwoff, const uint64_t* __restrict__ nkeys,
                                                    const double* __restrict__ nw, const int32_t* __restrict__ ncnt,
                                                    const int32_t* __restrict__ nlen, const double* __restrict__ nnorm,
                                                    const double* __restrict__ gauss, int n_gauss, int m, int max_caps,
                                                    double* __restrict__ sim, double* __restrict__ pair_out, int64_t pair_ld) {
    __shared__ uint64_t hk[4 * kRowWords];
    __shared__ double hw[4 * kRowWords];
    __shared__ double sc[kMaxCaps];
    __shared__ int32_t caps[kMaxCaps];
    __shared__ int32_t pre[kMaxK + 1];
    const int c = blockIdx.x, i = blockIdx.y, t = threadIdx.x;
    const int a = seg[i];
    int n = seg[i + 1] - a;
    if (top_k > 0 && n > top_k) n = top_k;
    if (c >= n) return;
    const int row = a + c;
    int na = ccnt[row];
    na = na < 0 ? 0 : (na > 4 * kRowWords ? 4 * kRowWords : na);
    for (int q = t; q < na; q += 256) {
        hk[q] = ckeys[(int64_t)row * cstride + q];
        hw[q] = cw[(int64_t)row * cstride + q];
    }
    const int nc = neighbour_captions(nn, nn_ld, i, k, cap_off, n_img, max_caps, pre, caps, t);
    const double hn[4] = {cnorm[(int64_t)row * 4], cnorm[(int64_t)row * 4 + 1], cnorm[(int64_t)row * 4 + 2], cnorm[(int64_t)row * 4 + 3]};
    const int hl = clen[row];
    __syncthreads();
    for (int j = t; j < nc; j += 256) {
        const int s = caps[j];
        const int64_t base = 4 * (int64_t)nwoff[s];
        const int nb = ncnt[s];
        double v[4];
        cider_walk(hk, hw, na, nkeys, nw, base, nb, v);
        const double rn[4] = {nnorm[(int64_t)s * 4], nnorm[(int64_t)s * 4 + 1], nnorm[(int64_t)s * 4 + 2], nnorm[(int64_t)s * 4 + 3]};
        int d = hl - nlen[s];
        d = d < 0 ? -d : d;
        cider_finish(v, hn, rn, gauss[d < n_gauss ? d : n_gauss - 1]);
        const double score = (((v[0] + v[1]) + v[2]) + v[3]) / 4.0 * 10.0;         // np.mean of the four orders, x 10 (:257-261)
        sc[j] = score;
        if (pair_out) pair_out[(int64_t)row * pair_ld + j] = score;
    }
    const double acc = sum_top_desc(sc, nc, m, t);
    if (t == 0) sim[row] = acc;
}

// One workgroup per image: order[seg[i] + r] = the image-local index of its r-th best candidate by the fp64 sums, descending, equal sums
// in ascending candidate index (stable: the reference's np.argsort(-sim) leaves ties open, consensus_reranking.py:172, and duplicate
// captions make exact ties routine); first[i] = order[seg[i]] (0 for an image without candidates): the grounding pick.
__global__ __launch_bounds__(256) void rank_kernel(const double* __restrict__ sim, const int32_t* __restrict__ seg, int top_k,
                                                   int32_t* __restrict__ order, int32_t* __restrict__ first) {
    const int i = blockIdx.x;
    const int a = seg[i];
    int n = seg[i + 1] - a;
    if (top_k > 0 && n > top_k) n = top_k;
    if (n <= 0) {
        if (threadIdx.x == 0 && first) first[i] = 0;
        return;
    }
    for (int r = threadIdx.x; r < n; r += blockDim.x) {
        const double v = sim[a + r];
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const double u = sim[a + j];
            rank += (u > v) || (u == v && j < r);
        }
        order[a + rank] = r;
        if (rank == 0 && first) first[i] = r;
    }
}

}  // namespace

SUBGC_API int subgc_consensus_cook(const void* tok, int tok64, const int32_t* woff, int T, const int32_t* row_len, const uint8_t* bad, int bad_n,
                                   int S, int max_words, const uint64_t* ukeys, const double* ulogdf, int64_t U, double ref_len, uint64_t* keys,
                                   double* wts, int32_t* cnt, int32_t* blen, double* norm, void* stream) {
    SUBGC_REQUIRE(S >= 0 && U >= 0 && (!bad || bad_n >= 1), "consensus_cook: S, U >= 0, bad_n >= 1 with a bad-endings table");
    SUBGC_REQUIRE(max_words >= 0 && max_words <= kMaxWords, "consensus_cook: a sentence holds at most %d words (got max_words = %d)", kMaxWords,
                  max_words);
    if (!woff) SUBGC_REQUIRE(T >= 1 && T <= kRowWords, "consensus_cook: token rows need 1 <= T <= %d (got %d)", kRowWords, T);
    if (S == 0) return SUBGC_OK;
    SUBGC_REQUIRE(tok && keys && wts && cnt && blen && norm && (U == 0 || (ukeys && ulogdf)), "consensus_cook: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (woff) {
        SUBGC_DEBUG_RANGE(woff, 4, 1, (int64_t)S + 1, (int64_t)S + 1, 0, (int64_t)1 << 29, -1, "consensus_cook: woff (CSR word offsets)", s);
        if (max_words > kRowWords)
            hipLaunchKernelGGL(cook_kernel<kMaxWords>, dim3(S), dim3(64), 0, s, tok, tok64, woff, T, row_len, bad, bad_n, ukeys, ulogdf, U, ref_len,
                               keys, wts, cnt, blen, norm);
        else
            hipLaunchKernelGGL(cook_kernel<kRowWords>, dim3(S), dim3(64), 0, s, tok, tok64, woff, T, row_len, bad, bad_n, ukeys, ulogdf, U, ref_len,
                               keys, wts, cnt, blen, norm);
    } else {
        hipLaunchKernelGGL(cook_kernel<kRowWords>, dim3(S), dim3(64), 0, s, tok, tok64, woff, T, row_len, bad, bad_n, ukeys, ulogdf, U, ref_len, keys,
                           wts, cnt, blen, norm);
    }
    return subgc::check_launch("subgc_consensus_cook");
}

SUBGC_API int subgc_consensus_score(const uint64_t* ckeys, const double* cw, const int32_t* ccnt, const int32_t* clen, const double* cnorm, int T,
                                    const int32_t* seg, int I, int max_cand, int top_k, const int32_t* nn, int nn_ld, int k,
                                    const int32_t* cap_off, int n_img, int n_caps, const int32_t* nwoff, const uint64_t* nkeys, const double* nw,
                                    const int32_t* ncnt, const int32_t* nlen, const double* nnorm, const double* gauss, int n_gauss, int m,
                                    int max_caps, double* sim, double* pair_out, int64_t pair_ld, void* stream) {
    SUBGC_REQUIRE(I >= 0 && max_cand >= 0 && top_k >= 0, "consensus_score: I, max_cand, top_k >= 0");
    SUBGC_REQUIRE(T >= 1 && T <= kRowWords, "consensus_score: 1 <= T <= %d (got %d)", kRowWords, T);
    SUBGC_REQUIRE(m >= 1, "consensus_score: m >= 1 (got %d): the m largest pair scores are summed", m);
    SUBGC_REQUIRE(k >= 1 && k <= kMaxK, "consensus_score: 1 <= k <= %d neighbour images (got %d)", kMaxK, k);
    SUBGC_REQUIRE(k <= nn_ld, "consensus_score: k = %d is larger than the neighbour lists (%d entries per image)", k, nn_ld);
    SUBGC_REQUIRE(max_caps >= 0 && max_caps <= kMaxCaps, "consensus_score: at most %d neighbour captions per image (got %d)", kMaxCaps, max_caps);
    SUBGC_REQUIRE(n_img >= 1 && n_caps >= 0 && n_gauss >= 1, "consensus_score: n_img >= 1, n_caps >= 0, n_gauss >= 1");
    SUBGC_REQUIRE(!pair_out || pair_ld >= max_caps, "consensus_score: pair_ld shorter than max_caps");
    if (I == 0 || max_cand == 0) return SUBGC_OK;
    SUBGC_REQUIRE(ckeys && cw && ccnt && clen && cnorm && seg && nn && cap_off && nwoff && nkeys && nw && ncnt && nlen && nnorm && gauss && sim,
                  "consensus_score: null pointer");
    hipStream_t s = (hipStream_t)stream;
    SUBGC_DEBUG_RANGE(nn, 4, I, k, nn_ld, 0, (int64_t)n_img - 1, -1, "consensus_score: nn (neighbour image indices)", s);
    SUBGC_DEBUG_RANGE(cap_off, 4, 1, (int64_t)n_img + 1, (int64_t)n_img + 1, 0, n_caps, -1, "consensus_score: cap_off (CSR caption offsets)", s);
    const int cand = top_k > 0 && top_k < max_cand ? top_k : max_cand;
    hipLaunchKernelGGL(score_kernel, dim3(cand, I), dim3(256), 0, s, ckeys, cw, ccnt, clen, cnorm, 4 * T, seg, top_k, nn, nn_ld, k, cap_off, n_img,
                       nwoff, nkeys, nw, ncnt, nlen, nnorm, gauss, n_gauss, m, max_caps, sim, pair_out, pair_ld);
    return subgc::check_launch("subgc_consensus_score");
}

SUBGC_API int subgc_consensus_rank(const double* sim, const int32_t* seg, int I, int top_k, int32_t* order, int32_t* first, void* stream) {
    SUBGC_REQUIRE(I >= 0 && top_k >= 0, "consensus_rank: I, top_k >= 0");
    if (I == 0) return SUBGC_OK;
    SUBGC_REQUIRE(sim && seg && order, "consensus_rank: null pointer");
    hipLaunchKernelGGL(rank_kernel, dim3(I), dim3(256), 0, (hipStream_t)stream, sim, seg, top_k, order, first);
    return subgc::check_launch("subgc_consensus_rank");
}
