// Accuracy scores of a decode batch (include/subgc_metrics_hip.h): per candidate row the BLEU material and sentence BLEU-1 .. 4
// (pycocoevalcap/bleu/bleu_scorer.py:26-93,208-256), CIDEr (pycocoevalcap/cider/cider_scorer.py:95-184) and ROUGE-L
// (pycocoevalcap/rouge/rouge.py:15-77) against the reference captions of the row's image, then per image the oracle picks over its
// first oracle_num rows and the top-1 row (misc/sentence_utils.py:28-53,108-125).  Two kernels: one workgroup per row, one per image.
// Words are 16-bit ids and n-grams 64-bit keys by caption.h, which also holds the caption rule of a token row; consensus.hip's cook
// launch prepares the tf-idf lists of both sides; counts
// are integers (LDS integer adds: order-free), the arithmetic is fp64 in the reference's own order, summed by one thread, with FMA
// contraction off for the whole file: equal inputs give equal bits, and ROUGE-L's and CIDEr's expressions round as Python's do.
#include "common.h"

#include "../../include/subgc_metrics_hip.h"

#pragma clang fp contract(off)

#include "caption.h"      // after the pragma: its functions are compiled without contraction here

namespace {

constexpr int kRowWords = 64;                           // words of a candidate row (the decode's T): one wavefront
constexpr int kRefWords = SUBGC_ACC_MAX_REF_WORDS;      // words of a reference caption
constexpr int kMaxRefs = SUBGC_ACC_MAX_REFS;            // reference captions of an image
constexpr int kRowKeys = 4 * kRowWords;                 // n-grams of a row, all orders

// One workgroup (4 waves) per candidate row.
//   BLEU: the row's <= 250 n-gram keys in LDS; the first occurrence of a key counts its repeats, finds the image's largest reference
//     count by binary search in the image's sorted table and adds min(count, that) to its order (cook_test, bleu_scorer.py:88-91).
//   CIDEr: thread s < R scores reference s against the row's cooked list (in LDS) by caption.h's cider_walk and cider_finish (sim,
//     cider_scorer.py:139-154); the R results wait in LDS for the one thread that adds them in reference order.
//   ROUGE-L: lane j of a wave holds word j of the row; a reference goes to a wave, each of its words w is one match mask
//     __ballot(word_j == w) and one step U = V & M, V = (V + U) | (V - U) of the bit-vector LCS on a 64-bit word; the LCS is the number of
//     zero bits among the row's low bits (my_lcs, rouge.py:15-37, without its table).
//   Thread 0 then spells the three scorers' fp64 arithmetic.
__global__ __launch_bounds__(256) void rows_kernel(const void* __restrict__ tok, int tok64, int T, const uint8_t* __restrict__ bad, int bad_n, int rows,
                                                   const int32_t* __restrict__ seg, int I, const int32_t* __restrict__ img_ref, int n_ref,
                                                   const uint64_t* __restrict__ ckeys, const double* __restrict__ cw, const int32_t* __restrict__ ccnt,
                                                   const int32_t* __restrict__ clen, const double* __restrict__ cnorm,
                                                   const int32_t* __restrict__ cap_off, int n_caps, const int32_t* __restrict__ rwoff,
                                                   const int32_t* __restrict__ rtok, int n_words, const uint64_t* __restrict__ rkeys,
                                                   const double* __restrict__ rw, const int32_t* __restrict__ rcnt, const int32_t* __restrict__ rlen,
                                                   const double* __restrict__ rnorm, const int32_t* __restrict__ boff,
                                                   const uint64_t* __restrict__ bkeys, const int32_t* __restrict__ bmax, int n_bkeys,
                                                   const double* __restrict__ gauss, int n_gauss, double beta2, int32_t* __restrict__ out_i, int ld_i,
                                                   double* __restrict__ out_d, int ld_d) {
    __shared__ uint32_t tk[kRowWords];
    __shared__ uint64_t gk[kRowKeys];
    __shared__ uint64_t hk[kRowKeys];
    __shared__ double hw[kRowKeys];
    __shared__ double cval[kMaxRefs * 4];
    __shared__ uint32_t rwd[4][kRefWords];
    __shared__ int lcs_sh[kMaxRefs], rl_sh[kMaxRefs], wl_sh[kMaxRefs];
    __shared__ int correct[4];
    __shared__ int L_sh;
    const int r = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    // the row's image: the last i with seg[i] <= r (a seg that is not monotone names some image; nothing is read out of range)
    int lo = 0, hi = I - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (seg[mid] <= r) lo = mid; else hi = mid - 1;
    }
    const int j = clampi(img_ref[lo], 0, n_ref - 1);
    const int c0 = clampi(cap_off[j], 0, n_caps), c1 = clampi(cap_off[j + 1], c0, n_caps);
    const int R = c1 - c0 < kMaxRefs ? c1 - c0 : kMaxRefs;
    const int b0 = clampi(boff[j], 0, n_bkeys), b1 = clampi(boff[j + 1], b0, n_bkeys);
    const int cstride = 4 * T;
    const int na = clampi(ccnt[r], 0, cstride < kRowKeys ? cstride : kRowKeys);
    if (wave == 0) {
        int64_t v;
        const int L = load_row(tok, tok64, T, r, bad, bad_n, lane, v);
        tk[lane] = lane < L ? (uint32_t)v & 0xffffu : 0u;
        if (lane == 0) L_sh = L;
    }
    if (t < 4) correct[t] = 0;
    for (int q = t; q < na; q += 256) {
        hk[q] = ckeys[(int64_t)r * cstride + q];
        hw[q] = cw[(int64_t)r * cstride + q];
    }
    __syncthreads();
    const int L = L_sh;
    int nk = 0;
    for (int o = 0; o < 4; ++o) {
        const int c = L - o;
        if (c <= 0) break;
        if (t < c) gk[nk + t] = ngram_key(tk, t, o);
        nk += c;
    }
    __syncthreads();
    for (int g = t; g < nk; g += 256) {
        const uint64_t key = gk[g];
        int c = 0, before = 0;                                              // caption.h's count_key, kept inline: through the function this
        for (int q = 0; q < nk; ++q) {                                      // kernel measured 0.8 us of 69 slower (profiles/r14)
            const bool same = gk[q] == key;
            c += same;
            before += same && q < g;
        }
        if (before) continue;
        int p0 = b0, p1 = b1;                                               // first table entry that is not below the key
        while (p0 < p1) {
            const int mid = (p0 + p1) >> 1;
            if (bkeys[mid] < key) p0 = mid + 1; else p1 = mid;
        }
        const int mx = (p0 < b1 && bkeys[p0] == key) ? bmax[p0] : 0;
        const int hit = c < mx ? c : mx;
        if (hit > 0) atomicAdd(&correct[key_order(key)], hit);              // integer adds: the result does not depend on the order
    }
    if (t < R) {
        const int s = c0 + t;
        const int w0 = clampi(rwoff[s], 0, n_words), w1 = clampi(rwoff[s + 1], w0, n_words);
        const int Lr = w1 - w0 < kRefWords ? w1 - w0 : kRefWords;
        const int64_t base = 4 * (int64_t)w0;
        const int nb = clampi(rcnt[s], 0, 4 * Lr);
        double v[4];
        cider_walk(hk, hw, na, rkeys, rw, base, nb, v);
        const double hn[4] = {cnorm[(int64_t)r * 4], cnorm[(int64_t)r * 4 + 1], cnorm[(int64_t)r * 4 + 2], cnorm[(int64_t)r * 4 + 3]};
        const double rn[4] = {rnorm[(int64_t)s * 4], rnorm[(int64_t)s * 4 + 1], rnorm[(int64_t)s * 4 + 2], rnorm[(int64_t)s * 4 + 3]};
        int d = clen[r] - rlen[s];
        d = d < 0 ? -d : d;
        cider_finish(v, hn, rn, gauss[clampi(d, 0, n_gauss - 1)]);
        for (int k = 0; k < 4; ++k) cval[t * 4 + k] = v[k];
        wl_sh[t] = Lr;
    }
    // ROUGE-L: `split(" ")` makes an empty caption ONE word, the empty word (id 0: never a real word), on both sides
    const int Lc = L > 0 ? L : 1;
    const uint32_t mine = lane < Lc ? tk[lane] : 0xffffffffu;               // tk[0] = 0 for an empty row; past the row: matches nothing
    const unsigned long long low = Lc >= 64 ? ~0ull : ((1ull << Lc) - 1ull);
    for (int s0 = 0; s0 < R; s0 += 4) {                                     // the same trip count in every wave: the barriers are uniform
        const int q = s0 + wave;
        int Lr = 0;
        if (q < R) {
            const int s = c0 + q;
            const int w0 = clampi(rwoff[s], 0, n_words), w1 = clampi(rwoff[s + 1], w0, n_words);
            Lr = w1 - w0 < kRefWords ? w1 - w0 : kRefWords;
            for (int p = lane; p < Lr; p += 64) rwd[wave][p] = (uint32_t)rtok[w0 + p] & 0xffffu;
            if (Lr == 0) {
                if (lane == 0) rwd[wave][0] = 0u;
                Lr = 1;
            }
        }
        __syncthreads();
        unsigned long long V = ~0ull;
        for (int p = 0; p < Lr; ++p) {
            const unsigned long long M = __ballot(mine == rwd[wave][p]);
            const unsigned long long U = V & M;
            V = (V + U) | (V - U);
        }
        if (q < R && lane == 0) {
            lcs_sh[q] = __popcll(~V & low);
            rl_sh[q] = Lr;
        }
        __syncthreads();
    }
    __syncthreads();
    if (t != 0) return;
    int32_t* oi = out_i + (int64_t)r * ld_i;
    double* od = out_d + (int64_t)r * ld_d;
    const double small = 1e-9, tiny = 1e-15;
    // BLEU (bleu_scorer.py:76-77, the closest reference length; :242-252)
    const int testlen = L, reflen = closest_len(wl_sh, R, -1, testlen);
    oi[SUBGC_ACC_TESTLEN] = testlen;
    oi[SUBGC_ACC_REFLEN] = reflen;
    double prod = 1.0, bl[4];
    for (int k = 0; k < 4; ++k) {
        const int guess = testlen - k > 0 ? testlen - k : 0;
        oi[SUBGC_ACC_GUESS + k] = guess;
        oi[SUBGC_ACC_CORRECT + k] = correct[k];
        prod *= ((double)correct[k] + tiny) / ((double)guess + small);
        bl[k] = k == 0 ? prod : (k == 1 ? sqrt(prod) : pow(prod, 1.0 / (double)(k + 1)));
    }
    const double ratio = ((double)testlen + tiny) / ((double)reflen + small);
    if (ratio < 1.0) {
        const double bp = exp(1.0 - 1.0 / ratio);
        for (int k = 0; k < 4; ++k) bl[k] *= bp;
    }
    for (int k = 0; k < 4; ++k) od[SUBGC_ACC_BLEU + k] = bl[k];
    // CIDEr (cider_scorer.py:166-180): the references in reference order, np.mean of the four orders, / R, x 10
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (int s = 0; s < R; ++s) {
        s0 += cval[s * 4];
        s1 += cval[s * 4 + 1];
        s2 += cval[s * 4 + 2];
        s3 += cval[s * 4 + 3];
    }
    double cider = (((s0 + s1) + s2) + s3) / 4.0;
    cider /= (double)(R > 0 ? R : 1);
    cider *= 10.0;
    od[SUBGC_ACC_CIDER] = cider;
    // ROUGE-L (rouge.py:64-76)
    double pmax = 0.0, rmax = 0.0;
    for (int s = 0; s < R; ++s) {
        const double p = (double)lcs_sh[s] / (double)Lc, q = (double)lcs_sh[s] / (double)rl_sh[s];
        pmax = p > pmax ? p : pmax;
        rmax = q > rmax ? q : rmax;
    }
    double rouge = 0.0;
    if (pmax != 0.0 && rmax != 0.0) rouge = (((1.0 + beta2) * pmax) * rmax) / (rmax + beta2 * pmax);
    od[SUBGC_ACC_ROUGE] = rouge;
}

// One workgroup per image: the oracle over its first min(n_i, oracle_num) rows and the top-1 row.  Thread t keeps the best of rows
// t, t + 256, ... (ascending, so `>` keeps the first); six threads then scan the 256 partial results, the lower row winning a tie.
__global__ __launch_bounds__(256) void oracle_kernel(const int32_t* __restrict__ row_i, int ld_i, const double* __restrict__ row_d, int ld_d, int rows,
                                                     const int32_t* __restrict__ seg, int I, int oracle_num, const int32_t* __restrict__ first,
                                                     int32_t* __restrict__ img_i, int ld_ii, double* __restrict__ img_d, int ld_id) {
    __shared__ double bv[6][256];
    __shared__ int bi[6][256];
    const int i = blockIdx.x, t = threadIdx.x;
    const int a = clampi(seg[i], 0, rows), b = clampi(seg[i + 1], a, rows);
    const int n = b - a, m = n < oracle_num ? n : oracle_num;
    int32_t* oi = img_i + (int64_t)i * ld_ii;
    double* od = img_d + (int64_t)i * ld_id;
    if (n <= 0) {
        for (int q = t; q < SUBGC_ACC_IMG_INT; q += 256) oi[q] = 0;
        if (t < SUBGC_ACC_IMG_F64) od[t] = 0.0;
        return;
    }
    double best[6];
    int idx[6];
    for (int k = 0; k < 6; ++k) { best[k] = -1.0; idx[k] = 0x7fffffff; }    // every score is >= 0
    for (int r = t; r < m; r += 256) {
        const double* v = row_d + (int64_t)(a + r) * ld_d;
        for (int k = 0; k < 6; ++k)
            if (v[k] > best[k]) { best[k] = v[k]; idx[k] = r; }
    }
    for (int k = 0; k < 6; ++k) { bv[k][t] = best[k]; bi[k][t] = idx[k]; }
    __syncthreads();
    if (t < 6) {
        double bb = bv[t][0];
        int ii = bi[t][0];
        for (int q = 1; q < 256; ++q) {
            const double v = bv[t][q];
            const int x = bi[t][q];
            if (v > bb || (v == bb && x < ii)) { bb = v; ii = x; }
        }
        ii = clampi(ii, 0, n - 1);
        od[SUBGC_ACC_IMG_BEST + t] = bb;
        if (t < 4) {
            oi[SUBGC_ACC_IMG_PICK + t] = ii;
            const int32_t* src = row_i + (int64_t)(a + ii) * ld_i;
            for (int q = 0; q < SUBGC_ACC_ROW_INT; ++q) oi[SUBGC_ACC_IMG_PICK_MAT + t * SUBGC_ACC_ROW_INT + q] = src[q];
        }
    } else if (t == 64) {
        const int f = first ? clampi(first[i], 0, n - 1) : 0;
        oi[SUBGC_ACC_IMG_ROWS] = m;
        oi[SUBGC_ACC_IMG_TOP1] = f;
        const int32_t* src = row_i + (int64_t)(a + f) * ld_i;
        for (int q = 0; q < SUBGC_ACC_ROW_INT; ++q) oi[SUBGC_ACC_IMG_TOP1_MAT + q] = src[q];
        const double* v = row_d + (int64_t)(a + f) * ld_d;
        for (int q = 0; q < SUBGC_ACC_ROW_F64; ++q) od[SUBGC_ACC_IMG_TOP1_VAL + q] = v[q];
    }
}

}  // namespace

SUBGC_API int subgc_accuracy_rows(const void* tok, int tok64, int T, const uint8_t* bad, int bad_n, int rows, const int32_t* seg, int I,
                                  const int32_t* img_ref, int n_ref, const uint64_t* ckeys, const double* cw, const int32_t* ccnt,
                                  const int32_t* clen, const double* cnorm, const int32_t* cap_off, int n_caps, const int32_t* rwoff,
                                  const int32_t* rtok, int n_words, const uint64_t* rkeys, const double* rw, const int32_t* rcnt,
                                  const int32_t* rlen, const double* rnorm, const int32_t* boff, const uint64_t* bkeys, const int32_t* bmax,
                                  int n_bkeys, const double* gauss, int n_gauss, double beta2, int32_t* out_i, int ld_i, double* out_d, int ld_d,
                                  void* stream) {
    SUBGC_REQUIRE(rows >= 0 && I >= 0 && n_ref >= 0 && n_caps >= 0 && n_words >= 0 && n_bkeys >= 0 && (!bad || bad_n >= 1),
                  "accuracy_rows: rows, I, n_ref, n_caps, n_words, n_bkeys >= 0, bad_n >= 1 with a bad-endings table");
    SUBGC_REQUIRE(T >= 1 && T <= kRowWords, "accuracy_rows: token rows need 1 <= T <= %d (got %d)", kRowWords, T);
    SUBGC_REQUIRE(ld_i >= SUBGC_ACC_ROW_INT && ld_d >= SUBGC_ACC_ROW_F64, "accuracy_rows: ld_i shorter than %d or ld_d shorter than %d",
                  SUBGC_ACC_ROW_INT, SUBGC_ACC_ROW_F64);
    if (rows == 0) return SUBGC_OK;
    SUBGC_REQUIRE(I >= 1 && n_ref >= 1 && n_caps >= 1 && n_gauss >= 1, "accuracy_rows: rows without an image, a reference image, a reference caption or a "
                                                                       "length-factor table");
    SUBGC_REQUIRE(tok && seg && img_ref && ckeys && cw && ccnt && clen && cnorm && cap_off && rwoff && rcnt && rlen && rnorm && boff && gauss &&
                      out_i && out_d && (n_words == 0 || (rtok && rkeys && rw)) && (n_bkeys == 0 || (bkeys && bmax)),
                  "accuracy_rows: null pointer");
    hipStream_t s = (hipStream_t)stream;
    SUBGC_DEBUG_MONO("accuracy_rows", "seg (row boundaries of the images)", "image", seg, I, rows, s);
    SUBGC_DEBUG_RANGE(img_ref, 4, 1, I, I, 0, (int64_t)n_ref - 1, -1, "accuracy_rows: img_ref (reference image of every batch image)", s);
    SUBGC_DEBUG_RANGE(cap_off, 4, 1, (int64_t)n_ref + 1, (int64_t)n_ref + 1, 0, n_caps, -1, "accuracy_rows: cap_off (CSR caption offsets)", s);
    SUBGC_DEBUG_RANGE(rwoff, 4, 1, (int64_t)n_caps + 1, (int64_t)n_caps + 1, 0, n_words, -1, "accuracy_rows: rwoff (CSR word offsets)", s);
    SUBGC_DEBUG_RANGE(boff, 4, 1, (int64_t)n_ref + 1, (int64_t)n_ref + 1, 0, n_bkeys, -1, "accuracy_rows: boff (CSR n-gram table offsets)", s);
    hipLaunchKernelGGL(rows_kernel, dim3(rows), dim3(256), 0, s, tok, tok64, T, bad, bad_n, rows, seg, I, img_ref, n_ref, ckeys, cw, ccnt, clen, cnorm,
                       cap_off, n_caps, rwoff, rtok, n_words, rkeys, rw, rcnt, rlen, rnorm, boff, bkeys, bmax, n_bkeys, gauss, n_gauss, beta2, out_i,
                       ld_i, out_d, ld_d);
    return subgc::check_launch("subgc_accuracy_rows");
}

SUBGC_API int subgc_accuracy_oracle(const int32_t* row_i, int ld_i, const double* row_d, int ld_d, int rows, const int32_t* seg, int I,
                                    int oracle_num, const int32_t* first, int32_t* img_i, int ld_ii, double* img_d, int ld_id, void* stream) {
    SUBGC_REQUIRE(rows >= 0 && I >= 0, "accuracy_oracle: rows, I >= 0");
    SUBGC_REQUIRE(oracle_num >= 1, "accuracy_oracle: oracle_num >= 1 (got %d)", oracle_num);
    SUBGC_REQUIRE(ld_i >= SUBGC_ACC_ROW_INT && ld_d >= SUBGC_ACC_ROW_F64 && ld_ii >= SUBGC_ACC_IMG_INT && ld_id >= SUBGC_ACC_IMG_F64,
                  "accuracy_oracle: a leading dimension is shorter than its record (%d, %d, %d, %d)", SUBGC_ACC_ROW_INT, SUBGC_ACC_ROW_F64,
                  SUBGC_ACC_IMG_INT, SUBGC_ACC_IMG_F64);
    if (I == 0) return SUBGC_OK;
    SUBGC_REQUIRE(seg && img_i && img_d && (rows == 0 || (row_i && row_d)), "accuracy_oracle: null pointer");
    hipStream_t s = (hipStream_t)stream;
    SUBGC_DEBUG_MONO("accuracy_oracle", "seg (row boundaries of the images)", "image", seg, I, rows, s);
    hipLaunchKernelGGL(oracle_kernel, dim3(I), dim3(256), 0, s, row_i, ld_i, row_d, ld_d, rows, seg, I, oracle_num, first, img_i, ld_ii, img_d, ld_id);
    return subgc::check_launch("subgc_accuracy_oracle");
}
