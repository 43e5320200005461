// Diversity scores of a decode batch (misc/diversity/diversity_score.py:55-163; the sentence BLEU-4 is bleu_scorer.py:26-93,248-256).
// A SET is an image of the batch (rows seg[i] .. seg[i+1]-1 of the token rows, in sGPN-ranked order) plus a DRAW, a list of image-local
// row indices (the script's `rand_ind`); one workgroup works on one set and no set needs another, so a batch times all its draws is one
// grid.  Three kernels: the best n_best rows of a draw by score (select), the distinct captions of a whole draw (distinct) and, over the
// selected rows, word / unigram / bigram counts, the novel count against a sorted training-caption index and the n_best sentence
// BLEU-4 values with their mean (best).  A caption is its tokens before the first id <= 0, trimmed like decode_sequence does when
// remove_bad_endings is on (caption.h's load_row); words are 16-bit ids, an n-gram one 64-bit key (caption.h's ngram_key), so
// every comparison is exact integer comparison -- the one hash (distinct) only pre-filters and is confirmed on the tokens.  Counts are
// integers (LDS integer adds: order-free), the BLEU arithmetic is fp64 in the reference's own order with no float atomics: equal inputs
// give equal bits.
#include "common.h"
#include "caption.h"

namespace {

constexpr int kMaxDraw = 1024;      // rows of one draw (the MRNN setting keeps up to 1000 sub-graphs per image)
constexpr int kRowWords = 64;       // words of a row (the decode's T)
constexpr int kMaxBest = 16;        // selected rows per set
constexpr int kCols = SUBGC_DIV_SEL;        // integer columns in front of the selection

__device__ __forceinline__ uint32_t order_key(float x) {         // a < b  <=>  order_key(a) < order_key(b); -0 counts as +0 (decode_sample.hip)
    uint32_t b = __float_as_uint(x);
    if (b == 0x80000000u) b = 0u;
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}

// Where a set lives: a = the image's first row, n = its rows, d0 = the draw's first slot, m = the draw's length (<= kMaxDraw; 0 for an
// image without rows).  Every field is clamped into what the buffers hold, whatever the index tensors say (debug bounds mode reports).
struct SetView { int a, n, d0, m; };
__device__ __forceinline__ SetView set_view(const int32_t* __restrict__ seg, int I, int rows, const int32_t* __restrict__ set_img,
                                            const int32_t* __restrict__ set_off, int n_draw, int s) {
    const int img = clampi(set_img[s], 0, I - 1);
    const int a = clampi(seg[img], 0, rows), b = clampi(seg[img + 1], a, rows);
    SetView v;
    v.a = a;
    v.n = b - a;
    v.d0 = 0;
    v.m = 0;
    if (set_off) {
        const int d0 = clampi(set_off[s], 0, n_draw), d1 = clampi(set_off[s + 1], d0, n_draw);
        v.d0 = d0;
        v.m = v.n > 0 ? (d1 - d0 < kMaxDraw ? d1 - d0 : kMaxDraw) : 0;
    }
    return v;
}

__device__ __forceinline__ uint64_t mix64(uint64_t x) {
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

// The best n_best rows of every draw by score, descending; among equal scores the row LATER in the draw first (the script's
// `rand_ind[np.argsort(score[rand_ind])[::-1][:5]]` with a stable ascending sort).  Rank by counting over the draw's keys in LDS.
__global__ __launch_bounds__(256) void select_kernel(const float* __restrict__ score, const int32_t* __restrict__ seg, int I, int rows,
                                                     const int32_t* __restrict__ set_img, const int32_t* __restrict__ set_off,
                                                     const int32_t* __restrict__ draw, int n_draw, int n_best, int32_t* __restrict__ out_i,
                                                     int ld_i) {
    __shared__ uint32_t keys[kMaxDraw];
    const int s = blockIdx.x, t = threadIdx.x;
    const SetView v = set_view(seg, I, rows, set_img, set_off, n_draw, s);
    for (int j = t; j < v.m; j += 256) keys[j] = order_key(score[v.a + clampi(draw[v.d0 + j], 0, v.n - 1)]);
    __syncthreads();
    int32_t* o = out_i + (int64_t)s * ld_i;
    const int nsel = v.m < n_best ? v.m : n_best;
    for (int j = t; j < v.m; j += 256) {
        const uint32_t k = keys[j];
        int rank = 0;
        for (int q = 0; q < v.m; ++q) {
            const uint32_t kq = keys[q];
            rank += (kq > k) || (kq == k && q > j);
        }
        if (rank < n_best) o[kCols + rank] = clampi(draw[v.d0 + j], 0, v.n - 1);
    }
    for (int q = nsel + t; q < n_best; q += 256) o[kCols + q] = -1;
    if (t == 0) o[SUBGC_DIV_SELECTED] = nsel;
}

// Drawn and distinct captions of every whole draw (metric 1, diversity_score.py:154-160).  A wave reads a row, its 64-bit hash (word and
// position mixed per lane, xor over the wave) and length go to LDS; a row counts when no EARLIER row of the draw has its hash, its
// length AND its tokens.
__global__ __launch_bounds__(256) void distinct_kernel(const void* __restrict__ tok, int tok64, int T, const uint8_t* __restrict__ bad, int bad_n,
                                                       const int32_t* __restrict__ seg, int I, int rows, const int32_t* __restrict__ set_img,
                                                       const int32_t* __restrict__ set_off, const int32_t* __restrict__ set_flags,
                                                       const int32_t* __restrict__ draw, int n_draw, int32_t* __restrict__ out_i, int ld_i) {
    __shared__ uint64_t hs[kMaxDraw];
    __shared__ int32_t rid[kMaxDraw];
    __shared__ uint8_t len[kMaxDraw];
    __shared__ int total;
    const int s = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int32_t* o = out_i + (int64_t)s * ld_i;
    if (!(set_flags[s] & SUBGC_DIV_WANT_DRAW)) {
        if (t == 0) o[SUBGC_DIV_DRAWN] = o[SUBGC_DIV_DISTINCT] = 0;
        return;
    }
    const SetView v = set_view(seg, I, rows, set_img, set_off, n_draw, s);
    if (t == 0) total = 0;
    for (int j = wave; j < v.m; j += 4) {
        const int r = v.a + clampi(draw[v.d0 + j], 0, v.n - 1);
        int64_t id;
        const int L = load_row(tok, tok64, T, r, bad, bad_n, lane, id);
        uint64_t h = lane < L ? mix64(((uint64_t)(lane + 1) << 16) | ((uint32_t)id & 0xffffu)) : 0ull;
        for (int d = 32; d > 0; d >>= 1) h ^= __shfl_xor((unsigned long long)h, d);
        if (lane == 0) {
            hs[j] = h;
            rid[j] = r;
            len[j] = (uint8_t)L;
        }
    }
    __syncthreads();
    int mine = 0;
    for (int j = t; j < v.m; j += 256) {
        const uint64_t h = hs[j];
        const int L = len[j], r = rid[j];
        bool first = true;
        for (int q = 0; q < j && first; ++q) {
            if (hs[q] != h || len[q] != L) continue;
            const int rq = rid[q];
            bool same = true;
            for (int p = 0; p < L && same; ++p) same = tok_at(tok, tok64, (int64_t)rq * T + p) == tok_at(tok, tok64, (int64_t)r * T + p);
            first = !same;
        }
        mine += first;
    }
    if (mine) atomicAdd(&total, mine);                                      // an integer count: the result does not depend on the order
    __syncthreads();
    if (t == 0) {
        o[SUBGC_DIV_DRAWN] = v.m;
        o[SUBGC_DIV_DISTINCT] = total;
    }
}

// a (La words in LDS) against caption c of the sorted index: < 0, 0, > 0 like a lexicographic compare of the id lists (a prefix sorts first)
__device__ __forceinline__ int cmp_caption(const uint32_t* a, int La, const int32_t* __restrict__ nv_off, const int32_t* __restrict__ nv_tok, int c) {
    const int b0 = nv_off[c];
    int Lb = nv_off[c + 1] - b0;
    if (Lb < 0) Lb = 0;
    const int n = La < Lb ? La : Lb;
    for (int p = 0; p < n; ++p) {
        const uint32_t x = a[p], y = (uint32_t)nv_tok[b0 + p] & 0xffffu;
        if (x != y) return x < y ? -1 : 1;
    }
    return La < Lb ? -1 : (La > Lb ? 1 : 0);
}

// The sum of n <= 16 contiguous doubles in np.mean's order (numpy's pairwise sum at this size): fewer than 8 in sequence; 8 and more:
// eight running lanes, combined as a tree, then the remainder in sequence
__device__ __forceinline__ double numpy_sum(const double* a, int n) {
    if (n < 8) {
        double res = 0.0;
        for (int i = 0; i < n; ++i) res += a[i];
        return res;
    }
    double r[8];
    for (int j = 0; j < 8; ++j) r[j] = a[j];
    int i = 8;
    for (; i < n - (n % 8); i += 8)
        for (int j = 0; j < 8; ++j) r[j] += a[i + j];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += a[i];
    return res;
}

// Everything over the selected rows of a set (metrics 3, 2, 4: diversity_score.py:96-108, :143-145, :67-79).
//   words / unigrams / bigrams: `sent.split(' ')` makes an empty caption ONE word, the empty word (id 0 here: never a real word);
//     bigrams are within a sentence; distinct = first occurrences, counted against the earlier entries of the flat list.
//   novel: the selected captions not found in the training-caption index (distinct id lists in lexicographic order, CSR): binary search
//     by comparing the id lists themselves.
//   BLEU-4: sentence q against the other selected sentences.  All n-grams (orders 1 .. 4, precook: `split()`, an empty caption has no
//     words) of all sentences lie in LDS; for the first occurrence of a key in q: min(its count in q, max over the others of their count)
//     goes to correct[q][order] (cook_refs / cook_test); then one thread per sentence spells bleu_scorer.py:248-256 in fp64.
__global__ __launch_bounds__(256) void best_kernel(const void* __restrict__ tok, int tok64, int T, const uint8_t* __restrict__ bad, int bad_n,
                                                   const int32_t* __restrict__ seg, int I, int rows, const int32_t* __restrict__ set_img,
                                                   const int32_t* __restrict__ set_flags, int n_best, const int32_t* __restrict__ nv_off,
                                                   const int32_t* __restrict__ nv_tok, int nv_n, int32_t* __restrict__ out_i, int ld_i,
                                                   double* __restrict__ out_d, int ld_d) {
    __shared__ uint32_t tk[kMaxBest * kRowWords];
    __shared__ uint32_t ul[kMaxBest * kRowWords];
    __shared__ uint32_t bl[kMaxBest * kRowWords];
    __shared__ uint64_t gk[kMaxBest * 4 * kRowWords];
    __shared__ int Ls[kMaxBest], woff[kMaxBest + 1], boff[kMaxBest + 1], goff[kMaxBest + 1];
    __shared__ int correct[kMaxBest * 4];
    __shared__ double b4[kMaxBest];
    __shared__ int n_uni, n_bi, n_novel;
    const int s = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int32_t* o = out_i + (int64_t)s * ld_i;
    double* od = out_d + (int64_t)s * ld_d;
    const int flags = set_flags[s];
    const SetView v = set_view(seg, I, rows, set_img, nullptr, 0, s);
    const int nsel = v.n > 0 ? clampi(o[SUBGC_DIV_SELECTED], 0, n_best) : 0;
    for (int q = wave; q < nsel; q += 4) {
        int64_t id;
        const int L = load_row(tok, tok64, T, v.a + clampi(o[kCols + q], 0, v.n - 1), bad, bad_n, lane, id);
        tk[q * kRowWords + lane] = lane < L ? (uint32_t)id & 0xffffu : 0u;
        if (lane == 0) Ls[q] = L;
    }
    if (t < kMaxBest * 4) correct[t] = 0;
    if (t == 0) n_uni = n_bi = n_novel = 0;
    __syncthreads();
    if (t == 0) {
        int w = 0, b = 0, g = 0;
        for (int q = 0; q < nsel; ++q) {
            const int L = Ls[q];
            woff[q] = w; boff[q] = b; goff[q] = g;
            w += L > 0 ? L : 1;
            b += L > 1 ? L - 1 : 0;
            for (int k = 0; k < 4; ++k) g += L > k ? L - k : 0;
        }
        woff[nsel] = w; boff[nsel] = b; goff[nsel] = g;
    }
    __syncthreads();
    for (int x = t; x < nsel * kRowWords; x += 256) {
        const int q = x >> 6, p = x & 63, L = Ls[q];
        const uint32_t* w = tk + q * kRowWords;
        if (p < L || (p == 0 && L == 0)) ul[woff[q] + p] = w[p];            // L == 0: w[0] = 0, the empty word
        if (p + 1 < L) bl[boff[q] + p] = (w[p] << 16) | w[p + 1];
        int base = goff[q];
        for (int k = 0; k < 4; ++k) {
            if (p + k < L) gk[base + p] = ngram_key(w, p, k);
            base += L > k ? L - k : 0;
        }
    }
    __syncthreads();
    const int nw = woff[nsel], nb = boff[nsel], ng = goff[nsel];
    if (flags & SUBGC_DIV_WANT_WORDS) {
        int u = 0, b = 0;
        for (int i = t; i < nw; i += 256) {
            const uint32_t x = ul[i];
            bool first = true;
            for (int j = 0; j < i && first; ++j) first = ul[j] != x;
            u += first;
        }
        for (int i = t; i < nb; i += 256) {
            const uint32_t x = bl[i];
            bool first = true;
            for (int j = 0; j < i && first; ++j) first = bl[j] != x;
            b += first;
        }
        if (u) atomicAdd(&n_uni, u);
        if (b) atomicAdd(&n_bi, b);
        if (nv_off && t < nsel) {
            const uint32_t* a = tk + t * kRowWords;
            const int La = Ls[t];
            int lo = 0, hi = nv_n;                                          // first caption that is not below a
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (cmp_caption(a, La, nv_off, nv_tok, mid) > 0) lo = mid + 1; else hi = mid;
            }
            if (!(lo < nv_n && cmp_caption(a, La, nv_off, nv_tok, lo) == 0)) atomicAdd(&n_novel, 1);
        }
    }
    const bool bleu = (flags & SUBGC_DIV_WANT_BLEU) && nsel >= 2;
    if (bleu) {
        for (int g = t; g < ng; g += 256) {
            int q = 0;
            while (goff[q + 1] <= g) ++q;
            const uint64_t key = gk[g];
            int before;
            const int c = count_key(gk, goff[q], goff[q + 1], g, before);
            if (before) continue;
            int mx = 0;
            for (int r = 0; r < nsel; ++r) {
                if (r == q) continue;
                int cr = 0;
                for (int j = goff[r]; j < goff[r + 1]; ++j) cr += gk[j] == key;
                mx = cr > mx ? cr : mx;
            }
            const int hit = c < mx ? c : mx;
            if (hit) atomicAdd(&correct[q * 4 + key_order(key)], hit);
        }
    }
    __syncthreads();
    if (t < n_best) {
        double val = 0.0;
        if (bleu && t < nsel) {
            const double small = 1e-9, tiny = 1e-15;
            const int testlen = Ls[t], reflen = closest_len(Ls, nsel, t, testlen);         // the other selected sentences are the references
            double prod = 1.0;
            for (int k = 0; k < 4; ++k) {
                const int guess = testlen - k > 0 ? testlen - k : 0;
                prod *= ((double)correct[t * 4 + k] + tiny) / ((double)guess + small);
            }
            val = pow(prod, 1.0 / 4.0);
            const double ratio = ((double)testlen + tiny) / ((double)reflen + small);
            if (ratio < 1.0) val *= exp(1.0 - 1.0 / ratio);
        }
        b4[t] = val;
        od[t] = val;
    }
    __syncthreads();
    if (t == 0) {
        const bool words = (flags & SUBGC_DIV_WANT_WORDS) != 0;
        o[SUBGC_DIV_WORDS] = words ? nw : 0;
        o[SUBGC_DIV_UNIGRAMS] = words ? n_uni : 0;
        o[SUBGC_DIV_BIGRAMS] = words ? n_bi : 0;
        o[SUBGC_DIV_NOVEL] = words && nv_off ? n_novel : 0;
        o[SUBGC_DIV_VALID] = bleu ? 1 : 0;
        od[n_best] = bleu ? numpy_sum(b4, nsel) / (double)nsel : 0.0;
    }
}

// debug bounds mode: block s walks the draw of set s (0 <= entry < rows of its image); out[0] = violations, out[1] = the smallest of
// (set << 20 | position)
__global__ __launch_bounds__(256) void check_draw_kernel(const int32_t* __restrict__ seg, int I, const int32_t* __restrict__ set_img,
                                                         const int32_t* __restrict__ set_off, const int32_t* __restrict__ draw, int n_draw,
                                                         unsigned long long* __restrict__ out) {
    const int s = blockIdx.x;
    const int img = clampi(set_img[s], 0, I - 1);
    const int n = seg[img + 1] - seg[img];
    const int d0 = clampi(set_off[s], 0, n_draw), d1 = clampi(set_off[s + 1], d0, n_draw);
    for (int j = threadIdx.x; j < d1 - d0; j += 256) {
        const int d = draw[d0 + j];
        if (d < 0 || d >= n) {
            atomicAdd(out, 1ull);
            atomicMin(out + 1, ((unsigned long long)s << 20) | (unsigned long long)(j < (1 << 20) - 1 ? j : (1 << 20) - 1));
        }
    }
}

// set_img, then seg, then -- where the launch reads one (set_off != NULL) -- the draws
int check_sets(const char* who, const int32_t* seg, int I, int rows, const int32_t* set_img, const int32_t* set_off, const int32_t* draw,
               int n_sets, int n_draw, hipStream_t s) {
    if (!subgc::debug_bounds() || subgc::capturing(s)) return SUBGC_OK;
    if (int rc = subgc::debug_check_range(set_img, 4, 1, n_sets, n_sets, 0, (int64_t)I - 1, -1, "diversity: set_img (image of every set)", s)) return rc;
    if (int rc = subgc::debug_check_mono(who, "seg (row boundaries of the images)", "image", seg, I, rows, s)) return rc;
    if (!set_off) return SUBGC_OK;
    unsigned long long res[2];
    if (int rc = subgc::run_check(s, [&](unsigned long long* out) {
            hipLaunchKernelGGL(check_draw_kernel, dim3(n_sets), dim3(256), 0, s, seg, I, set_img, set_off, draw, n_draw, out);
        }, res, who)) return rc;
    if (res[0] == 0) return SUBGC_OK;
    const int set = (int)(res[1] >> 20), pos = (int)(res[1] & 0xfffffull);
    int32_t off = 0, val = 0, img = 0, ab[2] = {0, 0};
    (void)hipMemcpy(&off, set_off + set, 4, hipMemcpyDeviceToHost);
    (void)hipMemcpy(&val, draw + off + pos, 4, hipMemcpyDeviceToHost);
    (void)hipMemcpy(&img, set_img + set, 4, hipMemcpyDeviceToHost);
    (void)hipMemcpy(ab, seg + img, sizeof(ab), hipMemcpyDeviceToHost);
    subgc::set_error("%s: draw (image-local row indices): %llu entries outside their image's rows (first at set %d, position %d: %d; image %d has "
                     "%d rows) [debug bounds mode]", who, res[0], set, pos, val, img, ab[1] - ab[0]);
    return SUBGC_EINVAL;
}

}  // namespace

SUBGC_API int subgc_diversity_select(const float* score, const int32_t* seg, int I, int rows, const int32_t* set_img, const int32_t* set_off,
                                     const int32_t* draw, int n_sets, int n_draw, int max_draw, int n_best, int32_t* out_i, int ld_i, void* stream) {
    SUBGC_REQUIRE(I >= 0 && rows >= 0 && n_sets >= 0 && n_draw >= 0, "diversity_select: I, rows, n_sets, n_draw >= 0");
    SUBGC_REQUIRE(n_best >= 2 && n_best <= kMaxBest, "diversity_select: 2 <= n_best <= %d (got %d)", kMaxBest, n_best);
    SUBGC_REQUIRE(max_draw >= 0 && max_draw <= kMaxDraw, "diversity_select: a draw holds at most %d rows (got max_draw = %d)", kMaxDraw, max_draw);
    SUBGC_REQUIRE(ld_i >= kCols + n_best, "diversity_select: ld_i shorter than %d + n_best", kCols);
    if (n_sets == 0) return SUBGC_OK;
    SUBGC_REQUIRE(I >= 1, "diversity_select: sets without an image");
    SUBGC_REQUIRE(seg && set_img && set_off && out_i && (rows == 0 || score) && (n_draw == 0 || draw), "diversity_select: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (int rc = check_sets("diversity_select", seg, I, rows, set_img, set_off, draw, n_sets, n_draw, s)) return rc;
    hipLaunchKernelGGL(select_kernel, dim3(n_sets), dim3(256), 0, s, score, seg, I, rows, set_img, set_off, draw, n_draw, n_best, out_i, ld_i);
    return subgc::check_launch("subgc_diversity_select");
}

SUBGC_API int subgc_diversity_distinct(const void* tok, int tok64, int T, const uint8_t* bad, int bad_n, const int32_t* seg, int I, int rows,
                                       const int32_t* set_img, const int32_t* set_off, const int32_t* set_flags, const int32_t* draw, int n_sets,
                                       int n_draw, int max_draw, int32_t* out_i, int ld_i, void* stream) {
    SUBGC_REQUIRE(I >= 0 && rows >= 0 && n_sets >= 0 && n_draw >= 0 && (!bad || bad_n >= 1),
                  "diversity_distinct: I, rows, n_sets, n_draw >= 0, bad_n >= 1 with a bad-endings table");
    SUBGC_REQUIRE(T >= 1 && T <= kRowWords, "diversity_distinct: token rows need 1 <= T <= %d (got %d)", kRowWords, T);
    SUBGC_REQUIRE(max_draw >= 0 && max_draw <= kMaxDraw, "diversity_distinct: a draw holds at most %d rows (got max_draw = %d)", kMaxDraw, max_draw);
    SUBGC_REQUIRE(ld_i >= kCols, "diversity_distinct: ld_i shorter than %d", kCols);
    if (n_sets == 0) return SUBGC_OK;
    SUBGC_REQUIRE(I >= 1, "diversity_distinct: sets without an image");
    SUBGC_REQUIRE(seg && set_img && set_off && set_flags && out_i && (rows == 0 || tok) && (n_draw == 0 || draw), "diversity_distinct: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (int rc = check_sets("diversity_distinct", seg, I, rows, set_img, set_off, draw, n_sets, n_draw, s)) return rc;
    hipLaunchKernelGGL(distinct_kernel, dim3(n_sets), dim3(256), 0, s, tok, tok64, T, bad, bad_n, seg, I, rows, set_img, set_off, set_flags, draw,
                       n_draw, out_i, ld_i);
    return subgc::check_launch("subgc_diversity_distinct");
}

SUBGC_API int subgc_diversity_best(const void* tok, int tok64, int T, const uint8_t* bad, int bad_n, const int32_t* seg, int I, int rows,
                                   const int32_t* set_img, const int32_t* set_flags, int n_sets, int n_best, const int32_t* nv_off,
                                   const int32_t* nv_tok, int nv_n, int32_t* out_i, int ld_i, double* out_d, int ld_d, void* stream) {
    SUBGC_REQUIRE(I >= 0 && rows >= 0 && n_sets >= 0 && nv_n >= 0 && (!bad || bad_n >= 1),
                  "diversity_best: I, rows, n_sets, nv_n >= 0, bad_n >= 1 with a bad-endings table");
    SUBGC_REQUIRE(T >= 1 && T <= kRowWords, "diversity_best: token rows need 1 <= T <= %d (got %d)", kRowWords, T);
    SUBGC_REQUIRE(n_best >= 2 && n_best <= kMaxBest, "diversity_best: 2 <= n_best <= %d (got %d)", kMaxBest, n_best);
    SUBGC_REQUIRE(ld_i >= kCols + n_best && ld_d >= n_best + 1, "diversity_best: ld_i shorter than %d + n_best or ld_d shorter than n_best + 1", kCols);
    SUBGC_REQUIRE(!nv_off || nv_n == 0 || nv_tok, "diversity_best: a training-caption index without its tokens");
    if (n_sets == 0) return SUBGC_OK;
    SUBGC_REQUIRE(I >= 1, "diversity_best: sets without an image");
    SUBGC_REQUIRE(seg && set_img && set_flags && out_i && out_d && (rows == 0 || tok), "diversity_best: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (int rc = check_sets("diversity_best", seg, I, rows, set_img, nullptr, nullptr, n_sets, 0, s)) return rc;
    hipLaunchKernelGGL(best_kernel, dim3(n_sets), dim3(256), 0, s, tok, tok64, T, bad, bad_n, seg, I, rows, set_img, set_flags, n_best, nv_off,
                       nv_tok, nv_n, out_i, ld_i, out_d, ld_d);
    return subgc::check_launch("subgc_diversity_best");
}
