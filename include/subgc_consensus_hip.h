/*
 * subgc_consensus_hip.h -- consensus re-ranking, method 'bleu', in libsubgc_hip.so (gfx950): the other half of `consensus_rerank`
 * (misc/consensus_reranking/concensus_reranking_utils/consensus_reranking.py:122-179), whose method 'cider' is subgc_consensus_cook /
 * _score / _rank of subgc_hip.h.
 *
 * The seventh public header.  subgc_hip.h is the model's drop-in boundary, subgc_metrics_hip.h, subgc_grounding_hip.h and
 * subgc_controllability_hip.h hold the evaluation scores, subgc_criterion_hip.h the label-smoothed loss, subgc_selfcritical_hip.h
 * self-critical training; all six stay as they are.  Same library, same contract as those: every function returns 0 (SUBGC_OK) or a
 * negative SUBGC_E* code with the text in subgc_last_error(), never allocates device memory and never synchronises the device (debug
 * bounds mode excepted, subgc_debug_bounds), enqueues on `stream` (a hipStream_t passed as void*), all pointers are BORROWED device
 * pointers, outputs are caller-allocated, everything is per call and there is no global state.  subgc_version() does not change with
 * this header.
 *
 * What is replaced:
 *   concensus_reranking_utils/bleu_score_util.py:15-61    calculate_bleu_sentence: the m-RNN sentence-level n-gram F-score (NOT the COCO
 *                                                         BLEU of subgc_accuracy_rows), two Counters of word tuples per order and pair;
 *   concensus_reranking_utils/consensus_reranking.py:152-169   the loops over images, candidates and neighbour captions around it, the
 *                                                         descending sort and the sum of the m largest pair scores;
 *   concensus_reranking_utils/conf_cr.py:45-48            k_bleu = 60, m_bleu = 175, fpr_bleu = 1.0, bleu_ngram = 4: arguments here.
 * The order of the sums (consensus_reranking.py:172) is subgc_consensus_rank of subgc_hip.h, unchanged.
 *
 * Words are 16-bit ids (1 .. 65535; 0 never inside a sentence) and an n-gram of order 1 .. 4 is ONE 64-bit key (word j in bits
 * 63-16j .. 48-16j), exactly as in subgc_consensus_cook: matching is exact integer comparison, counts are integers, there is no hashing
 * and no float atomic; equal inputs give equal bits.
 *
 * The pair score of candidate words t and neighbour caption words r, with n = the n-gram order and fpr:
 *   n > len(t) or n > len(r):  0 (bleu_score_util.py:27 tests n, not the order at hand: a 3-word sentence scores 0 with n = 4);
 *   else for o = 1 .. n:  acc = sum over the distinct o-grams g of t of min(count_t[g], count_r[g]);  acc == 0: f_o = 0;  else
 *       pre = acc / (len(t) - o + 1);  rec = acc / (len(r) - o + 1);  f_o = ((fpr + 1) * pre * rec) / (rec + fpr * pre)   (:48-50)
 *     in fp64, this operation order, one IEEE rounding per operation (no contraction, correctly rounded division);
 *   score = (((f_1 + f_2) + f_3) + f_4) / (double)n: the plain left-to-right sum where the reference's math.fsum (:58) rounds the exact
 *     sum once -- the two differ by at most (n + 2) u / (1 - (n + 2) u), u = 2^-53, of the score.
 */
#ifndef SUBGC_CONSENSUS_HIP_H
#define SUBGC_CONSENSUS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Sentences -> their distinct n-grams of orders 1 .. 4 with counts: what `Counter(ngrams(sentence, i + 1))` (bleu_score_util.py:33-34)
 * holds for every order at once, built once per sentence instead of once per pair.
 * Sentence s of S: CSR mode (woff != NULL): words tok[woff[s] .. woff[s + 1]), all non-zero, at most max_words <= 256 of them; row
 * mode (woff == NULL): row s of tok [S, T], T <= 64: the ids before the first id <= 0, at most row_len[s] (row_len NULL or negative:
 * no cap), minus -- bad != NULL -- its trailing words w with bad[w] != 0 unless every word is one (misc/utils.py:74-80).  tok is int32
 * or int64 (tok64).  These are subgc_consensus_cook's sentence arguments and rules.
 * The list of sentence s lands at keys / counts [4 * first word index ...) (first word index = woff[s] or s * T): keys ascending, every
 * key once, counts[.] = how often the n-gram occurs in the sentence; cnt[s] = the number of keys (<= 4 L - 6 for L >= 4 words),
 * wlen[s] = the number of words L.  keys / counts hold 4 * (number of words of tok) entries.  One wave per sentence; no fp arithmetic. */
int subgc_consensus_bleu_cook(const void* tok, int tok64, const int32_t* woff, int T, const int32_t* row_len, const uint8_t* bad,
                              int bad_n, int S, int max_words, uint64_t* keys, int32_t* counts, int32_t* cnt, int32_t* wlen,
                              void* stream);

/* sim[row] = the sum of the m largest pair scores (all of them where there are fewer) of candidate `row` against the captions of its
 * image's first k neighbour images, added in descending order as `b_s_arr.sort(reverse=True); sum(b_s_arr[:m])` adds them
 * (consensus_reranking.py:155-169 with bleu_score_util.py:15-61 as the pair score; the contract is in the head of this file).
 * Addressing is subgc_consensus_score's: image i of I owns the candidate rows seg[i] .. seg[i + 1] - 1 (at most max_cand; top_k > 0:
 * only its first top_k); its neighbours are nn[i * nn_ld + 0 .. k), k <= 256, indices into the corpus of n_img images, image j owning
 * the captions cap_off[j] .. cap_off[j + 1] - 1 of n_caps; caption s owns the cooked list at 4 * nwoff[s]; at most max_caps <= 2048
 * neighbour captions per image are scored.  c*: the candidates' lists from a row-mode cook of [rows, T] (list stride 4 T); n*: the
 * corpus's from a CSR cook over nwoff.  1 <= n <= 4; fpr finite and >= 0 (fpr = 0: f = pre); m >= 1; other values are SUBGC_EINVAL with
 * the value in the text.  pair_out (may be NULL): pair_out[row * pair_ld + j] = the score against the j-th neighbour caption in
 * neighbour order.  A neighbour index outside [0, n_img - 1] is clamped; debug bounds mode reports it instead.
 * One workgroup per (candidate, image), one thread per neighbour caption and pass, one merge walk over two ascending lists per pair. */
int subgc_consensus_bleu_score(const uint64_t* ckeys, const int32_t* ccounts, const int32_t* ccnt, const int32_t* cwlen, int T,
                               const int32_t* seg, int I, int max_cand, int top_k, const int32_t* nn, int nn_ld, int k,
                               const int32_t* cap_off, int n_img, int n_caps, const int32_t* nwoff, const uint64_t* nkeys,
                               const int32_t* ncounts, const int32_t* ncnt, const int32_t* nwlen, int n, double fpr, int m, int max_caps,
                               double* sim, double* pair_out, int64_t pair_ld, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SUBGC_CONSENSUS_HIP_H */
