/*
 * subgc_metrics_hip.h -- the evaluation-metric entry points of libsubgc_hip.so (gfx950): the accuracy scores of a decode batch.
 *
 * subgc_hip.h is the model's drop-in boundary and stays as it is; the metrics the reference computes AFTER the model has spoken are a
 * surface of their own and live here.  Same library, same contract as subgc_hip.h: every function returns 0 (SUBGC_OK) or a negative
 * SUBGC_E* code with the text in subgc_last_error(), never allocates device memory and never synchronises the device (debug bounds mode
 * excepted, subgc_debug_bounds), enqueues on `stream` (a hipStream_t passed as void*), all pointers are BORROWED device pointers,
 * outputs are caller-allocated, and there is no global state.  subgc_version() does not change with this header.
 *
 * What is replaced: `test.py --only_sent_eval 1 --oracle_num N` -> eval_split (misc/eval_utils.py:176-189) -> language_eval and
 * cal_bleu (misc/sentence_utils.py:28-53, :56-125), which run the COCO scorers once per caption position:
 *   BLEU    misc/coco-caption/pycocoevalcap/bleu/bleu_scorer.py:26-93 (precook, cook_refs, cook_test), :208-256 (compute_score)
 *   CIDEr   misc/coco-caption/pycocoevalcap/cider/cider_scorer.py:95-184 (compute_doc_freq, counts2vec, sim, compute_cider)
 *   ROUGE-L misc/coco-caption/pycocoevalcap/rouge/rouge.py:15-77 (my_lcs, calc_score)
 * Words are 16-bit ids (1 .. 65535; 0 = no word) and an n-gram of order 1 .. 4 is one 64-bit key (word j in bits 63-16j .. 48-16j), as in
 * the consensus family of subgc_hip.h: every match is an exact integer comparison.  All arithmetic is fp64 in an order fixed by the
 * inputs, without float atomics and without FMA contraction: equal inputs give equal bits.
 */
#ifndef SUBGC_METRICS_HIP_H
#define SUBGC_METRICS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* columns of a row's integer record (bleu_scorer.py:68-93: cook_test's result with the closest reference length) */
#define SUBGC_ACC_TESTLEN 0
#define SUBGC_ACC_REFLEN 1
#define SUBGC_ACC_GUESS 2      /* .. 5: max(0, testlen - k) */
#define SUBGC_ACC_CORRECT 6    /* .. 9: clipped matches of order k + 1 */
#define SUBGC_ACC_ROW_INT 10
/* columns of a row's fp64 record */
#define SUBGC_ACC_BLEU 0       /* .. 3: sentence BLEU-1 .. 4 (bleu_scorer.py:242-252) */
#define SUBGC_ACC_CIDER 4      /* cider_scorer.py:166-180 */
#define SUBGC_ACC_ROUGE 5      /* rouge.py:47-77 */
#define SUBGC_ACC_ROW_F64 6
/* columns of an image's integer record */
#define SUBGC_ACC_IMG_ROWS 0       /* min(n_i, oracle_num): the rows the oracle looked at */
#define SUBGC_ACC_IMG_TOP1 1       /* the top-1 row (image-local) */
#define SUBGC_ACC_IMG_TOP1_MAT 2   /* .. 11: its integer record */
#define SUBGC_ACC_IMG_PICK 12      /* .. 15: the row of the first maximum of sentence BLEU-1 .. 4 */
#define SUBGC_ACC_IMG_PICK_MAT 16  /* .. 55: the integer records of the four picks */
#define SUBGC_ACC_IMG_INT 56
/* columns of an image's fp64 record */
#define SUBGC_ACC_IMG_TOP1_VAL 0   /* .. 5: the fp64 record of the top-1 row */
#define SUBGC_ACC_IMG_BEST 6       /* .. 9: the largest sentence BLEU-1 .. 4; 10: the largest CIDEr; 11: the largest ROUGE-L */
#define SUBGC_ACC_IMG_F64 12

#define SUBGC_ACC_MAX_REFS 32        /* reference captions of an image */
#define SUBGC_ACC_MAX_REF_WORDS 256  /* words of a reference caption */

/* subgc_accuracy_rows: BLEU material and sentence BLEU-1 .. 4, CIDEr and ROUGE-L of every candidate row of a decode batch against the
 * reference captions of its image (what ONE pass of language_eval's loop, sentence_utils.py:84-107, computes for one caption position --
 * here for all positions at once).
 *   tok [rows, T] int32 (tok64 = 0) or int64 (1), T <= 64: a caption is the ids before the first id <= 0, minus its trailing words w
 *     with bad[w] != 0 unless every word is one (bad NULL: no trimming; misc/utils.py:74-80, the rule of subgc_consensus_cook).
 *   seg [I + 1]: batch image i owns rows seg[i] .. seg[i+1]-1; img_ref [I]: its image in the reference tables (0 .. n_ref - 1).
 *   ckeys / cw / ccnt / clen / cnorm: the rows cooked by subgc_consensus_cook in row mode with this T, `bad` and the REFERENCE tables'
 *     log df and ref_len (cider_scorer.py:104-123 for the candidate).
 *   Reference tables: image j owns captions cap_off[j] .. cap_off[j+1]-1 (1 .. SUBGC_ACC_MAX_REFS of them), caption s the words
 *     rtok[rwoff[s] .. rwoff[s+1]) (<= SUBGC_ACC_MAX_REF_WORDS; rouge.py:61-67 reads these) and the cooked list rkeys / rw
 *     [4 * rwoff[s] ...] with rcnt / rlen / rnorm [s] (subgc_consensus_cook in CSR mode); image j's distinct n-gram keys in ascending
 *     order with the largest count over its captions are bkeys / bmax [boff[j] .. boff[j+1]) (cook_refs' maxcounts, bleu_scorer.py:45-52).
 *   gauss [n_gauss]: the length factor by |difference of the bigram counts| (cider_scorer.py:148-160); beta2 = beta ** 2 of rouge.py:46.
 *   out_i [rows, ld_i >= SUBGC_ACC_ROW_INT], out_d [rows, ld_d >= SUBGC_ACC_ROW_F64].
 * ROUGE-L splits at single spaces (rouge.py:59-63): an empty caption is the one-word caption of the empty word (id 0) there, for
 * candidates and references alike.  Every index is clamped into its buffer; debug bounds mode checks seg (monotone inside [0, rows]),
 * img_ref and the three CSR offset tables first and reports instead.                                                                */
int subgc_accuracy_rows(const void* tok, int tok64, int T, const uint8_t* bad, int bad_n, int rows, const int32_t* seg, int I,
                        const int32_t* img_ref, int n_ref, const uint64_t* ckeys, const double* cw, const int32_t* ccnt,
                        const int32_t* clen, const double* cnorm, const int32_t* cap_off, int n_caps, const int32_t* rwoff,
                        const int32_t* rtok, int n_words, const uint64_t* rkeys, const double* rw, const int32_t* rcnt,
                        const int32_t* rlen, const double* rnorm, const int32_t* boff, const uint64_t* bkeys, const int32_t* bmax,
                        int n_bkeys, const double* gauss, int n_gauss, double beta2, int32_t* out_i, int ld_i, double* out_d, int ld_d,
                        void* stream);

/* subgc_accuracy_oracle (sentence_utils.py:108-125 with cal_bleu, :28-53; the padding of eval_utils.py:183-187 changes no maximum and no
 * first arg-max): per image, over its first min(n_i, oracle_num) rows of the records subgc_accuracy_rows wrote, the row of the FIRST
 * maximum of each sentence BLEU order (np.argmax; compared in fp64) with that row's integer record, the largest CIDEr and the largest
 * ROUGE-L; and the same records of the top-1 row: first[i] (image-local, clamped; NULL: row 0).  An image without rows gets zeros.
 *   img_i [I, ld_ii >= SUBGC_ACC_IMG_INT], img_d [I, ld_id >= SUBGC_ACC_IMG_F64].  Corpus numbers are formed on the host.              */
int subgc_accuracy_oracle(const int32_t* row_i, int ld_i, const double* row_d, int ld_d, int rows, const int32_t* seg, int I,
                          int oracle_num, const int32_t* first, int32_t* img_i, int ld_ii, double* img_d, int ld_id, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SUBGC_METRICS_HIP_H */
