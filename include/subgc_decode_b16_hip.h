/*
 * subgc_decode_b16_hip.h -- the two pointwise kernels of the bf16-batched decode step in libsubgc_hip.so (gfx950): the LSTM cell that
 * keeps c in fp32 and writes h as bf16 straight into the operands of the next products, and the beam-search state fork for that
 * mixed-type state.
 *
 * The eleventh public header.  subgc_hip.h is the model's drop-in boundary; the nine headers after it (metrics, grounding,
 * controllability, criterion, selfcritical, consensus, forced, control_input, beam_att) stay as they are, and so do subgc_lstm_fwd,
 * subgc_token_rows_f32 and subgc_gather_rows_multi (signatures and bits).  Same library, same contract as those: every function returns
 * 0 (SUBGC_OK) or a negative SUBGC_E* code with the text in subgc_last_error(), never allocates device memory and never synchronises
 * the device, enqueues on `stream` (a hipStream_t passed as void*) and can be captured into a hipGraph, all pointers are BORROWED
 * device pointers, outputs are caller-allocated, everything is per call and there is no global state.  subgc_version() does not change
 * with this header.
 *
 * What is replaced: the pointwise half of AttModel.py:405-427 (TopDownCore.forward: two nn.LSTMCell updates around the attention) for
 * a decode of more than 32 rows whose products run on bf16 operands (subgc_gemm_bf16), and the state re-arrangement of
 * CaptionModel.py:76-90 for that state.  Cell state, pre-activations and the gate arithmetic are fp32; only h is stored as bf16
 * (round-to-nearest-even, once), because its only readers are products.  No float atomics, no LDS.
 * Out of scope: dropout (decode only), saved gates (no backward), bf16 cell state.
 */
#ifndef SUBGC_DECODE_B16_HIP_H
#define SUBGC_DECODE_B16_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SUBGC_DECODE_B16_MAX_DST 3      /* destinations of h in one cell launch */

/* nn.LSTMCell pointwise, gate order i,f,g,o (AttModel.py:413 att_lstm, :423 lang_lstm), on pre-activations a bf16 product left in fp32:
 *   pre[r, :] = g0[r, :] + (table ? table[clamp(tok[r]), :] : 0) + g2[r, :] + b0 + b1        (each of table / g2 / b0 / b1 may be NULL)
 *   c[r]      = sig(f) c_prev[r] + sig(i) tanh(g)        fp32 [S, R], contiguous; c_prev must not be c (the host double-buffers)
 *   h[r]      = sig(o) tanh(c[r])                        rounded ONCE to bf16 (nearest-even) and written to hd0 and, when not NULL,
 *                                                        hd1 and hd2: [S, R] bf16 views with their own row pitches ldh0..2 (elements)
 * g0 [S, 4R] (ld0), g2 [S, 4R] (ld2), b0 / b1 [4R].  table [vocab_rows, 4R] (ldt) is the x->gates table of the attention LSTM
 * (relu(Emb) . W_ih[:, 2R:]^T, AttModel.py:332 feeding :409-411) gathered by tok int64 [S] (tok_stride apart), clamped to
 * [0, vocab_rows) exactly as subgc_token_rows_f32 clamps; the language LSTM passes table = tok = NULL.
 * Activations are subgc_lstm_fwd's (the same expressions in the same order), so c equals that kernel's c on equal pre-activations.
 * One lane owns 8 consecutive hidden units of one row: float4 reads, one 16-byte store per destination.
 * Refused (SUBGC_EINVAL, the number in the text): S < 1, R % 8 != 0, more than SUBGC_DECODE_B16_MAX_DST destinations or none
 * (n_dst counts hd0..), a destination that is not 16-byte aligned or whose pitch is not a multiple of 8 or below R, an fp32 operand
 * that is not 16-byte aligned or whose pitch is not a multiple of 4 or below 4R, a table without tokens or vocab_rows < 1.             */
int subgc_decode_cell_b16(const float* g0, int64_t ld0, const float* table, int64_t ldt, const int64_t* tok, int64_t tok_stride,
                          int vocab_rows, const float* g2, int64_t ld2, const float* b0, const float* b1, const float* c_prev, float* c,
                          uint16_t* hd0, int64_t ldh0, uint16_t* hd1, int64_t ldh1, uint16_t* hd2, int64_t ldh2, int n_dst, int S, int R,
                          void* stream);

/* CaptionModel.py:76-90 ("rearrange recurrent states") for the bf16-batched state, one launch:
 *   db0[m, :cb0] = sb0[src[m], :cb0],  db1[m, :cb1] = sb1[src[m], :cb1]      bf16 (row pitches lds* / ldd* in elements)
 *   df0[m, :cf0] = sf0[src[m], :cf0],  df1[m, :cf1] = sf1[src[m], :cf1]      fp32
 * for m < S; src int32 [S], entries clamped to [0, S) in the kernel (the host refuses the ones it knows).  Rows move as 16-byte
 * pieces: cb* % 8 == 0, cf* % 4 == 0, pitches multiples of the same, every pointer 16-byte aligned -- anything else is refused with
 * the number in the text.  No destination may overlap a source (not checked: the caller keeps two buffer sets, as DecodeState.reorder
 * does).  One workgroup per (row, tensor).                                                                                              */
int subgc_decode_fork_b16(const uint16_t* sb0, int64_t lds0, uint16_t* db0, int64_t ldd0, int cb0, const uint16_t* sb1, int64_t lds1,
                          uint16_t* db1, int64_t ldd1, int cb1, const float* sf0, int64_t ldsf0, float* df0, int64_t lddf0, int cf0,
                          const float* sf1, int64_t ldsf1, float* df1, int64_t lddf1, int cf1, const int32_t* src, int S, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SUBGC_DECODE_B16_HIP_H */
