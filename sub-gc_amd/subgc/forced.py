"""Forced decode on the device: the decoder FOLLOWS given tokens (include/subgc_forced_hip.h).

What it gives: the per-token log-probabilities and the log-likelihood / perplexity of any caption under the model without the training
graph (`score_captions`: validation, rescoring of candidates), and the teacher-forced attention of any (sub-graph, sentence) pair
(`forced_decode(return_att=True)`), from which `eval_glue.ground_gt_images` forms the grounding accuracy on ground-truth sentences
(subgc.grounding_gt).  The loop is `sampling.decode`'s batched `DecodeState` loop with `subgc_forced_pick` in the place of
`subgc_decode_pick`, then `subgc_forced_finish`; only C-ABI launches are issued.  `sampling._forced_pick` and the `forced=` hook of
`_sample` stay what they are: torch-level test plumbing.

Rows: candidate j of image i (counterpart 0 of the loader's five copies) is decoded along tokens[i][j] -- every candidate in INPUT order,
no NMS and no sorting (the `sct` row rule of `select_subgraphs`, whatever `model.sct` says); an image may bring fewer token rows than it
has candidates (its first rows are decoded), never more.  A Full-GC model repeats the image's full-graph row once per token row.  Which
sub-graph a sentence is decoded on is the caller's choice.  Step j is fed word j - 1 (<bos> at step 0) and scores word j, so attention
row j belongs to word j; a row is live up to and including its first 0 (the end token), which is scored as LanguageModelCriterion scores
it.  Tf comes from the token rows (<= 64), not from `model.seq_length`.
"""
from __future__ import annotations

import numpy as np
import torch

from . import functions as F_
from . import ops
from ._lib import SubgcError, call_forced
from .models import sampling

MAX_V = 16384            # SUBGC_FORCED_MAX_V
MAX_T = 64               # SUBGC_FORCED_MAX_T


def forced_pick(logits, forced, t, seq, seqlp, next_tok, unfinished, n_unf, prev_count=None, raw=False):
    """One forced step (subgc_forced_pick): row r files forced[r, t]; the bookkeeping is decode_pick's."""
    n, V = logits.shape
    if forced.dim() != 2 or forced.size(0) != n or (forced.size(1) > 1 and forced.stride(1) != 1):
        raise SubgcError(f"forced_pick: forced tokens [n = {n}, Tf] with unit inner stride, got {tuple(forced.shape)} / {forced.stride()}")
    call_forced("subgc_forced_pick", ops._ptr(logits, torch.float32), ops.ld(logits), n, V, ops._ptr(forced, torch.int64), max(forced.stride(0), forced.size(1)),
                forced.size(1), int(t), ops._ptr(seq, torch.int64), ops._ptr(seqlp, torch.float32), seq.size(1), ops._ptr(next_tok, torch.int64),
                ops._ptr(unfinished, torch.int32), ops._ptr(n_unf, torch.int32), ops._ptr(prev_count, torch.int32), int(raw), ops._stream())


def forced_finish(seq, seqlp, Tf=None, ll=None, n_tok=None):
    """-> (ll fp64 [n], n_tok int32 [n]) of the rows subgc_forced_pick filed (subgc_forced_finish)."""
    n, T = seq.shape
    if not (seq.is_contiguous() and seqlp.is_contiguous()) or seqlp.shape != seq.shape:
        raise SubgcError("forced_finish: contiguous seq / seqlp of one shape")
    ll = torch.empty(n, device=seq.device, dtype=torch.float64) if ll is None else ll
    n_tok = torch.empty(n, device=seq.device, dtype=torch.int32) if n_tok is None else n_tok
    call_forced("subgc_forced_finish", ops._ptr(seq, torch.int64), ops._ptr(seqlp, torch.float32), T, n, T if Tf is None else int(Tf),
                ops._ptr(ll, torch.float64), ops._ptr(n_tok, torch.int32), ops._stream())
    return ll, n_tok


def _token_rows(tokens, n_images):
    """tokens: per image an int array / tensor [rows_i, Tf_i] -> (host int64 [rows, Tf] zero-padded, rows per image)."""
    if len(tokens) != n_images:
        raise SubgcError(f"forced_decode: {len(tokens)} token arrays for {n_images} images")
    arrs = []
    for i, t in enumerate(tokens):
        a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
        if a.ndim != 2 or (a.size and not np.issubdtype(a.dtype, np.integer)):
            raise SubgcError(f"forced_decode: image {i}: integer token rows [rows, Tf], got {a.dtype} {a.shape}")
        arrs.append(a.astype(np.int64))
    Tf = max([a.shape[1] for a in arrs] + [0])
    if Tf > MAX_T:
        raise SubgcError(f"forced_decode: token rows of {Tf} steps; the limit is {MAX_T}")
    if Tf < 1:
        raise SubgcError("forced_decode: token rows need at least one column")
    out = np.zeros((sum(a.shape[0] for a in arrs), Tf), np.int64)
    r = 0
    for a in arrs:
        out[r:r + a.shape[0], :a.shape[1]] = a
        r += a.shape[0]
    return out, [a.shape[0] for a in arrs]


def _candidate_rows(m, X2, N, rows_in, counts):
    """The first counts[i] candidate sub-graphs of every image in input order -> (fc, lens, idx, img): `select_subgraphs`' sct branch
    with the row list uploaded instead of built by torch."""
    dev, L = X2.device, m.GCN_dim
    fr = sampling.score_candidates(m, X2, N, rows_in)
    for i, (c, s) in enumerate(zip(counts, fr.sizes)):
        if c > s:
            raise SubgcError(f"forced_decode: image {i} brings {c} token rows and has {s} candidate sub-graphs")
    glob = ops.upload([int(fr.offs[i]) + j for i, c in enumerate(counts) for j in range(c)], torch.int64, dev)
    n = glob.numel()
    e = lambda *sh, dt=torch.float32: torch.empty(*sh, device=dev, dtype=dt)
    fc, ro, h = e(n, 2 * L), e(n, 2 * L), e(n, m.att_hid_size)
    lens_g, idx_g, img_g = e(n, dt=torch.int32), e(n, fr.idx.size(1), dt=torch.int64), e(n, dt=torch.int32)
    idx = fr.idx if fr.idx.is_contiguous() else fr.idx.contiguous()
    ops.take_rows([(fr.read_out, ro), (fr.lens_i, lens_g), (idx, idx_g), (fr.img, img_g)], glob)
    ops.gemm(ro, m.P("gpn_layer.read_out_proj.0.weight"), h, tb=True, bias=m.P("gpn_layer.read_out_proj.0.bias"))
    ops.gemm(h, m.P("gpn_layer.read_out_proj.1.weight"), fc, tb=True, bias=m.P("gpn_layer.read_out_proj.1.bias"))
    return fc, lens_g, idx_g, img_g


def _full_graph_rows(m, X2, N, rows_in, counts):
    """Full-GC: the image's one full-graph row, repeated once per token row."""
    dev = X2.device
    w = sampling.full_graph_rows(m, X2, N, rows_in).whole
    glob = ops.upload([i for i, c in enumerate(counts) for _ in range(c)], torch.int64, dev)
    n = glob.numel()
    e = lambda *sh, dt=torch.float32: torch.empty(*sh, device=dev, dtype=dt)
    fc, lens_g, idx_g, img_g = e(n, w["fc"].size(1)), e(n, dt=torch.int32), e(n, w["idx"].size(1), dt=torch.int64), e(n, dt=torch.int32)
    ops.take_rows([(w["fc"], fc), (w["lens"], lens_g), (w["idx"], idx_g), (w["img"], img_g)], glob)
    return fc, lens_g, idx_g, img_g


@torch.no_grad()
def forced_decode(model, images, tokens, return_att=False, batch_out=None):
    """Decode along given tokens.  images: list of dicts with the test loader's keys (`sample_images`); tokens[i]: int [rows_i, Tf_i]
    (array or tensor; shorter rows are zero-padded to the longest).  -> dict of DEVICE tensors over all rows in image order:
      seq int64 [rows, Tf] (the tokens of the live steps), seqlp fp32 [rows, Tf] (their log-probabilities, 0 behind the end token),
      ll fp64 [rows] / n_tok int32 [rows] (subgc_forced_finish), tokens int64 [rows, Tf] (the forced rows as uploaded),
      idx int64 [rows, N] / lens int32 [rows] (node lists), img int32 [rows], bounds (python list of the images' row boundaries), rows, Tf
      and with return_att AL fp32 [Tf, rows, N]: the attention of step j = word j (else None).
    `batch_out` (a dict): receives the same entries."""
    tok_host, counts = _token_rows(tokens, len(images))
    rows, Tf = tok_host.shape
    bounds = [0]
    for c in counts:
        bounds.append(bounds[-1] + c)
    out = dict(rows=rows, Tf=Tf, bounds=bounds, AL=None)
    was_training = model.training
    model.eval()
    try:
        if rows:
            att, obj, pred, rel = ops.stack_first([[im[k] for im in images] for k in ("att_feats", "obj_dist", "pred_dist", "rel_ind")])
            I, N, _ = att.shape
            dev = att.device
            X2 = model._encode(att, obj, pred, rel).reshape(I * N, model.GCN_dim).contiguous()
            rows_in = [(i, im["gpn_obj_ind"], im["att_masks"], im["gpn_pool_mtx"]) for i, im in enumerate(images)]
            fc, lens, idx, img = (_candidate_rows if model.gpn else _full_graph_rows)(model, X2, N, rows_in, counts)
            tok = ops.upload(tok_host.ravel(), torch.int64, dev).view(rows, Tf)
            P = model._decoder_params()
            pr = F_.Prepared(fc, X2, lens, idx, img, N, P, None, None, 1.0)
            st = F_.DecodeState(pr, P, N, return_att, xt_table=model.xt_gates_table(), fuse_lstm=True, snapshots=model.decode_snapshots(),
                                W16=model.decode_w16(), b16_batched=model.decode_b16_on())
            if st.V1 > MAX_V:
                raise SubgcError(f"forced_decode: {st.V1} logit columns; the limit is {MAX_V}")
            z = lambda *s, dt=torch.float32: ops.zero_(torch.empty(*s, device=dev, dtype=dt))
            seq, seqlp, it = z(rows, Tf, dt=torch.long), z(rows, Tf), z(rows, dt=torch.long)
            unfinished, counts_d = z(rows, dt=torch.int32), z(Tf, dt=torch.int32)
            AL = z(Tf, rows, N) if return_att else None
            for t in range(Tf):
                logits = st.step(it, AL[t] if return_att else None, normalize=False)
                forced_pick(logits, tok, t, seq, seqlp, it, unfinished, counts_d[t:t + 1], counts_d[t - 1:t] if t > 0 else None, raw=True)
            ll, n_tok = forced_finish(seq, seqlp, Tf)
            out.update(seq=seq, seqlp=seqlp, ll=ll, n_tok=n_tok, tokens=tok, idx=idx, lens=lens, img=img, AL=AL, N=N)
    finally:
        model.train(was_training)
    if batch_out is not None:
        batch_out.update(out)
    return out


def perplexity(ll, n_tok):
    """exp(-ll / n_tok) per caption (fp64, host); a caption without tokens gives NaN."""
    ll, n_tok = np.asarray(ll, np.float64), np.asarray(n_tok, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.exp(-ll / n_tok)


@torch.no_grad()
def score_captions(model, images, tokens):
    """The log-likelihood of given captions under the model -> host dict: ll fp64 [rows], n_tok int32 [rows], perplexity fp64 [rows],
    seqlp fp32 [rows, Tf], bounds; `mean_nll` = -sum(ll) / sum(n_tok), LanguageModelCriterion's masked mean over these rows."""
    d = forced_decode(model, images, tokens)
    if d["rows"] == 0:
        e = np.zeros(0)
        return dict(ll=e, n_tok=e.astype(np.int32), perplexity=e, seqlp=np.zeros((0, d["Tf"]), np.float32), bounds=d["bounds"], mean_nll=float("nan"))
    ll, n_tok = d["ll"].cpu().numpy(), d["n_tok"].cpu().numpy()
    return dict(ll=ll, n_tok=n_tok, perplexity=perplexity(ll, n_tok), seqlp=d["seqlp"].cpu().numpy(), bounds=d["bounds"],
                mean_nll=float(-ll.sum() / n_tok.sum()))
