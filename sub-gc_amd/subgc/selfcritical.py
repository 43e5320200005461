"""Self-critical sequence training (SCST) on the device: the rollout, its reward and the references the reward is scored against.

The reference carries the plumbing of this objective and never runs it: `RewardCriterion` (misc/utils.py:89-109), `--self_critical_after`
(opts.py:66), `--cached_tokens` (opts.py:24), `--cider_reward_weight` / `--bleu_reward_weight` (opts.py:149-152), the `gts` list the loader
builds for every batch (dataloaders/dataloader.py:209-213) and the `gts` / `gt_indices` arguments of LossWrapper.forward (train.py:151,
models/loss_wrapper.py:14), which ignores both.  In the project it descends from these pieces are REINFORCE on the decoder with the greedy
caption's score as the baseline: reward = score(sampled caption) - score(greedy caption), loss = RewardCriterion(log p(sampled), reward).

The decoder's state depends on the sampled tokens only as inputs, so "sample with gradient" = "sample without gradient, then teacher-force
the sampled tokens": `rollout` runs ONE batched decode loop over the training batch's sub-graphs twice (sampled half, greedy half;
`subgc_sc_pick`), `SelfCriticalReward` scores both halves with the accuracy kernels (`subgc_accuracy_rows`: sentence BLEU-4 and CIDEr in
fp64) and forms the reward (`subgc_sc_reward`), and AttModel._forward replays the sampled tokens through the existing decoder Function
with the reward-weighted criterion (`subgc_reward_logits_fwd` / `subgc_reward_logsoftmax_bwd`).  No host copy and no synchronisation
anywhere on that path.

`RewardReferences` is the one-time setup (numpy allowed): document frequencies and `ref_len = log(n_img)` are taken over exactly the images
given -- the upstream "corpus" mode with the training set as the corpus, so `--cached_tokens` needs no file.

With `sc_samples = n >= 2` (the upstream `train_sample_n` with the `new_self_critical` baseline) the step is ONE pass instead: the decoder
Function runs n b5 rows, sample-major, and every row draws its own next input word from the logits it has just formed
(`functions.DecoderFn.forward`, the `sc_onepass` branch), so the rollout and the replay's forward are the same launches and the logits
`subgc_sc_pick` reads are the logits the criterion differentiates, in every dtype.  There is no greedy half: a sample's baseline is the mean
score of the other n - 1 samples of its caption row (`SelfCriticalReward.enqueue_loo`, restated by `loo_reward_restatement`).

Out of scope: the structure-loss variants of later upstream versions, the greedy baseline beside several samples, decode rules inside the
sampling loop, METEOR and SPICE rewards.
"""
from __future__ import annotations

import numpy as np
import torch

from . import functions as F_
from . import ops
from ._lib import SubgcError
from .accuracy import MAX_T, AccuracyReferences, AccuracyScorer

SC_STREAM = 0x1F83D9ABFB41BD6B          # the rollout's own Philox stream (sampling._uniforms and scheduled sampling keep theirs)


def rows_to_words(rows, eos=True):
    """Token rows [n, L] (0-padded) -> per row the list of words as the reward scores them: the decimal strings of the ids before the first
    0 and, with `eos`, the end token itself as the word '0' (the upstream array_to_str; a row without a 0 has no end token)."""
    out = []
    for row in np.asarray(rows).reshape(len(rows), -1):
        words = []
        for w in row:
            if int(w) <= 0:
                if eos:
                    words.append("0")
                break
            words.append(str(int(w)))
        out.append(words)
    return out


class RewardReferences(AccuracyReferences):
    """The ground-truth captions of the training images as the reward needs them.  gts_per_image[j]: int array [n_caps, seq_length],
    0-padded -- what dataloaders/dataloader.py:212 slices out of `self.label` for image j.  Words are the decimal strings of the ids, so a
    model id keeps its value on the device; with `eos` the end token is the word '0', which receives a fresh id above every model id
    (`eos_id`).  `vocab_size`: the model's (ids 1 .. vocab_size); default: the largest id in the references."""

    def __init__(self, gts_per_image, eos=True, vocab_size=None, device="auto"):
        gts = [np.asarray(g) for g in gts_per_image]
        for j, g in enumerate(gts):
            if g.ndim != 2 or not np.issubdtype(g.dtype, np.integer):
                raise SubgcError(f"self-critical reward: the captions of image {j} are an int array [n_caps, seq_length], got {g.dtype} {g.shape}")
            if g.size and g.min() < 0:
                raise SubgcError(f"self-critical reward: a negative word id in the captions of image {j}")
        top = max([int(g.max()) for g in gts if g.size] + [int(vocab_size or 0), 1])
        self.eos = bool(eos)
        self.vocab_size = top
        ix_to_word = {str(i): str(i) for i in range(1, top + 1)}
        super().__init__([rows_to_words(g, self.eos) for g in gts], ix_to_word, device=device)
        # '0' is no model word, so build_id_map gave it the first fresh id; without an end token in any reference it has none yet
        self.eos_id = int(self.word_to_ix.get("0", top + 1)) if self.eos else 0

    @classmethod
    def from_labels(cls, label, label_start_ix, label_end_ix, indices, **kw):
        """From the loader's own arrays (dataloaders/dataloader.py:209-213): image `ix` owns label[label_start_ix[ix] - 1 : label_end_ix[ix]].
        `indices`: the dataset indices of the images, in the order gt_indices will name them (position in this list)."""
        label = np.asarray(label)
        return cls([label[int(label_start_ix[ix]) - 1:int(label_end_ix[ix])] for ix in indices], **kw)


class SelfCriticalReward:
    """reward = score(sampled) - score(greedy), score = cider_weight * CIDEr + bleu_weight * BLEU-4 (opts.py:149-152), per sub-graph."""

    def __init__(self, refs, cider_weight=1.0, bleu_weight=0.0):
        if not isinstance(refs, RewardReferences):
            raise SubgcError("self-critical reward: the references are a subgc.selfcritical.RewardReferences")
        self.cider_weight, self.bleu_weight = ops.check_reward_weights(cider_weight, bleu_weight)
        self.refs = refs
        self.scorer = AccuracyScorer(refs, oracle_num=1)
        self._seg = {}

    def check_index(self, image_index):
        """Host-side check of the images' indices into the references -> the list of ints."""
        idx = [int(x) for x in image_index]
        for i, j in enumerate(idx):
            if not 0 <= j < self.refs.n_img:
                raise SubgcError(f"self-critical reward: batch image {i} names reference image {j}; the references hold {self.refs.n_img} images "
                                 "(gt_indices are positions in the list the RewardReferences were built from)")
        return idx

    @staticmethod
    def check_steps(T):
        if T + 1 > MAX_T:
            raise SubgcError(f"self-critical reward: rollouts of {T} steps are scored as rows of T + 1 = {T + 1} words; the limit is {MAX_T}")

    def _segments(self, S, I, dev, n=2, pad=0):
        """Row boundaries of n blocks of S rows, image i owning S / I rows of every block; `pad` rows behind them form one more segment."""
        key = (S, I, str(dev), n, pad)
        if key not in self._seg:
            per = S // I
            self._seg[key] = ops.upload([k * S + i * per for k in range(n) for i in range(I)] + [n * S] + ([n * S + pad] if pad else []),
                                        torch.int32, dev)
        return self._seg[key]

    def _const(self, name, value, dev):
        key = (name, value, str(dev))
        if key not in self._seg:
            self._seg[key] = ops.upload([float(value)], torch.float64, dev)
        return self._seg[key]

    def enqueue_loo(self, rows, S, d_index, n):
        """The leave-one-out reward of a one-pass step ("new_self_critical": every sample's baseline is the mean score of the other
        samples of its caption row).  rows: device int64 [>= S + S % 2, T1], the scored rows as subgc_sc_prepare writes them, of which the
        first S = n b5 count, sample-major: row k b5 + s is sample k of caption row s, and image i owns the caption rows
        [i b5 / I, (i + 1) b5 / I) of every sample block; d_index: device int32 [I].
        -> (reward [S, T1] fp32, mean_reward [] fp32, scores [S] fp64, baseline [S] fp64), on the device, no host read.

        The contract (`loo_reward_restatement` restates it in numpy), every operation a correctly rounded fp64 one, no contraction:
            s_r          = w_cider * CIDEr_r + w_bleu * BLEU4_r                  as subgc_sc_reward forms it: they are ITS `scores` output
            tot_s        = ((s_{0,s} + s_{1,s}) + ...) + s_{n-1,s}               over the samples in ascending k
            baseline_k,s = (tot_s - s_{k,s}) / (n - 1)                           a true division
            reward[r, t] = float32(s_r - baseline_r)                             for every t < T1
            mean_reward  = float32(mean of float64(reward[:, 0]))                a statistic; its summation order is not pinned
        subgc_sc_reward scores an even number of rows, so an odd S scores one padding row more (an all-zero row of the caller's zero
        half, scored against image d_index[0] in a segment of its own; nothing reads its record).  The header table is closed, so the
        arithmetic behind `scores` is a handful of elementwise fp64 tensor operations on [n, b5] numbers, each its own launch (which is
        what keeps a multiply and an add from being contracted): n - 1 adds, a subtract, a divide by a DEVICE scalar (a host scalar
        would become a multiplication by its reciprocal), a subtract, the cast, and the copy that lays the reward out along t."""
        n = int(n)
        if rows.dim() != 2 or rows.dtype != torch.int64 or n < 2 or S % n or rows.size(0) < S + S % 2:
            raise SubgcError(f"self-critical reward: int64 scored rows [>= {S + S % 2}, T + 1] of {n} >= 2 sample blocks, got {rows.dtype} {tuple(rows.shape)}")
        b5, T1, I, pad = S // n, rows.size(1), d_index.numel(), S % 2
        self.check_steps(T1 - 1)
        if I < 1 or b5 % I:
            raise SubgcError(f"self-critical reward: {b5} caption rows do not divide over {I} images")
        dev = rows.device
        R, segs = S + pad, n * I + pad
        arena = torch.empty(max(self.scorer.arena_words(R, segs), 2), device=dev, dtype=torch.int32)
        idx = torch.cat([d_index] * n + ([d_index[:1]] if pad else [])).to(torch.int32)
        self.scorer.enqueue(rows[:R], self._segments(b5, I, dev, n, pad), segs, idx, None, 0, arena, oracle=False)
        row_d = self.scorer.views(arena, R, segs)[0]
        _, _, scores = ops.sc_reward(row_d, R // 2, T1, self.cider_weight, self.bleu_weight)
        s = scores[:S].view(n, b5)
        tot = s[0] + s[1]
        for k in range(2, n):
            tot = tot + s[k]
        baseline = (tot.unsqueeze(0) - s) / self._const("n-1", n - 1, dev)
        r32 = (s - baseline).to(torch.float32).view(S, 1)
        reward = r32.expand(S, T1).contiguous()
        return reward, r32.to(torch.float64).mean().to(torch.float32), scores[:S], baseline.view(S)

    def enqueue(self, seq2, d_index, rows=None):
        """seq2: device int64 [2S, T], sampled half first; d_index: device int32 [I], the reference image of every batch image, image i
        owning the sampled rows [i S / I, (i + 1) S / I) and the same greedy rows.  -> (reward [S, T + 1] fp32, mean_reward [] fp32,
        scores [2S] fp64), all on the device: four launches, no host copy, no synchronisation.  `rows`: the scored rows [2S, T + 1] when
        the caller's own subgc_sc_prepare launch has already written them (with this object's refs.eos_id)."""
        if seq2.dim() != 2 or seq2.size(0) % 2 or seq2.dtype != torch.int64:
            raise SubgcError(f"self-critical reward: int64 rollout tokens [2 S, T], got {seq2.dtype} {tuple(seq2.shape)}")
        S, T = seq2.size(0) // 2, seq2.size(1)
        self.check_steps(T)
        I = d_index.numel()
        if I < 1 or S % I:
            raise SubgcError(f"self-critical reward: {S} sub-graphs do not divide over {I} images")
        dev = seq2.device
        if rows is None:
            _, _, rows = ops.sc_prepare(seq2.contiguous(), self.refs.n_ids + 1, self.refs.eos_id, want_replay=False)
        elif tuple(rows.shape) != (2 * S, T + 1) or rows.dtype != torch.int64:
            raise SubgcError(f"self-critical reward: scored rows are int64 [2 S, T + 1] = [{2 * S}, {T + 1}], got {rows.dtype} {tuple(rows.shape)}")
        arena = torch.empty(max(self.scorer.arena_words(2 * S, 2 * I), 2), device=dev, dtype=torch.int32)
        idx2 = torch.cat([d_index, d_index]).to(torch.int32)
        self.scorer.enqueue(rows, self._segments(S, I, dev), 2 * I, idx2, None, 0, arena, oracle=False)
        row_d = self.scorer.views(arena, 2 * S, 2 * I)[0]
        return ops.sc_reward(row_d, S, T + 1, self.cider_weight, self.bleu_weight)


MAX_SAMPLES = 16


def check_samples(sc_samples):
    """The `sc_samples` / `train_sample_n` option -> int: 1 is the two-pass step with the greedy baseline, 2 .. 16 the one-pass step with the
    leave-one-out baseline; anything else is refused with the number in the text."""
    if isinstance(sc_samples, bool) or not isinstance(sc_samples, (int, np.integer)) or not 1 <= int(sc_samples) <= MAX_SAMPLES:
        raise ValueError(f"sc_samples = {sc_samples!r}: the samples per caption row are an int in 1 .. {MAX_SAMPLES} (1: greedy baseline, two passes; "
                         f">= 2: leave-one-out baseline, one pass)")
    return int(sc_samples)


def loo_reward_restatement(scores, n):
    """The contract of `SelfCriticalReward.enqueue_loo` in numpy: scores fp64 [n b5], sample-major -> (reward fp32 [n b5], baseline fp64
    [n b5], mean_reward float).  Explicit adds in ascending sample order, a true division, one operation per statement."""
    n = int(n)
    s = np.asarray(scores, np.float64).reshape(n, -1)
    if n < 2:
        raise ValueError(f"loo_reward_restatement: n = {n}; a leave-one-out baseline needs at least 2 samples")
    tot = s[0] + s[1]
    for k in range(2, n):
        tot = tot + s[k]
    rest = tot[None, :] - s
    baseline = rest / np.float64(n - 1)
    reward = (s - baseline).astype(np.float32)
    return reward.reshape(-1), baseline.reshape(-1), float(reward.astype(np.float64).mean())


def onepass_uniforms(model, T, S, dev):
    """The one-pass step's Philox uniforms [T, S], drawn as `rollout` draws its own: stream SC_STREAM, one more `_sample_calls`."""
    model.__dict__["_sample_calls"] = model.__dict__.get("_sample_calls", 0) + 1
    seed = (int(torch.initial_seed()) * 1000003 + model.__dict__["_sample_calls"]) & 0xFFFFFFFFFFFFFFFF
    return ops.uniform((T, S), seed ^ SC_STREAM, 0, dev)


@torch.no_grad()
def rollout(model, fc, Xb, lens, sel_idx, img_s, N, uniforms=None, T=None):
    """The sampled and the greedy caption of every training sub-graph in ONE decode loop: rows [0, b5) sample from the whole distribution
    (the upstream sample_max = 0), rows [b5, 2 b5) are their greedy baselines.  fc [b5, 2L], Xb [B N, L] (detached here), lens, sel_idx,
    img_s: what AttModel._forward hands its decoder Function.  -> seq2 int64 [2 b5, T].  No dropout (functions.DecodeState has none), the
    bf16 decode weights under bf16 storage, no host read inside the loop; `uniforms` [T, b5] replaces the model's own Philox stream.
    `T`: the steps (default: the model's seq_length; AttModel._forward passes the width of the loader's captions)."""
    dev = fc.device
    b5, T = fc.size(0), int(T or model.seq_length)
    SelfCriticalReward.check_steps(T)
    two = lambda t: torch.cat([t, t]).contiguous()
    P = [p.detach() for p in model._decoder_params()]
    pr = F_.Prepared(two(fc.detach()), Xb.detach().contiguous(), two(lens), two(sel_idx), two(img_s), N, P, None, None, 1.0)
    st = F_.DecodeState(pr, P, N, False, xt_table=model.xt_gates_table(), fuse_lstm=True, snapshots=model.decode_snapshots(), W16=model.decode_w16(),
                        b16_batched=model.decode_b16_on())
    if uniforms is None:
        model.__dict__["_sample_calls"] = model.__dict__.get("_sample_calls", 0) + 1
        seed = (int(torch.initial_seed()) * 1000003 + model.__dict__["_sample_calls"]) & 0xFFFFFFFFFFFFFFFF
        uniforms = ops.uniform((T, b5), seed ^ SC_STREAM, 0, dev)
    elif tuple(uniforms.shape) != (T, b5):
        raise SubgcError(f"rollout: step-major uniforms [T, b5] = [{T}, {b5}], got {tuple(uniforms.shape)}")
    n = 2 * b5
    z = lambda *s, dt=torch.float32: ops.zero_(torch.empty(*s, device=dev, dtype=dt))
    seq, seqlp, it = z(n, T, dt=torch.long), z(n, T), z(n, dt=torch.long)
    unfinished, counts = z(n, dt=torch.int32), z(T, dt=torch.int32)
    for t in range(T):
        logits = st.step(it, None, normalize=False)
        ops.sc_pick(logits, b5, 1.0, uniforms[t], t, seq, seqlp, it, unfinished, counts[t:t + 1], counts[t - 1:t] if t > 0 else None, raw=True)
    return seq
