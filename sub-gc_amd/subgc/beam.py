"""Beam search / diverse beam search on the HIP decode path.

Reference: CaptionModel.beam_search (models/CaptionModel.py:28-176) driven per sub-graph by
AttModel._sample_sentences (models/AttModel.py:179-234).  The reference walks the sub-graphs one by
one, sorts a [beam, V+1] matrix on the CPU-visible side every step and forks Python lists of states.

Here every sub-graph and every beam of one image is a row of ONE decode batch (rows = n_subgraphs x beam):
the attention rows of a sub-graph are shared by its beams through the (offset, length) table, a step is
the same kernel sequence as greedy decode, `subgc_row_topk_f32` hands back the leading beam+2 log-probs of
every row, the candidate bookkeeping (tiny: beam^2 numbers per sub-graph) runs on the host in the
reference's exact order and arithmetic (fp32 sums, stable sort over the column-major candidate list), and
the fork "beam q -> slot vix" is one row gather of the recurrent state.

Why beam+2 columns are enough: a group's augmented row differs from the raw one only at the UNK column
(-1000, CaptionModel.py:137), at the previous word (decoding_constraint, :134-135) and at the <= beam-bdash
distinct words the earlier groups picked (:33-40), all of which only move DOWN; the top bdash of the
augmented row therefore lie within the top (bdash + those) <= beam+2 of the raw row.  Under `beam_rules` (block_trigrams and the
bad-ending ban per beam) "the raw row" is the RULED row -- `subgc_decode_rules` rewrites the logits row in place
before the top-k reads it -- so the same argument holds word for word.
"""
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch

from . import functions as F_
from . import ops

_F32 = np.float32


def penalty_builder(cfg):
    """misc/utils.py:145-171."""
    if cfg == "":
        return lambda length, logprob: logprob
    kind, alpha = cfg.split("_")
    alpha = float(alpha)
    if kind == "wu":
        return lambda length, logprob: logprob / (((5 + length) ** alpha) / ((5 + 1) ** alpha))
    if kind == "avg":
        return lambda length, logprob: logprob / length
    raise ValueError(f"unknown length_penalty {cfg!r} (expected '', 'wu_<alpha>' or 'avg_<alpha>')")


# What `search` hands to an engine's `first` / `advance` under beam_rules: `rules` (DecodeRules), `words` int64 [rows, T] (row r: the
# words of the beam that occupies state row r, unshifted, -1 behind its length), `length` int [rows] and `t` = the decoder step about
# to be ruled (0: <bos>; loop iteration i feeds step i + 1) and `columns` = T + group_size - 1, the width of the device layout.  A live
# row of group g has length t - g.
RuleHistory = namedtuple("RuleHistory", "rules words length t columns")


def shifted_history(words, length, t, Th):
    """The device layout of the histories of one step: int64 [rows, Th], row r = (t - length[r]) times -1, then its words, then -1:
    word w of a group-g row sits in column g + w, so ONE step number t serves every live group in `subgc_decode_rules`."""
    words, length = np.asarray(words, np.int64), np.asarray(length, np.int64)
    out = np.full((words.shape[0], Th), -1, np.int64)
    for r in range(words.shape[0]):
        L = int(length[r])
        if L > t:
            raise ValueError(f"beam rules: row {r} holds {L} words before step {t}")
        out[r, t - L:t] = words[r, :L]
    return out


def check_rule_limits(T, G):
    """The history of a state row has T + G - 1 columns and is staged in LDS by `subgc_decode_rules` (SUBGC_RULES_MAX_T)."""
    if T + G - 1 > 64:
        raise ValueError(f"beam_rules: the history of a state row takes T + group_size - 1 = {T + G - 1} columns; the limit is 64")


def ruled_topk(logits, kk, history, bufs):
    """The top-k of one step of the host `search` over an engine's logits [rows, V1] on the device -> (values, indices) as numpy
    [rows, kk].  `history` None: `subgc_row_topk_f32` folds the log-softmax in.  A RuleHistory: the two launches of `DeviceSearch.loop`
    -- `subgc_decode_rules` on the shifted histories (in place on `logits`), then the top-k of the ruled rows with log_softmax = 0.
    `bufs`: a dict the caller keeps for the life of its engine; the output buffers and the uploaded bad-ending ids live there."""
    rows, dev = logits.size(0), logits.device
    if "vals" not in bufs:
        bufs["vals"] = torch.empty(rows, kk, device=dev, dtype=torch.float32)
        bufs["idx"] = torch.empty(rows, kk, device=dev, dtype=torch.int32)
    vals, idx = bufs["vals"], bufs["idx"]
    if history is None:
        ops.row_topk(logits, kk, vals, idx, log_softmax=True)
    else:
        rules = history.rules
        if "bad_ids" not in bufs:
            bufs["bad_ids"] = ops.upload(list(rules.bad_ids), torch.int32, dev) if (rules.block_bad_endings and rules.bad_ids) else None
        hist = torch.from_numpy(shifted_history(history.words, history.length, history.t, history.columns)).to(dev)
        ops.decode_rules(logits, hist, history.t, rules.flags, rules.trigram_pen, bufs["bad_ids"], None, None)
        ops.row_topk(logits, kk, vals, idx, log_softmax=False)
    return vals.cpu().numpy(), idx.cpu().numpy()


def _active(rules):
    return rules if (rules is not None and rules.active) else None


def _beam_events(rules, seq_row, length):
    from .decode_rules import sequence_events                                 # (decode_rules imports eval_glue: not at module load)
    return sequence_events(seq_row, length, rules)


def winners_rule_stats(done_beams):
    """int32 [n, 4] (a CPU tensor): the "rule_stats" of every sub-graph's winning beam, done_beams[s][0]."""
    return torch.from_numpy(np.stack([np.asarray(b[0]["rule_stats"], np.int32) for b in done_beams]).reshape(-1, 4))


class _Group:
    """One beam group of one sub-graph: the tables of CaptionModel.py:106-108."""
    __slots__ = ("seq", "lps", "sums", "done", "anc")

    def __init__(self, T, bd):
        self.seq = np.zeros((T, bd), np.int64)
        self.anc = np.zeros((T, bd), np.int32)                                   # the slot every beam held after each of its words
        self.lps = np.zeros((T, bd), _F32)
        self.sums = np.zeros(bd, _F32)
        self.done = []


def _beam_step(grp, vals, idx, tau, bd, unk, constraint, earlier, lam):
    """CaptionModel.py:44-94 on the leading columns.  vals/idx: [bd, kk] raw log-probs (descending) and
    their word ids.  Returns the source beam of every new slot."""
    vals = vals.copy()
    if constraint and tau > 0:                                                   # :134-135
        vals[idx == grp.seq[tau - 1][:, None]] = -np.inf
    vals[idx == unk] -= _F32(1000)                                               # :137
    unaug = vals.copy()
    for prev in earlier:                                                         # add_diversity, :33-40
        for tok in prev.seq[tau]:
            vals[idx == tok] -= lam
    order = np.argsort(-vals, axis=1, kind="stable")
    rows = 1 if tau == 0 else bd
    cols = min(bd, vals.shape[1])
    cands = []
    for c in range(cols):
        for q in range(rows):
            j = order[q, c]
            cands.append((_F32(grp.sums[q] + vals[q, j]), q, int(idx[q, j]), unaug[q, j]))
    cands.sort(key=lambda x: -x[0])                                              # stable, like sorted() at :73
    prev_seq, prev_lps, prev_anc = grp.seq[:tau].copy(), grp.lps[:tau].copy(), grp.anc[:tau].copy()
    src = []
    for vix in range(bd):
        p, q, tok, r = cands[vix]
        grp.seq[:tau, vix] = prev_seq[:, q]
        grp.lps[:tau, vix] = prev_lps[:, q]
        grp.anc[:tau, vix] = prev_anc[:, q]
        grp.anc[tau, vix] = vix
        grp.seq[tau, vix] = tok
        grp.lps[tau, vix] = r
        grp.sums[vix] = p
        src.append(q)
    return src


class _BatchEngine:
    """All sub-graphs x beams of an image batch as rows of one DecodeState (the product path)."""

    def __init__(self, pr, P, N, beam, xt_table=None, snapshots=None, return_att=False, W16=None, b16_batched=False):
        n, dev = pr.S, pr.f.device
        self.n, self.rows, self.dev = n, n * beam, dev
        rep = torch.arange(n, device=dev).repeat_interleave(beam)
        prb = SimpleNamespace(S=self.rows, N=N, f=pr.f.index_select(0, rep).contiguous(), u=pr.u, v=pr.v,
                              off=pr.off.index_select(0, rep).contiguous(), lens=pr.lens.index_select(0, rep).contiguous())
        self.pr, self.prb, self.rep = pr, prb, rep
        self.st = F_.DecodeState(prb, P, N, bool(return_att), xt_table=xt_table, fuse_lstm=True, snapshots=snapshots,      # fused for <= 32 rows
                                   W16=W16, b16_batched=b16_batched)                  # default: no twins, beam search streams the fp32 weights
        self.V1 = self.st.V1
        self.alpha = torch.empty(self.rows, N, device=dev, dtype=torch.float32) if return_att else None    # host `search`: the last step's rows
        self.topk_bufs = {}                                                      # `ruled_topk`'s outputs (and the uploaded bad-ending ids)

    def refresh(self):
        """Re-derive the per-beam rows from `pr` and restart the recurrent state (hipGraph replay: `pr` was overwritten in place)."""
        ops.take_rows([(self.pr.f, self.prb.f), (self.pr.off, self.prb.off), (self.pr.lens, self.prb.lens)], self.rep)      # one launch
        self.st.reset()

    def _topk(self, logits, kk, history=None):
        return ruled_topk(logits, kk, history, self.topk_bufs)

    def first(self, kk, history=None):                                           # <bos>, AttModel.py:223-227
        return self._topk(self.st.step(torch.zeros(self.rows, device=self.dev, dtype=torch.long), self.alpha, normalize=False), kk, history)

    def advance(self, tok, kk, history=None):
        return self._topk(self.st.step(torch.from_numpy(tok).to(self.dev), self.alpha, normalize=False), kk, history)

    def attention(self):
        """[rows, N] attention rows of the step `first` / `advance` just ran (host `search` with return_att)."""
        if self.alpha is None:
            raise ValueError("this engine was built without attention output (return_att)")
        return self.alpha.cpu().numpy()

    def reorder(self, src):
        if self.st.b16 and src.size and not (0 <= int(src.min()) and int(src.max()) < self.rows):      # the host knows these rows: refuse, not clamp
            from ._lib import SubgcError
            raise SubgcError(f"beam fork: source rows {int(src.min())} .. {int(src.max())} outside the state's {self.rows} rows")
        self.st.reorder(torch.from_numpy(src).to(self.dev))

    def snapshot(self):
        return [x.clone() for x in self.st.recurrent()]       # bf16 [h2 | h1] and h2 slot, fp32 c1, c2 in the bf16-batched regime

    def restore(self, rows, snap):
        sel = torch.from_numpy(rows.astype(np.int64)).to(self.dev)
        for cur, saved in zip(self.st.recurrent(), snap):
            cur[sel] = saved[sel]


class _StepEngine:
    """The reference's own calling convention (CaptionModel.beam_search): a (h, c) state of shape [2, beam, R] that the
    CALLER owns, advanced through `model.get_logprobs_state` -- one sub-graph, `beam` rows."""

    def __init__(self, model, init_state, init_logprobs, args):
        self.m, self.state, self.logp, self.args = model, tuple(init_state), init_logprobs, args
        self.n, self.rows, self.dev, self.V1 = 1, init_logprobs.size(0), init_logprobs.device, init_logprobs.size(1)

    def _topk(self, logp, kk):
        vals = torch.empty(self.rows, kk, device=self.dev, dtype=torch.float32)
        idx = torch.empty(self.rows, kk, device=self.dev, dtype=torch.int32)
        ops.row_topk(logp.float().contiguous(), kk, vals, idx, log_softmax=False)
        return vals.cpu().numpy(), idx.cpu().numpy()

    _NO_RULES = ("beam_rules: the step-API engine (get_logprobs_state) hands over log-probabilities its caller computed and cannot rule "
                 "them; decode through mode='sample' / sample_images")

    def first(self, kk, history=None):
        if history is not None:
            raise ValueError(self._NO_RULES)
        return self._topk(self.logp, kk)

    def advance(self, tok, kk, history=None):
        if history is not None:
            raise ValueError(self._NO_RULES)
        logp, self.state = self.m.get_logprobs_state(torch.from_numpy(tok).to(self.dev), *self.args, self.state)
        return self._topk(logp, kk)

    def attention(self):
        raise ValueError("the step-API engine has no attention output: its <bos> step is the caller's (CaptionModel.beam_search)")

    def reorder(self, src):
        sel = torch.from_numpy(src.astype(np.int64)).to(self.dev)
        self.state = tuple(s.index_select(1, sel) for s in self.state)

    def snapshot(self):
        return [s.clone() for s in self.state]

    def restore(self, rows, snap):
        sel = torch.from_numpy(rows.astype(np.int64)).to(self.dev)
        self.state = tuple(s.clone() for s in self.state)
        for cur, saved in zip(self.state, snap):
            cur[:, sel] = saved[:, sel]


@torch.no_grad()
def beam_decode(pr, P, N, T, opt, xt_table=None, on_device=True, return_att=False, W16=None, b16_batched=False, rules=None):
    """Decode every sub-graph of `pr` (an F_.Prepared) with beam search.
    Returns (seq [n, T] int64, seqLogprobs [n, T] fp32, done_beams) -- CPU tensors, as the reference's are.
    `on_device` (default): the candidate bookkeeping runs in `subgc_beam_step`, the loop has no host round trip;
    False keeps it on the host (`search`, the restatement the device kernel is tested against).
    `return_att`: a fourth element {"AL": fp32 [T + 1, n, N] (device tensor; numpy from the host `search`), "len": int array [n]}: the
    attention rows of every sub-graph's winning beam, AL[w, s] = the distribution of the decoder step whose logits produced word w of
    seq[s], zero for w >= len[s] (len counts the end token and is T for a beam cut at the last step).  Beam search never feeds its last
    word (CaptionModel.py:170-171), so unlike a greedy decode there is no attention row behind the last word: AL[T] is all zero.
    `rules` (DecodeRules.from_beam_options, active): every step's rows are ruled before the top-k reads them and
    every kept beam gains "rule_stats"; on the host path through the same two launches, so the two agree bit for bit."""
    eng = _BatchEngine(pr, P, N, int(opt.get("beam_size", 10)), xt_table, return_att=return_att, W16=W16, b16_batched=b16_batched)
    return search_device(eng, T, opt, return_att, rules) if on_device else search(eng, T, opt, return_att, rules)


def check_picks(pick, cnt):
    """The host's range check in front of `subgc_beam_att_gather`: pick int [n, 2] = (group, finished-beam slot) per sub-graph, cnt int
    [n, G] = the finished beams of every group.  Raises SubgcError naming the first offender; needs no GPU."""
    from ._lib import SubgcError
    pick, cnt = np.asarray(pick), np.asarray(cnt)
    if pick.ndim != 2 or pick.shape[1] != 2 or cnt.ndim != 2 or pick.shape[0] != cnt.shape[0]:
        raise SubgcError(f"beam attention: picks [n, 2] and finished-beam counts [n, G], got {pick.shape} and {cnt.shape}")
    n, G = cnt.shape
    for s in range(n):
        g, j = int(pick[s, 0]), int(pick[s, 1])
        if not 0 <= g < G:
            raise SubgcError(f"beam attention: sub-graph {s} picks group {g}; the search has {G}")
        if not 0 <= j < int(cnt[s, g]):
            raise SubgcError(f"beam attention: sub-graph {s} picks finished beam {j} of group {g}, which finished {int(cnt[s, g])}")
    return pick.astype(np.int32)


def check_att_limits(T, bd, kk, N):
    """The limits of subgc_beam_att_hip.h, refused on the host with the number in the text."""
    from ._lib import SubgcError
    if T > 64 or bd > 16 or kk > 18:
        raise SubgcError(f"beam attention: T = {T}, beams per group = {bd}, leading columns = {kk}; the limits are T <= 64, bd <= 16, kk <= 18")
    if not 1 <= N <= ops.BEAM_ATT_MAX_N:
        raise SubgcError(f"beam attention: {N} attention columns; the limit is {ops.BEAM_ATT_MAX_N}")


class DeviceTables:
    """The tables of CaptionModel.py:106-109 for n sub-graphs x G groups, resident on the device."""

    def __init__(self, n, G, T, bd, dev, return_att=False):
        z = lambda *s, dt: ops.zero_(torch.empty(*s, device=dev, dtype=dt))
        self.cap = bd * T                                                         # a group finishes at most bd beams per step
        # the ancestry tables of subgc_beam_step_anc (return_att): forked like `seq`, filed like `done_seq`; they stay on the device
        self.anc = z(n, G, T, bd, dt=torch.int32) if return_att else None
        self.done_anc = z(n, G, self.cap, T, dt=torch.int32) if return_att else None
        self.seq, self.lps, self.sums = z(n, G, T, bd, dt=torch.int32), z(n, G, T, bd, dt=torch.float32), z(n, G, bd, dt=torch.float32)
        # the finished-beam tables are views of ONE 4-byte buffer: `collect` brings them to the host with a single copy (five
        # synchronising copies cost 0.15 ms of a 2.8 ms one-image search)
        cap = self.cap
        sizes = [n * G, n * G * cap * T, n * G * cap * T, n * G * cap, n * G * cap]
        self.done_all = z(sum(sizes), dt=torch.int32)
        parts, o = [], 0
        for k in sizes:
            parts.append(self.done_all[o:o + k]); o += k
        self.done_cnt = parts[0].view(n, G)
        self.done_seq, self.done_lps = parts[1].view(n, G, cap, T), parts[2].view(torch.float32).view(n, G, cap, T)
        self.done_p, self.done_len = parts[3].view(torch.float32).view(n, G, cap), parts[4].view(n, G, cap)
        self._sizes = sizes

    def done_to_host(self):
        """(cnt, seq, lps, p, len) as numpy arrays after ONE device -> host copy."""
        n, G = self.done_cnt.shape
        cap, T = self.cap, self.done_seq.size(3)
        h = self.done_all.cpu().numpy()
        out, o = [], 0
        for k in self._sizes:
            out.append(h[o:o + k]); o += k
        return (out[0].reshape(n, G), out[1].reshape(n, G, cap, T), out[2].view(np.float32).reshape(n, G, cap, T),
                out[3].view(np.float32).reshape(n, G, cap), out[4].reshape(n, G, cap))


def _check(opt, eng):
    beam = int(opt.get("beam_size", 10))
    G = int(opt.get("group_size", 1))
    if G < 1 or beam % G:
        raise ValueError(f"beam_size {beam} must be a multiple of group_size {G}")
    bd = beam // G
    if eng.rows != eng.n * beam:
        raise ValueError(f"{eng.rows} state rows for {eng.n} sub-graph(s) x beam {beam}")
    kk = min(eng.V1, beam + 2)
    if bd > kk:
        raise ValueError("beam wider than the vocabulary")
    return beam, G, bd, kk


class DeviceSearch:
    """`search` with the per-step bookkeeping in `subgc_beam_step`: every step is top-k -> beam step -> state gather ->
    decoder step on the stream (`loop`: launches only, no host read, so it can be captured in a hipGraph); the host reads
    the finished beams once, after the last step (`collect`).
    `rules` (active): every decoder step is followed by `subgc_decode_rules` on the rows' histories, which live on the device as two
    ping-pong int64 buffers [rows, T + G - 1] (word w of group g in column g + w, -1 elsewhere), forked with the state's `src` after
    every beam step; the top-k then reads the ruled rows with log_softmax = 0.  The launch sequence stays static."""

    def __init__(self, eng, T, opt, return_att=False, rules=None):
        self.eng, self.T, self.opt = eng, T, dict(opt)
        self.rules = _active(rules)
        self.beam, self.G, self.bd, self.kk = _check(opt, eng)
        self.lam = float(_F32(opt.get("diversity_lambda", 0.5)))
        self.constraint = opt.get("decoding_constraint", 0)
        n, rows, dev, G, bd, kk = eng.n, eng.rows, eng.dev, self.G, self.bd, self.kk
        self.return_att = bool(return_att)
        self.tb = DeviceTables(n, G, T, bd, dev, self.return_att)
        self.AL_step = None
        if self.return_att:
            # step-major attention rows: slice 0 = the <bos> step, slice t + 1 = the decoder step of loop iteration t (the last
            # iteration, T + G - 2, feeds nothing: T + G - 1 slices).  Histories are NOT reordered per step -- the ancestry table says
            # on which row every word of a beam was produced, and one gather after the ranking reads exactly the winners' rows.
            self.N = int(eng.st.N)
            check_att_limits(T, bd, kk, self.N)
            self.AL_step = ops.zero_(torch.empty(T + G - 1, rows, self.N, device=dev, dtype=torch.float32))
        self.tok = ops.zero_(torch.empty(rows, device=dev, dtype=torch.long))
        self.src = ops.zero_(torch.empty(rows, device=dev, dtype=torch.int32))
        self.tv = torch.empty(rows, kk, device=dev, dtype=torch.float32)
        self.ti = torch.empty(rows, kk, device=dev, dtype=torch.int32)
        if G > 1:
            self.nv, self.ni = torch.empty_like(self.tv), torch.empty_like(self.ti)
            base = torch.arange(rows, device=dev).view(n, G, bd)
            self.group_rows = [base[:, g].reshape(-1).contiguous() for g in range(G)]
        self.hist = self.hist_now = None
        if self.rules is not None:
            check_rule_limits(T, G)
            Th = self.Th = T + G - 1
            self.bad_ids = None
            if self.rules.block_bad_endings and self.rules.bad_ids:
                self.bad_ids = ops.upload(list(self.rules.bad_ids), torch.int32, dev)
            # the constant template (all -1) and the two copies that ping-pong; `loop` starts from the template, so a replay starts clean
            self.hist0 = torch.empty(rows, Th, device=dev, dtype=torch.long)     # (one uploaded row, gathered into every row)
            ops.take_rows([(ops.upload([-1] * Th, torch.int64, dev).view(1, Th), self.hist0)], ops.zero_(torch.empty(rows, device=dev, dtype=torch.long)))
            self.hist = [torch.empty_like(self.hist0), torch.empty_like(self.hist0)]
            if G > 1:                                                             # column t belongs to the groups that are live at iteration t
                g_of = (torch.arange(rows, device=dev) // bd) % G
                t_of = torch.arange(Th, device=dev).view(Th, 1)
                self.live_rows = ((g_of <= t_of) & (t_of <= T - 1 + g_of)).contiguous()

    def _fork_history(self, cur, t):
        """history[row] <- history[src[row]], then column t <- the step's `tok` for the rows of the groups that stepped (a sleeping
        group's tok of 0 is not written: its column keeps -1).  G == 1: two C-ABI launches on the 4-byte word views."""
        a, b = self.hist[cur], self.hist[1 - cur]
        ops.gather_rows(ops._words(a), self.src, ops._words(b))
        if self.G == 1:
            ops.copy2d(ops._words(self.tok.view(-1, 1)), ops._words(b)[:, 2 * t:2 * t + 2])
        else:
            b[:, t] = torch.where(self.live_rows[t], self.tok, self.hist0[:, t])
        return 1 - cur

    def _rule(self, logits, cur, t):
        r = self.rules
        ops.decode_rules(logits, self.hist[cur], t, r.flags, r.trigram_pen, self.bad_ids, None, None)

    def loop(self, fresh_tables=False):
        eng, T, G, bd, kk, tb = self.eng, self.T, self.G, self.bd, self.kk, self.tb
        n, unk = eng.n, eng.V1 - 1
        tv, ti, tok, src = self.tv, self.ti, self.tok, self.src
        if not fresh_tables:
            for x in (tb.seq, tb.lps, tb.sums, tb.done_cnt, tok):
                ops.zero_(x)
        att = self.AL_step
        step = ops.beam_step_anc if att is not None else ops.beam_step
        ruled = self.rules is not None                                           # the top-k then reads log-probabilities (log_softmax = 0)
        logits = eng.st.step(tok, None if att is None else att[0], normalize=False)                                         # <bos>, AttModel.py:223-227
        if ruled:
            now = 0                                                              # which of the two history copies is current
            ops.copy_(self.hist[0], self.hist0)
            self._rule(logits, now, 0)
        ops.row_topk(logits, kk, tv, ti, log_softmax=not ruled)
        if G > 1:
            init = eng.snapshot()
            tv4, ti4, nv4, ni4 = (x.view(n, G, bd, kk) for x in (tv, ti, self.nv, self.ni))
        for t in range(T + G - 1):
            step(tv, ti, tb, tok, src, t, T, G, bd, kk, unk, self.constraint, self.lam)
            if ruled:
                now = self.hist_now = self._fork_history(now, t)
            if not any(g <= t + 1 <= T + g - 1 for g in range(G)):
                break
            if G > 1 and 0 < t < G:                                               # group t starts now: give it the post-<bos> state
                sel = self.group_rows[t]
                for cur, saved in zip(eng.st.recurrent(), init):
                    cur.index_copy_(0, sel, saved.index_select(0, sel))
            eng.st.reorder(src)
            logits = eng.st.step(tok, None if att is None else att[t + 1], normalize=False)
            if ruled:
                self._rule(logits, now, t + 1)
            if G == 1:
                ops.row_topk(logits, kk, tv, ti, log_softmax=not ruled)
            else:
                ops.row_topk(logits, kk, self.nv, self.ni, log_softmax=not ruled)
                for g in range(G):
                    if g <= t <= T + g - 1:                                       # only the groups that stepped take the new rows
                        tv4[:, g], ti4[:, g] = nv4[:, g], ni4[:, g]

    def collect(self, which=(0, 0)):
        """-> (seq, seqlp, done_beams) and, with return_att, a fourth element {"AL": fp32 [T + 1, n, N] on the device, "len": int32 [n]}
        (see `beam_decode`) gathered by ONE launch behind the host's ranking.  `which` = (group g, rank r): the attention of the
        kept beam done_beams[s][g * bd + r] of every sub-graph instead of the winner's (0, 0)."""
        tb, T, G, bd, n, opt = self.tb, self.T, self.G, self.bd, self.eng.n, self.opt
        length_penalty = penalty_builder(opt.get("length_penalty", ""))
        # one read of the finished beams; ranking (:174-175) vectorised, python objects only for the beams that are kept
        cnt, dseq, dlps, dp, dlen = tb.done_to_host()
        valid = np.arange(tb.cap)[None, None, :] < cnt[:, :, None]
        if opt.get("length_penalty", "") == "":
            p = dp.astype(np.float64)
        else:                                                                         # the reference's python-float arithmetic, entry by entry
            p = np.zeros(dp.shape, np.float64)
            for s_, g_, j_ in zip(*np.nonzero(valid)):
                p[s_, g_, j_] = length_penalty(int(dlen[s_, g_, j_]), float(dp[s_, g_, j_]))
        if n and int(cnt.min()) < bd:
            raise RuntimeError("beam search ended with fewer finished beams than slots")   # the last step finishes every slot (:151)
        order = np.argsort(np.where(valid, -p, np.inf), axis=-1, kind="stable")[:, :, :bd]
        oi = order[..., None]                                                         # numpy gathers: single-threaded, no thread-pool wake-ups
        top_seq = torch.from_numpy(np.take_along_axis(dseq, oi, 2).astype(np.int64))  # [n, G, bd, T]
        top_lps = torch.from_numpy(np.take_along_axis(dlps, oi, 2))
        top_p = np.take_along_axis(p, order, -1).reshape(-1).tolist()
        top_un = np.take_along_axis(dlps.sum(-1, dtype=_F32), order, -1).reshape(-1).tolist()
        rs, rl = top_seq.reshape(-1, T).unbind(0), top_lps.reshape(-1, T).unbind(0)
        per = G * bd
        done_beams = [[{"seq": rs[k], "logps": rl[k], "unaug_p": top_un[k], "p": top_p[k]} for k in range(s * per, (s + 1) * per)]
                      for s in range(n)]
        if self.rules is not None:                                                    # every kept beam's counters, from its own words
            from .decode_rules import sequence_events_rows
            ev = sequence_events_rows(top_seq.reshape(-1, T).numpy(), np.take_along_axis(dlen, order, -1).reshape(-1), self.rules)
            for s in range(n):
                for k, b in enumerate(done_beams[s]):
                    b["rule_stats"] = ev[s * per + k]
        seq, seqlp = top_seq[:, 0, 0].clone(), top_lps[:, 0, 0].clone()
        if not self.return_att:
            return seq, seqlp, done_beams
        g, r = int(which[0]), int(which[1])
        if not (0 <= g < G and 0 <= r < bd):
            from ._lib import SubgcError
            raise SubgcError(f"beam attention: kept beam (group {g}, rank {r}) of {G} group(s) x {bd} beam(s)")
        pick = check_picks(np.stack([np.full(n, g, np.int64), order[:, g, r]], 1) if n else np.zeros((0, 2), np.int64), cnt)
        lens = np.minimum(dlen[np.arange(n), g, pick[:, 1]], T).astype(np.int32) if n else np.zeros(0, np.int32)
        AL = torch.empty(T + 1, n, self.N, device=self.eng.dev, dtype=torch.float32)      # every element is written, zero rows included
        if n:
            ops.beam_att_gather(self.AL_step, tb, ops.upload(pick.ravel(), torch.int32, self.eng.dev), n, G, bd, T, AL)
        return seq, seqlp, done_beams, {"AL": AL, "len": lens}


@torch.no_grad()
def search_device(eng, T, opt, return_att=False, rules=None):
    ds = DeviceSearch(eng, T, opt, return_att, rules)
    ds.loop(fresh_tables=True)
    return ds.collect()


@torch.no_grad()
def search(eng, T, opt, return_att=False, rules=None):
    """The bookkeeping of CaptionModel.beam_search (:97-176) over an engine that owns the recurrent state.
    `rules` (DecodeRules.from_beam_options, active): before every `first` / `advance` the words of the beam that occupies each state row
    (after the fork; unshifted, per group) go to the engine as `history=RuleHistory(...)`, and the engine rules its rows -- log-softmax,
    then block_trigrams and the bad-ending ban of `subgc_decode_rules` -- before its top-k; every kept beam gains "rule_stats"
    (`decode_rules.sequence_events`).  Inactive or None: the engines are called exactly as before.
    `return_att`: the engine also answers `attention()` ([rows, N] of the step it just ran); every kept beam gains "att" (fp32 [len, N]:
    the attention row of the step whose logits produced each of its words, backtracked through the beam's ancestry: word 0 from the
    <bos> step, word w >= 1 of group g from the step of loop iteration w + g - 1 at the row of the slot the beam held after word
    w - 1), "anc" and "len", and a fourth element {"AL": numpy fp32 [T + 1, n, N], "len": int32 [n]} describes the winners."""
    beam = int(opt.get("beam_size", 10))
    G = int(opt.get("group_size", 1))
    lam = opt.get("diversity_lambda", 0.5)
    constraint = opt.get("decoding_constraint", 0)
    length_penalty = penalty_builder(opt.get("length_penalty", ""))
    if G < 1 or beam % G:
        raise ValueError(f"beam_size {beam} must be a multiple of group_size {G}")
    lam = _F32(lam)
    bd = beam // G
    n, rows, V1 = eng.n, eng.rows, eng.V1
    if rows != n * beam:
        raise ValueError(f"{rows} state rows for {n} sub-graph(s) x beam {beam}")
    unk = V1 - 1
    kk = min(V1, beam + 2)
    if bd > kk:
        raise ValueError("beam wider than the vocabulary")
    shape = (n, G, bd, kk)
    rules = _active(rules)
    if rules is not None:
        check_rule_limits(T, G)
        words, length = np.full((n, G, bd, T), -1, np.int64), np.zeros((n, G, bd), np.int64)
        hist = lambda step: {"history": RuleHistory(rules, words.reshape(rows, T), length.reshape(rows), step, T + G - 1)}
    else:
        hist = lambda step: {}
    tv, ti = (x.reshape(shape).copy() for x in eng.first(kk, **hist(0)))
    att_steps = [np.array(eng.attention(), np.float32)] if return_att else None     # slice 0: <bos>; slice t + 1: iteration t's step
    init = eng.snapshot() if G > 1 else None
    groups = [[_Group(T, bd) for _ in range(G)] for _ in range(n)]
    base = np.arange(rows, dtype=np.int32).reshape(n, G, bd)
    for t in range(T + G - 1):
        live = [g for g in range(G) if g <= t <= T + g - 1]
        src = base.copy()
        tok = np.zeros((n, G, bd), np.int64)
        for g in live:
            tau = t - g
            for s in range(n):
                grp = groups[s][g]
                q = _beam_step(grp, tv[s, g], ti[s, g], tau, bd, unk, constraint, groups[s][:g], lam)
                src[s, g] = base[s, g][q]
                for vix in range(bd):                                            # :150-166
                    if grp.seq[tau, vix] == 0 or t == T + g - 1:
                        final = {"seq": grp.seq[:, vix].copy(), "logps": grp.lps[:, vix].copy(),
                                 "unaug_p": float(grp.lps[:, vix].sum(dtype=_F32)), "p": float(grp.sums[vix])}
                        final["p"] = length_penalty(tau + 1, final["p"])
                        if return_att:
                            final.update(anc=grp.anc[:tau + 1, vix].copy(), len=tau + 1, rows=base[s, g].copy(), shift=g)
                        if rules is not None:
                            final["rule_stats"] = _beam_events(rules, grp.seq[:, vix], tau + 1)
                        grp.done.append(final)
                        grp.sums[vix] = -1000
                tok[s, g] = grp.seq[tau]
        if not any(g <= t + 1 <= T + g - 1 for g in range(G)):
            break                                                                # the reference's last step (:170-171) feeds nothing
        if G > 1 and 0 < t < G:                                                  # group t starts now: give it the post-<bos> state
            eng.restore(base[:, t].reshape(-1), init)
        eng.reorder(src.reshape(-1))
        if rules is not None:                                                    # the rows' beams after the fork: t + 1 - g words of group g
            length[:] = 0
            for g in live:
                for s in range(n):
                    words[s, g, :, :t - g + 1] = groups[s][g].seq[:t - g + 1].T
                length[:, g] = t - g + 1
        nv, ni = (x.reshape(shape) for x in eng.advance(tok.reshape(-1), kk, **hist(t + 1)))
        if return_att:
            att_steps.append(np.array(eng.attention(), np.float32))
        for g in live:
            tv[:, g], ti[:, g] = nv[:, g], ni[:, g]
    seq = torch.zeros(n, T, dtype=torch.long)
    seqlp = torch.zeros(n, T, dtype=torch.float32)
    done_beams = []
    for s in range(n):
        beams = []
        for g in range(G):
            beams += sorted(groups[s][g].done, key=lambda x: -x["p"])[:bd]       # :174-175
        for b in beams:
            b["seq"], b["logps"] = torch.from_numpy(b["seq"]), torch.from_numpy(b["logps"])
        done_beams.append(beams)
        seq[s], seqlp[s] = beams[0]["seq"], beams[0]["logps"]
    if not return_att:
        return seq, seqlp, done_beams
    N = att_steps[0].shape[1]
    AL, lens = np.zeros((T + 1, n, N), np.float32), np.zeros(n, np.int32)
    for s, beams in enumerate(done_beams):
        for b in beams:
            rows_g, g = b.pop("rows"), b.pop("shift")
            b["att"] = np.stack([att_steps[0][rows_g[0]]] + [att_steps[w + g][rows_g[b["anc"][w - 1]]] for w in range(1, b["len"])])
        AL[:beams[0]["len"], s], lens[s] = beams[0]["att"], beams[0]["len"]
    return seq, seqlp, done_beams, {"AL": AL, "len": lens}
