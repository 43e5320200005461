"""Decode rules of the non-beam token loop: block_trigrams, decoding_constraint (the repeat ban), block_bad_endings and suppress_unk.

The reference's `test.py` accepts `--block_trigrams`, `--decoding_constraint` and `--remove_bad_endings` (opts.py:78-80) but its
`_sample` loop (AttModel.py:282-319) applies none of them; only beam search honours `decoding_constraint` (CaptionModel.py:128-131).
Here the rules act on the log-probabilities of a step, between AttModel.py:289 and :295, as ONE row pass on the device
(`ops.decode_rules`, include/subgc_decode_rules_hip.h) in front of the unchanged pick kernels.

`DecodeRules` is the host-side description (hashable: it keys the graph caches); `apply_rules_restatement` restates the contract in
numpy with an fp64 log-softmax -- what the tests compare the kernel with, and the host loop of the stand-in states.

Beam search takes block_trigrams and the bad-ending ban per beam through `eval_kwargs["beam_rules"]` (`DecodeRules.from_beam_options`;
`beam.DeviceSearch` / `beam.search` rule every state row before the top-k reads it); `sequence_events` counts what the rules did
along one beam.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from .eval_glue import BAD_ENDINGS

MAX_BAD_IDS = 64                      # SUBGC_RULES_MAX_BAD
FLAG_TRIGRAMS, FLAG_UNK, FLAG_REPEAT, FLAG_BAD_END = 1, 2, 4, 8
STAT_NAMES = ("trigram", "repeat", "bad_ending", "changed")
BEAM_REFUSED = ("block_trigrams", "block_bad_endings", "suppress_unk")
BEAM_RULE_KEYS = ("block_trigrams", "trigram_alpha", "block_bad_endings", "bad_ending_ids")   # eval_kwargs["beam_rules"]


def bad_ending_ids(ix_to_word):
    """The ids (ascending) of `eval_glue.BAD_ENDINGS` present in the vocabulary `ix_to_word` ({str(id): word})."""
    return tuple(sorted(int(ix) for ix, w in ix_to_word.items() if w in BAD_ENDINGS))


@dataclass(frozen=True)
class DecodeRules:
    block_trigrams: int = 0
    trigram_alpha: float = 2.0        # the penalty of one earlier occurrence is -0.693 * alpha (upstream: 2.0); inf: a hard block
    decoding_constraint: int = 0
    block_bad_endings: int = 0
    suppress_unk: int = 0
    bad_ids: tuple = ()

    def __post_init__(self):
        a = float(self.trigram_alpha)
        if math.isnan(a) or a < 0:
            raise ValueError(f"trigram_alpha = {self.trigram_alpha}: the trigram penalty needs alpha >= 0 (inf: a hard block)")
        ids = tuple(int(i) for i in self.bad_ids)
        if len(ids) > MAX_BAD_IDS:
            raise ValueError(f"bad_ids holds {len(ids)} ids: the bad-ending list takes at most {MAX_BAD_IDS}")
        if any(i < 0 for i in ids):
            raise ValueError(f"bad_ids holds a negative id: {min(ids)}")
        for name in ("block_trigrams", "decoding_constraint", "block_bad_endings", "suppress_unk"):
            object.__setattr__(self, name, int(bool(getattr(self, name))))
        object.__setattr__(self, "trigram_alpha", a)
        object.__setattr__(self, "bad_ids", ids)

    @property
    def active(self):
        return bool(self.block_trigrams or self.decoding_constraint or self.block_bad_endings or self.suppress_unk)

    @property
    def flags(self):
        return (FLAG_TRIGRAMS * self.block_trigrams + FLAG_UNK * self.suppress_unk + FLAG_REPEAT * self.decoding_constraint
                + FLAG_BAD_END * self.block_bad_endings)

    @property
    def trigram_pen(self):
        """The fp32 constant one earlier occurrence adds: float32(float32(-0.693) * float32(alpha)); alpha = 0 gives -0.0."""
        with np.errstate(over="ignore"):
            return np.float32(np.float32(-0.693) * np.float32(self.trigram_alpha))

    @property
    def key(self):
        """Hashable: what a captured loop depends on (an inactive set of rules is one key whatever its fields)."""
        if not self.active:
            return None
        return (self.flags, float(self.trigram_pen) if self.block_trigrams else 0.0, self.bad_ids if self.block_bad_endings else ())

    @classmethod
    def from_options(cls, opt, ix_to_word=None):
        """The rules of an `eval_kwargs` dict.  Keys: block_trigrams, trigram_alpha, decoding_constraint, block_bad_endings,
        suppress_unk and, for block_bad_endings, bad_ending_ids (a list of ids) unless `ix_to_word` is given.  With beam_size > 1 the
        three rules beam search does not know raise; decoding_constraint keeps its beam meaning there (the rules returned are inactive)."""
        opt = opt or {}
        if int(opt.get("beam_size", 1) or 1) > 1:
            for name in BEAM_REFUSED:
                if opt.get(name, 0):
                    raise ValueError(f"{name} = {opt[name]} with beam_size = {opt['beam_size']}: the decode rules act on the greedy / "
                                     "sampling loop only (beam search honours decoding_constraint alone; block_trigrams and "
                                     "block_bad_endings under beam search go into eval_kwargs['beam_rules'])")
            return cls()
        ids = ()
        if opt.get("block_bad_endings", 0):
            if opt.get("bad_ending_ids") is not None:
                ids = tuple(int(i) for i in opt["bad_ending_ids"])
            elif ix_to_word is not None:
                ids = bad_ending_ids(ix_to_word)
            else:
                raise ValueError("block_bad_endings needs the ids of the bad endings: pass eval_kwargs['bad_ending_ids'] "
                                 "(decode_rules.bad_ending_ids(ix_to_word)) or the vocabulary")
        return cls(block_trigrams=opt.get("block_trigrams", 0) or 0, trigram_alpha=opt.get("trigram_alpha", 2.0),
                   decoding_constraint=opt.get("decoding_constraint", 0) or 0, block_bad_endings=opt.get("block_bad_endings", 0) or 0,
                   suppress_unk=opt.get("suppress_unk", 0) or 0, bad_ids=ids)


    @classmethod
    def from_beam_options(cls, opt, ix_to_word=None):
        """The rules of `eval_kwargs["beam_rules"]`: a dict with the keys block_trigrams, trigram_alpha, block_bad_endings and
        bad_ending_ids (or `ix_to_word`), honoured by beam search only.  -> a DecodeRules with at most the trigram and bad-ending
        flags set (inactive when the key is absent).  Same limits and messages as `from_options`; beam_size <= 1, a
        decoding_constraint / suppress_unk entry (beam search has its own repeat ban, the top-level decoding_constraint, and always
        applies the UNK penalty) and unknown keys raise."""
        opt = opt or {}
        br = opt.get("beam_rules")
        if br is None:
            return cls()
        if not isinstance(br, dict):
            raise ValueError(f"beam_rules must be a dict with keys among {BEAM_RULE_KEYS}, got {type(br).__name__}")
        beam = int(opt.get("beam_size", 1) or 1)
        if beam <= 1:
            raise ValueError(f"beam_rules with beam_size = {beam}: the key is honoured by beam search only; the greedy / sampling loop "
                             "takes the top-level keys block_trigrams, trigram_alpha, block_bad_endings and bad_ending_ids")
        for name in ("decoding_constraint", "suppress_unk"):
            if name in br:
                raise ValueError(f"beam_rules['{name}']: beam search has its own repeat ban (the top-level decoding_constraint) and "
                                 "always applies the UNK penalty; beam_rules takes " + ", ".join(BEAM_RULE_KEYS))
        unknown = sorted(k for k in br if k not in BEAM_RULE_KEYS)
        if unknown:
            raise ValueError(f"beam_rules: unknown key(s) {unknown}; it takes " + ", ".join(BEAM_RULE_KEYS))
        ids = ()
        if br.get("block_bad_endings", 0):
            if br.get("bad_ending_ids") is not None:
                ids = tuple(int(i) for i in br["bad_ending_ids"])
            elif ix_to_word is not None:
                ids = bad_ending_ids(ix_to_word)
            else:
                raise ValueError("block_bad_endings needs the ids of the bad endings: pass eval_kwargs['beam_rules']['bad_ending_ids'] "
                                 "(decode_rules.bad_ending_ids(ix_to_word)) or the vocabulary")
        return cls(block_trigrams=br.get("block_trigrams", 0) or 0, trigram_alpha=br.get("trigram_alpha", 2.0),
                   block_bad_endings=br.get("block_bad_endings", 0) or 0, bad_ids=ids)


def sequence_events(seq_row, length, rules):
    """The counters of ONE beam under `beam_rules`, from its own words: int32 [4] in STAT_NAMES order -- the number of steps
    0 .. length - 1 at which a trigram penalty applied (the words before the step repeat their last two somewhere earlier, followed by
    a word >= 0), 0, the number of steps at which the bad-ending ban applied (the word before is a listed id), and -1: "the first
    arg-max moved" is undefined under beam search."""
    return sequence_events_rows(np.asarray(seq_row).reshape(1, -1), [int(length)], rules)[0]


def sequence_events_rows(seqs, lengths, rules):
    """`sequence_events` of many beams at once: seqs int [m, T], lengths int [m] -> int32 [m, 4]."""
    h = np.asarray(seqs, np.int64)
    m, T = h.shape
    L = np.minimum(np.asarray(lengths, np.int64).reshape(m), T)
    out = np.zeros((m, 4), np.int32)
    out[:, 3] = -1
    for t in range(1, T):
        step = t < L                                                  # the beam has a word t, chosen from the row ruled at step t
        if rules.block_trigrams and t >= 3:
            hit = np.zeros(m, bool)
            for j in range(t - 2):
                hit |= (h[:, j] == h[:, t - 2]) & (h[:, j + 1] == h[:, t - 1]) & (h[:, j + 2] >= 0)
            out[:, 0] += hit & step
        if rules.block_bad_endings and rules.bad_ids:
            out[:, 2] += np.isin(h[:, t - 1], rules.bad_ids) & step
    return out


def trigram_counts(h, t, V):
    """{column: count} of block_trigrams at step t for the history h[0 .. t-1]."""
    out = {}
    if t >= 3:
        for j in range(t - 2):
            if h[j] == h[t - 2] and h[j + 1] == h[t - 1] and 0 <= h[j + 2] < V:
                out[int(h[j + 2])] = out.get(int(h[j + 2]), 0) + 1
    return out


def apply_rules_restatement(logits, history, t, rules, return_events=False):
    """The contract of `subgc_decode_rules` in numpy: fp64 log-softmax of `logits` ([n, V] or [V]), then the rules of step t from
    `history` ([n, >= t] or [>= t]) in the contract's order.  -> the ruled rows (float64, same shape); with `return_events` also
    int64 [n, 4]: per row whether a trigram penalty / the repeat ban / the bad-ending ban was applied and whether the first arg-max
    moved (the columns of `stats`)."""
    x = np.asarray(logits, dtype=np.float64)
    one = x.ndim == 1
    x = np.atleast_2d(x)
    h = np.atleast_2d(np.asarray(history, dtype=np.int64))
    if h.size == 0:
        h = np.zeros((x.shape[0], 0), np.int64)
    n, V = x.shape
    mx = x.max(1, keepdims=True)
    lp = (x - mx) - np.log(np.exp(x - mx).sum(1, keepdims=True))
    before = lp.argmax(1)
    ev = np.zeros((n, 4), np.int64)
    pen = float(rules.trigram_pen)
    for r in range(n):
        hr = h[r]
        if rules.block_trigrams:
            for col, c in sorted(trigram_counts(hr, t, V).items()):
                lp[r, col] = lp[r, col] + float(c) * pen
                ev[r, 0] = 1
        if rules.suppress_unk:
            lp[r, V - 1] = lp[r, V - 1] - 1000.0
        if t >= 1:
            last = int(hr[t - 1])
            if rules.decoding_constraint and 0 <= last < V:
                lp[r, last] = -np.inf
                ev[r, 1] = 1
            if rules.block_bad_endings and last in rules.bad_ids:
                lp[r, 0] = -np.inf
                ev[r, 2] = 1
    ev[:, 3] = lp.argmax(1) != before
    lp = lp[0] if one else lp
    return (lp, ev) if return_events else lp
