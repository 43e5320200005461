"""A decoder stand-in for the beam-rules tests: the logits of a row depend only on (its sub-graph, the last token it was fed) through a
fixed table [n, V1 + 1, V1] (row V1: the <bos> state).  The table holds multiples of 1/4 (exact in fp32, ties on purpose); a 4-word
cycle 1 -> 2 -> 3 -> 4 -> 1 is boosted by +4, so a plain beam search walks the cycle and repeats trigrams, and every end-token entry is
lowered by 1, so beams run long enough to do so.  (tests/beam_att_fake.py's hash decoder never repeats a trigram: useless here.)

It comes as a numpy engine (the `beam.search` protocol; it honours the `history` keyword through `apply_rules_restatement`), as a
device state (what `DeviceSearch.loop` asks of `eng.st`) and as a device-backed host engine that rules and ranks its rows through
`beam.ruled_topk`, `_BatchEngine`'s own two launches.  The "attention row" of a step is an exact integer code of (sub-graph, last token fed)."""
import numpy as np
import torch

from subgc import beam
from subgc.decode_rules import DecodeRules, apply_rules_restatement

V1 = 12                      # 11 words + UNK (the last column); column 0 is the end token
BOS = V1                     # the table row of the <bos> state
CYCLE = (1, 2, 3, 4)
SHAPES = ((2, 1), (3, 1), (4, 2), (6, 3))        # (beam, group)


def table(n, salt, end_boost=0.0):
    """fp32 [n, V1 + 1, V1].  `end_boost` (the bad-ending tests): added to the end-token entry behind the words 1..3, so that a plain
    search does end "listed id, end token"."""
    rng = np.random.default_rng(1000 + salt)
    tab = rng.integers(0, 12, size=(n, V1 + 1, V1)).astype(np.float32) / 4
    for a, b in zip(CYCLE, CYCLE[1:] + CYCLE[:1]):
        tab[:, a, b] += 4
    tab[:, :, 0] -= 1
    tab[:, 1:4, 0] += np.float32(end_boost)
    return tab


def code(s, last, length, N):
    """The attention row of a step of sub-graph s run after feeding `last` (BOS for the first step): zero behind the length."""
    out = np.zeros(N, np.float32)
    out[:length] = (s * 131 + int(last) * 17 + np.arange(length)).astype(np.float32)
    return out


def ruled_row(tab, s, words, t, rules):
    """fp32 [V1]: the restatement's ruled log-probabilities of the step that chooses word t of a beam of sub-graph s with `words`."""
    last = BOS if t == 0 else int(words[t - 1])
    return apply_rules_restatement(tab[s, last], np.asarray(words[:t], np.int64), t, rules).astype(np.float32)


def repeats_trigram(words, length):
    w = [int(x) for x in words[:length]]
    seen = set()
    for j in range(len(w) - 2):
        tri = tuple(w[j:j + 3])
        if tri in seen:
            return True
        seen.add(tri)
    return False


def length_of(words, T):
    """Length of a kept beam of this decoder: up to and with its first end token, else T (cut)."""
    w = [int(x) for x in words]
    return w.index(0) + 1 if 0 in w else T


class HostEngine:
    """The engine protocol of `beam.search` on numpy."""

    def __init__(self, n, beam_size, lens, N, salt, end_boost=0.0):
        self.n, self.rows, self.V1, self.N = n, n * beam_size, V1, N
        self.tab = table(n, salt, end_boost)
        self.sub = np.repeat(np.arange(n), beam_size)
        self.lens = np.repeat(np.asarray(lens, np.int64), beam_size)
        self.last = np.full(self.rows, BOS, np.int64)
        self.alpha = None

    def _step(self, last, kk, history):
        self.last = np.asarray(last, np.int64).copy()
        self.alpha = np.stack([code(s, l, int(k), self.N) for s, l, k in zip(self.sub, self.last, self.lens)])
        x = self.tab[self.sub, self.last]
        if history is None:
            lp = apply_rules_restatement(x, np.zeros((self.rows, 0), np.int64), 0, DecodeRules())
        else:
            lp = np.stack([apply_rules_restatement(x[r], history.words[r, :history.length[r]], int(history.length[r]), history.rules)
                           for r in range(self.rows)])
        lp = lp.astype(np.float32)
        idx = np.argsort(-lp, axis=1, kind="stable")[:, :kk]                       # value descending, index ascending
        return np.take_along_axis(lp, idx, 1), idx.astype(np.int32)

    def first(self, kk, history=None):
        return self._step(np.full(self.rows, BOS, np.int64), kk, history)

    def advance(self, tok, kk, history=None):
        return self._step(tok, kk, history)

    def attention(self):
        return self.alpha

    def reorder(self, src):
        self.last = self.last[np.asarray(src, np.int64)]

    def snapshot(self):
        return [self.last.copy()]

    def restore(self, rows, snap):
        self.last = self.last.copy()
        self.last[rows] = snap[0][rows]


class _DeviceState:
    """What `DeviceSearch.loop` asks of `eng.st`: step / reorder / recurrent / reset and N, on device tensors."""

    def __init__(self, n, beam_size, lens, N, salt, dev, end_boost=0.0):
        self.N, self.dev, self.V1 = N, dev, V1
        self.tab = torch.from_numpy(table(n, salt, end_boost)).to(dev)
        self.sub = torch.arange(n, device=dev).repeat_interleave(beam_size)
        self.lens = torch.tensor(list(lens), dtype=torch.int64, device=dev).repeat_interleave(beam_size)
        self.reset()

    def reset(self):
        self.last = torch.full_like(self.sub, BOS)
        self.fresh = True

    def recurrent(self):
        return [self.last]

    def reorder(self, src):
        self.last = self.last[src.long()]

    def step(self, it, alpha_out, normalize=True):
        self.last = torch.full_like(self.sub, BOS) if self.fresh else it.clone()
        self.fresh = False
        if alpha_out is not None:
            j = torch.arange(self.N, device=self.dev)[None, :]
            a = (self.sub[:, None] * 131 + self.last[:, None] * 17 + j).float()
            alpha_out.copy_(torch.where(j < self.lens[:, None], a, torch.zeros_like(a)))
        x = self.tab[self.sub, self.last]
        return torch.log_softmax(x, 1).contiguous() if normalize else x.contiguous()


class DeviceEngine:
    """For `DeviceSearch` (st / snapshot) and, through first / advance / ..., for the host `search`: the same state on the device, its
    rows ruled and ranked by `beam.ruled_topk`, the function `_BatchEngine` itself calls."""

    def __init__(self, n, beam_size, lens, N, salt, dev, end_boost=0.0):
        self.n, self.rows, self.dev, self.V1 = n, n * beam_size, torch.device(dev), V1
        self.st = _DeviceState(n, beam_size, lens, N, salt, self.dev, end_boost)
        self.alpha = torch.zeros(self.rows, N, device=self.dev)
        self.topk_bufs = {}

    def snapshot(self):
        return [x.clone() for x in self.st.recurrent()]

    def restore(self, rows, snap):
        sel = torch.from_numpy(np.asarray(rows, np.int64)).to(self.dev)
        self.st.last[sel] = snap[0][sel]

    def reorder(self, src):
        self.st.reorder(torch.from_numpy(np.asarray(src, np.int64)).to(self.dev))

    def first(self, kk, history=None):
        return beam.ruled_topk(self.st.step(torch.zeros(self.rows, device=self.dev, dtype=torch.long), self.alpha, normalize=False), kk, history, self.topk_bufs)

    def advance(self, tok, kk, history=None):
        return beam.ruled_topk(self.st.step(torch.from_numpy(np.asarray(tok, np.int64)).to(self.dev), self.alpha, normalize=False), kk, history, self.topk_bufs)

    def attention(self):
        return self.alpha.cpu().numpy()
