"""A decoder stand-in for the beam-attention tests: a row's whole "state" is an integer hash of the tokens it was fed, its logits are a
fixed pseudo-random function of that hash over a 12-word vocabulary (the end token comes early, beams end at different lengths) and its
"attention row" is an affine code of the same hash.  So the attention that belongs to word w of a beam is known in closed form from the
beam's own tokens -- code(chain(seq[:w])) -- and any off-by-one in step, slot or group shift of the ancestry bookkeeping shows.

Integer arithmetic stays below 2^62, so numpy int64 (host engine) and torch int64 (device engine) agree bit for bit."""
import numpy as np
import torch

V1 = 12                      # 11 words + UNK (the last column)
MOD = 2147483647


def mix(h, tok):
    """State after feeding `tok` to a row in state h (works on python ints, numpy int64 and torch int64)."""
    return (h * 1103515245 + tok * 12345 + 1013904223) % MOD


def seed_of(s, salt):
    return (s * 7919 + salt * 104729 + 17) % MOD


def chain(s, salt, tokens):
    """The state of a row of sub-graph s after <bos> and then `tokens`."""
    h = mix(seed_of(s, salt), 0)
    for w in tokens:
        h = mix(h, int(w))
    return h


def code(h, length, N):
    """The attention row of a step run in state h on a sub-graph of `length` nodes: exact small integers, zero behind the length."""
    out = np.zeros(N, np.float32)
    for j in range(length):
        out[j] = float((h % 65521) * (j + 1) % 4093 + j)
    return out


def logits_np(h):
    """[rows] int64 -> [rows, V1] fp32: multiples of 1/4 (ties on purpose), the end token favoured in one state out of three."""
    v = np.arange(V1, dtype=np.int64)[None, :]
    x = ((h[:, None] % 100003) * (v * 7919 + 13)) % 29
    x = x.astype(np.float32) / 4
    x[:, 0] += np.where(h % 3 == 0, 5.0, -2.0).astype(np.float32)
    return x


def logits_torch(h):
    v = torch.arange(V1, device=h.device, dtype=torch.int64)[None, :]
    x = (((h[:, None] % 100003) * (v * 7919 + 13)) % 29).float() / 4
    x[:, 0] += torch.where(h % 3 == 0, 5.0, -2.0)
    return x


def code_torch(h, lens_rows, N):
    j = torch.arange(N, device=h.device, dtype=torch.int64)[None, :]
    a = ((h[:, None] % 65521) * (j + 1) % 4093 + j).float()
    return torch.where(j < lens_rows[:, None], a, torch.zeros_like(a))


class HostEngine:
    """The engine protocol of `beam.search` (first / advance / reorder / snapshot / restore / attention) on numpy."""

    def __init__(self, n, beam, lens, N, salt):
        self.n, self.rows, self.V1, self.N, self.salt = n, n * beam, V1, N, salt
        self.lens = np.repeat(np.asarray(lens, np.int64), beam)
        self.h = np.repeat(np.array([seed_of(s, salt) for s in range(n)], np.int64), beam)
        self.alpha = None

    def _step(self, tok, kk):
        self.h = mix(self.h, np.asarray(tok, np.int64))
        self.alpha = np.stack([code(int(h), int(l), self.N) for h, l in zip(self.h, self.lens)])
        x = logits_np(self.h)
        m = x.max(1, keepdims=True)
        lp = (x - m - np.log(np.exp(x - m).sum(1, keepdims=True, dtype=np.float32))).astype(np.float32)
        idx = np.argsort(-lp, axis=1, kind="stable")[:, :kk]                       # value descending, index ascending
        return np.take_along_axis(lp, idx, 1), idx.astype(np.int32)

    def first(self, kk):
        return self._step(np.zeros(self.rows, np.int64), kk)

    def advance(self, tok, kk):
        return self._step(tok, kk)

    def attention(self):
        return self.alpha

    def reorder(self, src):
        self.h = self.h[np.asarray(src, np.int64)]

    def snapshot(self):
        return [self.h.copy()]

    def restore(self, rows, snap):
        self.h = self.h.copy()
        self.h[rows] = snap[0][rows]


class _DeviceState:
    """What `DeviceSearch.loop` asks of `eng.st`: step / reorder / recurrent / reset and N, on device tensors."""

    def __init__(self, n, beam, lens, N, salt, dev):
        self.N, self.dev = N, dev
        self.seed = torch.tensor([seed_of(s, salt) for s in range(n)], dtype=torch.int64, device=dev).repeat_interleave(beam)
        self.lens = torch.tensor(list(lens), dtype=torch.int64, device=dev).repeat_interleave(beam)
        self.h = self.seed.clone()
        self.V1 = V1

    def reset(self):
        self.h = self.seed.clone()

    def recurrent(self):
        return [self.h]

    def reorder(self, src):
        self.h = self.h[src.long()]

    def step(self, it, alpha_out, normalize=True):
        self.h = mix(self.h, it)
        if alpha_out is not None:
            alpha_out.copy_(code_torch(self.h, self.lens, self.N))
        x = logits_torch(self.h)
        return torch.log_softmax(x, 1).contiguous() if normalize else x.contiguous()


class DeviceEngine:
    def __init__(self, n, beam, lens, N, salt, dev):
        self.n, self.rows, self.dev, self.V1 = n, n * beam, torch.device(dev), V1
        self.st = _DeviceState(n, beam, lens, N, salt, self.dev)

    def snapshot(self):
        return [x.clone() for x in self.st.recurrent()]


def check_beam(b_seq, b_att, length, s, salt, n_nodes, N):
    """The hash-chain property of one beam: attention row w is the code of the state reached along the beam's OWN first w words."""
    seq = [int(x) for x in b_seq]
    assert len(b_att) == length
    for w in range(length):
        want = code(chain(s, salt, seq[:w]), n_nodes, N)
        np.testing.assert_array_equal(np.asarray(b_att[w], np.float32), want, err_msg=f"sub-graph {s} word {w} of {seq}")
