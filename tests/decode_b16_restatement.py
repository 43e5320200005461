"""The bf16-batched decode step (functions.DecodeState, regime "bf16-batched") restated in numpy fp64, with round-to-nearest-even to bf16
at exactly the points include/subgc_decode_b16_hip.h and DESIGN 4.U name: the six weight twins, h_att / h_lang (= hout) / ctx as stored,
and fc for Gf.  Everything else -- products, pre-activations, cell state, attention scores, logits -- is fp64 here and fp32 on the device.
No GPU, no torch."""
import numpy as np


def bf16(x):
    """float -> nearest bf16 (ties to even), returned as float64.  The value goes through fp32 first, as on the device."""
    u = np.ascontiguousarray(np.asarray(x, np.float64).astype(np.float32)).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32).astype(np.float64).reshape(np.shape(x))


def bf16_bits(x):
    """The 16-bit patterns of `bf16(x)` as int64 (neighbouring bf16 values of one sign differ by 1)."""
    return (np.ascontiguousarray(bf16(x).astype(np.float32)).view(np.uint32) >> 16).astype(np.int64).reshape(np.shape(x))


def bits_to_f64(b):
    """uint16 bf16 bit patterns -> float64."""
    return (np.asarray(b).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def cell(pre, c_prev):
    """nn.LSTMCell pointwise, gate order i, f, g, o -> (c fp64, h fp64 before rounding)."""
    R = pre.shape[1] // 4
    i, f, g, o = sigmoid(pre[:, :R]), sigmoid(pre[:, R:2 * R]), np.tanh(pre[:, 2 * R:3 * R]), sigmoid(pre[:, 3 * R:])
    c = f * (0.0 if c_prev is None else c_prev) + i * g
    return c, o * np.tanh(c)


def cell_pre(g0, table=None, tok=None, g2=None, b0=None, b1=None):
    """subgc_decode_cell_b16's pre-activation: g0 + table[clamp(tok)] + g2 + b0 + b1 (each optional)."""
    pre = np.asarray(g0, np.float64).copy()
    if table is not None:
        pre = pre + np.asarray(table, np.float64)[np.clip(np.asarray(tok), 0, table.shape[0] - 1)]
    for t in (g2, b0, b1):
        if t is not None:
            pre = pre + np.asarray(t, np.float64)
    return pre


def attention(ah, u, v, mask, w_a, b_a):
    """AttModel.py:445-471 on fp64: u [S, n, A], v [S, n, R], mask [S, n] -> (ctx [S, R], alpha [S, n])."""
    e = np.tanh(u + ah[:, None, :]) @ w_a.reshape(-1) + float(np.asarray(b_a).reshape(-1)[0])
    e = np.where(mask > 0, e, -np.inf)
    e = e - e.max(1, keepdims=True)
    w = np.exp(e)
    w = w / w.sum(1, keepdims=True)
    return np.einsum("sn,snr->sr", w, v), w


def log_softmax(x):
    x = x - x.max(1, keepdims=True)
    return x - np.log(np.exp(x).sum(1, keepdims=True))


class Restated:
    """One decode of S rows.  W: {reference state_dict key: array} (fp32 masters); f [S, R], v [S, n, R], u [S, n, A], mask [S, n]: the
    prepared features (fp32 values; the attention sets are NOT rounded -- they stay fp32 on the device)."""

    def __init__(self, W, f, v, u, mask):
        d = lambda k: np.asarray(W[k], np.float64)
        self.R = R = d("core.att_lstm.weight_hh").shape[1]
        w1i = d("core.att_lstm.weight_ih")
        # the twins (natural gate order), K-concatenated as the device does
        self.Wc1 = np.concatenate([bf16(w1i[:, :R]), bf16(d("core.att_lstm.weight_hh"))], 1)                      # . [h_lang | h_att]
        self.Wc2 = np.concatenate([bf16(d("core.lang_lstm.weight_ih")), bf16(d("core.lang_lstm.weight_hh"))], 1)  # . [ctx | h_att | h_lang]
        self.W1f, self.h2a, self.lg = bf16(w1i[:, R:2 * R]), bf16(d("core.attention.h2att.weight")), bf16(d("logit.weight"))
        # the x->gates table is built by an fp32 product of the fp32 masters (AttModel.xt_gates_table) and read as fp32
        self.table = np.maximum(d("embed.0.weight"), 0.0) @ w1i[:, 2 * R:].T
        self.b1 = d("core.att_lstm.bias_ih") + d("core.att_lstm.bias_hh")
        self.b2 = d("core.lang_lstm.bias_ih") + d("core.lang_lstm.bias_hh")
        self.h2a_b, self.lg_b = d("core.attention.h2att.bias"), d("logit.bias")
        self.w_a, self.b_a = d("core.attention.alpha_net.weight"), d("core.attention.alpha_net.bias")
        self.v, self.u, self.mask = (np.asarray(x, np.float64) for x in (v, u, mask))
        S = self.v.shape[0]
        self.Gf = bf16(f) @ self.W1f.T                                                                            # once per decode
        z = lambda: np.zeros((S, R))
        self.h_att, self.h_lang, self.ctx, self.c1, self.c2 = z(), z(), z(), z(), z()                             # h / ctx: bf16 values

    def step(self, tok):
        """-> (logits fp64 [S, V+1], alpha); the state moves on."""
        pre1 = np.concatenate([self.h_lang, self.h_att], 1) @ self.Wc1.T
        self.c1, h = cell(cell_pre(pre1, self.table, tok, self.Gf, self.b1), self.c1)
        self.h_att = bf16(h)
        ah = self.h_att @ self.h2a.T + self.h2a_b
        ctx, alpha = attention(ah, self.u, self.v, self.mask, self.w_a, self.b_a)
        self.ctx = bf16(ctx)
        pre2 = np.concatenate([self.ctx, self.h_att, self.h_lang], 1) @ self.Wc2.T
        self.c2, h = cell(cell_pre(pre2, b0=self.b2), self.c2)
        self.h_lang = bf16(h)
        return self.h_lang @ self.lg.T + self.lg_b, alpha
