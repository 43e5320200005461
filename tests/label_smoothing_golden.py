"""Shared by the label-smoothing tests: the fixture the reference's own LabelSmoothing wrote (tests/golden/make_golden_label_smoothing.py)
and an fp64 numpy restatement of the closed form in include/subgc_criterion_hip.h.  test_label_smoothing_cpu.py ties the restatement to the
fixture; the GPU tests then use it as the reference on other shapes."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = 2.0 ** -24                                     # unit roundoff of fp32


def load_case():
    with open(os.path.join(GOLDEN, "label_smoothing_meta.json")) as f:
        meta = json.load(f)
    with np.load(os.path.join(GOLDEN, "label_smoothing_case.npz")) as z:
        return meta, {k: z[k] for k in z.files}


def load_train():
    with np.load(os.path.join(GOLDEN, "label_smoothing_train.npz")) as z:
        return {k: z[k] for k in z.files}


def constants(s, V):
    """conf, e, H in fp64 (0 log 0 = 0 at both ends)."""
    conf, e = 1.0 - s, s / (V - 1)
    H = (conf * np.log(conf) if conf > 0 else 0.0) + (s * np.log(e) if s > 0 else 0.0)
    return conf, e, H


def closed_form(logp, target, mask, s, dloss=1.0):
    """fp64: (loss, dlogp) of LabelSmoothing on log-probabilities [S, T, V]; target / mask may be wider than T (truncated)."""
    lp = np.asarray(logp, np.float64)
    S, T, V = lp.shape
    w = np.asarray(target)[:, :T].astype(np.int64)
    m = np.asarray(mask, np.float64)[:, :T]
    conf, e, H = constants(float(s), V)
    lpw = np.take_along_axis(lp, w[:, :, None], 2)[:, :, 0]
    row = H - conf * lpw - e * (lp.sum(2) - lpw)
    den = m.sum()
    td = np.full(lp.shape, e)
    np.put_along_axis(td, w[:, :, None], conf, 2)
    return float((m * row).sum() / den), -(dloss * m / den)[:, :, None] * td


def log_softmax64(x):
    x = np.asarray(x, np.float64)
    mx = x.max(-1, keepdims=True)
    return x - (mx + np.log(np.exp(x - mx).sum(-1, keepdims=True)))


def loss_bound(logp64, target, mask, s, lse=None):
    """The absolute bound of DESIGN 4.M on |loss_fp32 - loss_fp64| for the device's order of operations.
    slp is a sum of V fp32 terms: a lane adds ceil(V / 256) of them in sequence, six tree levels and four waves follow, so its error is at
    most (ceil(V / 256) + 10) u sum|lp|; it enters the row with the weight e = s / (V - 1).  The row itself is four rounded operations on
    terms bounded by |H| + |lp[w]| + e |slp|, the sum over the rows and the division a few more (16 u of the same magnitude covers them,
    the fp32 rounding of conf, e and H included).  With raw logits every lp carries the error of lse (three roundings at magnitude |lse|
    plus the relative error of the summed exponentials, (ceil(V / 256) + 12) u) and one rounding of the subtraction."""
    lp = np.asarray(logp64, np.float64)
    S, T, V = lp.shape
    conf, e, H = constants(float(s), V)
    per = -(-V // 256)
    lpw = np.abs(np.take_along_axis(lp, np.asarray(target)[:, :T, None].astype(np.int64), 2)).max()
    sabs = np.abs(lp).sum(2).max()
    mag = abs(H) + lpw + e * sabs
    b = e * (per + 10) * U * sabs + 16 * U * mag
    if lse is not None:
        d_lp = U * (3 * np.abs(lse).max() + per + 12) + U * np.abs(lp).max()
        b += (conf + s * V / (V - 1)) * d_lp                 # lp[w] with weight conf - e, the V terms of slp with weight e each
    return b
