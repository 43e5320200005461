"""Shared by the self-critical tests: the fixtures the reference's own RewardCriterion and COCO scorers wrote
(tests/golden/make_golden_self_critical.py), fp64 numpy restatements of what include/subgc_selfcritical_hip.h declares (the criterion and
its mask, the end-token rule of the scored rows, the inverse-CDF pick) and the error bounds of DESIGN 4.N as functions of a test's inputs.
test_self_critical_cpu.py ties the restatements to the fixtures; the GPU tests then use them as the reference on other shapes."""
import json
import os

import numpy as np

import accuracy_golden as AG

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = 2.0 ** -24                                     # unit roundoff of fp32
LANES = 256                                        # one workgroup of 256 lanes sums: per-lane sequence, six tree levels, four waves


def load_case():
    with open(os.path.join(GOLDEN, "self_critical_meta.json")) as f:
        meta = json.load(f)
    with np.load(os.path.join(GOLDEN, "self_critical_case.npz")) as z:
        return meta, {k: z[k] for k in z.files}


def load_train():
    with np.load(os.path.join(GOLDEN, "self_critical_train.npz")) as z:
        return {k: z[k] for k in z.files}


def per_image(rows, cap_off):
    return [rows[cap_off[j]:cap_off[j + 1]] for j in range(len(cap_off) - 1)]


# ------------------------------------------------------------------------------------------------------------------ the criterion
def mask_of(seq):
    """misc/utils.py:98-99: m[s, 0] = 1, m[s, t] = seq[s, t - 1] > 0."""
    seq = np.asarray(seq)
    m = np.ones(seq.shape, np.float64)
    m[:, 1:] = seq[:, :-1] > 0
    return m


def criterion64(inp, seq, reward, gpn=None, dloss=1.0):
    """fp64 RewardCriterion on gathered log-probabilities [S, T] -> (loss, d input, d gpn_loss or None)."""
    x, r, m = np.asarray(inp, np.float64), np.asarray(reward, np.float64), mask_of(seq)
    den = m.sum()
    term = -x * r
    dg = None
    if gpn is not None:
        g = np.asarray(gpn, np.float64)[:, None]
        term = term + g * np.exp(r)
        dg = dloss * (np.exp(r) * m).sum(1) / den
    return float((term * m).sum() / den), -dloss * r * m / den, dg


def terms_abs(inp, seq, reward, gpn=None):
    x, r, m = np.asarray(inp, np.float64), np.asarray(reward, np.float64), mask_of(seq)
    a = np.abs(x * r) * m
    b = np.zeros_like(a) if gpn is None else np.abs(np.asarray(gpn, np.float64)[:, None] * np.exp(r)) * m
    return a, b, m.sum()


def sum_depth(n):
    """Roundings a term can pass through in the fixed-order sum of n terms: its lane's sequence, six tree levels, four waves."""
    return -(-n // LANES) + 10


def loss_bound(inp, seq, reward, gpn=None):
    """|loss_fp32 - loss_fp64| of the stand-alone criterion.  A term -x r m carries two roundings (the product, and the mask factor, which
    is exact); with gpn_loss the term g exp(r) adds the error of expf (1 ulp = 2 u), its product and the addition: 5 u of its magnitude
    covers them.  The sum of n terms adds (ceil(n / 256) + 10) u sum|term|, the division one more rounding; den is an exact integer."""
    a, b, den = terms_abs(inp, seq, reward, gpn)
    mag = (a + b).sum()
    loss = abs(criterion64(inp, seq, reward, gpn)[0])
    return ((2 * a + 5 * b).sum() * U + sum_depth(a.size) * U * mag) / den + U * loss


def log_softmax64(x):
    x = np.asarray(x, np.float64)
    mx = x.max(-1, keepdims=True)
    return x - (mx + np.log(np.exp(x - mx).sum(-1, keepdims=True)))


def fused64(lp64, target, mask, reward, dloss=1.0, den=None):
    """fp64 RewardCriterion on the decoder's rows: lp64 [S, T, V] log-probabilities, target / mask / reward [S, T] ->
    (loss, dlogits [S, T, V]); `den` replaces the mask sum."""
    lp = np.asarray(lp64, np.float64)
    w = np.asarray(target).astype(np.int64)
    m, r = np.asarray(mask, np.float64), np.asarray(reward, np.float64)
    d = m.sum() if den is None else float(den)
    lpw = np.take_along_axis(lp, w[:, :, None], 2)[:, :, 0]
    onehot = np.zeros(lp.shape)
    np.put_along_axis(onehot, w[:, :, None], 1.0, 2)
    g = dloss * r * m / d
    return float(-(r * m * lpw).sum() / d), g[:, :, None] * (np.exp(lp) - onehot)


def fused_loss_bound(lp64, target, mask, reward, lse64=None, den=None):
    """|loss_fp32 - loss_fp64| of the fused forward.  Each term -lp r m carries two roundings; on raw logits lp = x[w] - lse also carries
    the error of lse, u (3 |lse| + ceil(V / 256) + 12), and the rounding of the subtraction, all weighted by |r|.  The fixed-order sum
    and the division as in `loss_bound`."""
    lp = np.asarray(lp64, np.float64)
    S, T, V = lp.shape
    w = np.asarray(target).astype(np.int64)
    m, r = np.asarray(mask, np.float64), np.asarray(reward, np.float64)
    d = m.sum() if den is None else float(den)
    lpw = np.abs(np.take_along_axis(lp, w[:, :, None], 2)[:, :, 0])
    term = lpw * np.abs(r) * m
    b = 2 * U * term.sum() + sum_depth(S * T) * U * term.sum()
    if lse64 is not None:
        d_lp = U * (3 * np.abs(np.asarray(lse64)).reshape(S, T) + (-(-V // 256)) + 12) + U * lpw
        b += (d_lp * np.abs(r) * m).sum()
    return b / d + U * abs(fused64(lp, target, mask, reward, den=den)[0])


# ------------------------------------------------------------------------------------------------------------------ the scored rows
def eos_rows(seq2, eos_id):
    """subgc_sc_prepare's scored rows [2S, T + 1]: the first 0 of a row becomes eos_id, everything behind it 0; eos_id = 0 copies."""
    seq2 = np.asarray(seq2)
    out = np.zeros((seq2.shape[0], seq2.shape[1] + 1), np.int64)
    for i, row in enumerate(seq2):
        if eos_id <= 0:
            out[i, :-1] = row
            continue
        for t, w in enumerate(row):
            if w == 0:
                out[i, t] = eos_id
                break
            out[i, t] = w
    return out


def replay_labels(seq2):
    seq2 = np.asarray(seq2)
    S, T = seq2.shape[0] // 2, seq2.shape[1]
    lab = np.zeros((S, T + 2), np.int64)
    lab[:, 1:T + 1] = seq2[:S]
    m = np.zeros((S, T + 1))
    m[:, :T] = mask_of(seq2[:S])
    return lab, m


def ids_with_eos(row, eos_id):
    """A 0-padded row -> the id list the scorers see: the words before the first 0, then the end token when there is one."""
    out = []
    for w in row:
        if int(w) == 0:
            if eos_id > 0:
                out.append(int(eos_id))
            break
        out.append(int(w))
    return out


def restate_scores(cand, cand_img, refs, eos_id):
    """fp64 (BLEU-4, CIDEr) of every candidate row against its image's references with the document frequencies of exactly the images given
    (tests/accuracy_golden.py's restatement of the COCO scorers on id lists)."""
    ref_ids = [[ids_with_eos(r, eos_id) for r in caps] for caps in refs]
    cands = [ids_with_eos(r, eos_id) for r in cand]
    rows = AG.restate_rows(cands, list(range(len(cands) + 1)), [int(j) for j in cand_img], ref_ids)
    vals = np.array([v for _, v in rows], np.float64)
    return vals[:, 3], vals[:, 4]


# ------------------------------------------------------------------------------------------------------------------ the pick
def cdf64(logits, temp=1.0):
    x = np.asarray(logits, np.float64) / temp
    e = np.exp(x - x.max())
    return np.cumsum(e) / e.sum()


def inv_cdf_pick(logits, u, temp=1.0):
    """pick = #{c : u >= cdf_c}, clamped to V - 1, on the fp64 CDF in column order."""
    c = cdf64(logits, temp)
    return int(min(np.count_nonzero(u >= c), len(c) - 1))


def boundary_distance(logits, u, temp=1.0):
    return float(np.abs(cdf64(logits, temp) - u).min())
