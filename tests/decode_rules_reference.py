"""What the decode-rule tests share, without a GPU: the error bound of DESIGN 4.W (coded once, here), the histories of the kernel cases,
a Markov stand-in decode state with its host loop over the restatement, and the CPU oracle driven step by step under the rules."""
import math

import numpy as np
import torch

from subgc.decode_rules import DecodeRules, apply_rules_restatement, trigram_counts

U = 2.0 ** -24
KINDS = ("no match", "one match", "multiplicity 3", "pair at t-3", "zeros", "id V-1")
EACH_AND_ALL = (dict(block_trigrams=1), dict(suppress_unk=1), dict(decoding_constraint=1), dict(block_bad_endings=1),
                dict(block_trigrams=1, suppress_unk=1, decoding_constraint=1, block_bad_endings=1))


def bad_ids_for(V):
    return (0, 2, 5, V - 1)


def lp_bound(V, d, log_s, lp):
    """|lp - exact| <= u (|d| + |lp| + 2 |ln S| + ln V + CH + 10), first order, with 0.1 % for the higher orders
    (arrays or numbers)."""
    ch = (V + 255) // 256
    return 1.001 * U * (np.abs(d) + np.abs(lp) + 2 * np.abs(log_s) + math.log(V) + ch + 10)


def ruled_bound(x, h, t, rules):
    """DESIGN 4.W for one row: per column the bound of the fp32 ruled value against the fp64 restatement -- the log-softmax term of
    `lp_bound`, plus one rounding of the product c * p and one of the sum on a counted column, plus one rounding of the subtraction on
    the UNK column.  (-inf columns are compared by position, not by value.)"""
    x = np.asarray(x, np.float64)
    V = x.size
    d = x - x.max()
    log_s = math.log(np.exp(d).sum())
    lp = d - log_s
    b = lp_bound(V, d, log_s, lp)
    val = lp.copy()
    pen = float(rules.trigram_pen)
    if rules.block_trigrams and np.isfinite(pen):
        for col, c in trigram_counts(h, t, V).items():
            prod = c * pen
            val[col] = lp[col] + prod
            b[col] += 1.001 * U * (abs(prod) + abs(val[col]))
    if rules.suppress_unk and np.isfinite(val[V - 1]):
        val[V - 1] -= 1000.0
        b[V - 1] += 1.001 * U * abs(val[V - 1])
    return b


def history(kind, T, t, V, salt=0):
    """One history row [T] int64 of the named kind for step t; entries from t on are never read and hold V - 1."""
    h = np.full(T, V - 1, np.int64)
    i = np.arange(T)
    if kind == "no match":
        h[:t] = 1 + (i[:t] + salt) % 3
        if t >= 2:
            h[t - 2:t] = (5, 6)
    elif kind == "one match":
        h[:t] = 1 + (i[:t] + salt) % 3
        if t >= 2:
            h[t - 2:t] = (5, 6)
        if t >= 5:
            h[0:3] = (5, 6, 4)
        elif t == 4:                                        # 5 6 5 6: start 0 matches, start 1 does not
            h[:4] = (5, 6, 5, 6)
        elif t == 3:                                        # the only start is j = 0: a a a
            h[:3] = 4
    elif kind == "multiplicity 3":
        h[:t] = 4 + (i[:t] + salt) % 3                       # 4 5 6 4 5 6 ...: the last pair came before, always in front of one column
    elif kind == "pair at t-3":
        h[:t] = 1 + (i[:t] + salt) % 3
        if t >= 3:
            h[t - 3:t] = 3
            if t >= 4:
                h[t - 4] = 6
    elif kind == "zeros":
        h[:t] = 0
    elif kind == "id V-1":
        h[:t] = np.where((i[:t] + salt) % 2 == 0, V - 1, 2)
    else:
        raise KeyError(kind)
    return h


def histories(n, T, t, V, first=0):
    """[n, T]: row r holds kind (first + r) % 6."""
    return np.stack([history(KINDS[(first + r) % len(KINDS)], T, t, V, salt=r // len(KINDS)) for r in range(n)])


def top2_gap(row):
    s = np.sort(row[np.isfinite(row)])
    return float(s[-1] - s[-2]) if s.size > 1 else float("inf")


# ------------------------------------------------------------------------------------------------ the Markov stand-in
def markov_tables(n, V, seed=0):
    """fp32 [n, V, V]: row r's logits after previous token p are tables[r, p].  Row 0 makes plain greedy repeat 1 2 3 1 2 3 ...: the
    cycle's next word leads by 1.0 (less than one trigram penalty, 1.386), so block_trigrams breaks it at step 5; the other rows are
    noise around their own cycles.  No end token wins early: column 0 sits low."""
    g = np.random.default_rng(seed)
    tab = (g.standard_normal((n, V, V)) * 0.5).astype(np.float32)
    tab[:, :, 0] -= 6.0
    nxt = {0: 1, 1: 2, 2: 3, 3: 1}
    for r in range(n):
        for p in range(V):
            q = nxt.get(p, 1 + (p + r) % (V - 1))
            tab[r, p, q] += 4.0
            tab[r, p, 1 + (q + 2) % (V - 1)] += 3.0
    tab[0, :, :] = -4.0
    for p, q in nxt.items():
        tab[0, p, q] = 2.0
    tab[0, :, 4] = 1.0                                                        # the runner-up everywhere on row 0
    tab[0, 4, 5] = 2.0
    tab[0, 5, 1] = 2.0
    return tab


class MarkovState:
    """A stand-in decode state for `sampling.token_loop`: the step's logits depend on the previous token alone.  `step` returns a fresh
    fp32 [n, V] tensor (the rules act in place on it)."""

    def __init__(self, tables):
        self.tab = tables                                                       # device fp32 [n, V, V]
        self.rows = torch.arange(tables.size(0), device=tables.device)
        self.steps = 0

    def step(self, it, att_out=None, normalize=False):
        self.steps += 1
        return self.tab[self.rows, it].contiguous()


def host_loop(step_logits, n, T, rules):
    """The greedy token loop on the host over the restatement: step_logits(it [n] int64) -> [n, V] logits.  -> (seq [n, T], seqlp
    fp64 [n, T], stats [n, 4], the smallest ruled top-2 gap met); the rules' counters run on every row while the loop runs, as the
    device's do."""
    seq, lps, stats = np.zeros((n, T), np.int64), np.zeros((n, T)), np.zeros((n, 4), np.int64)
    it, unf, worst = np.zeros(n, np.int64), np.ones(n, bool), float("inf")
    for t in range(T):
        if t > 0 and not unf.any():
            break
        lp, ev = apply_rules_restatement(step_logits(it), seq, t, rules, return_events=True)
        stats += ev
        tok = lp.argmax(1)
        worst = min([worst] + [top2_gap(lp[r]) for r in range(n) if (t == 0 or unf[r])])
        unf = (tok > 0) if t == 0 else unf & (tok > 0)
        it = tok * unf
        seq[:, t] = it
        lps[:, t] = lp[np.arange(n), tok]
    return seq, lps, stats, worst


# ------------------------------------------------------------------------------------------------ the CPU oracle under the rules
def oracle_ruled_greedy(orc, args, rules, T=None):
    """The oracle's `sample` loop (oracle/subgc_oracle.py, beam_size == 1, greedy) with the restatement between `core_step` and the
    choice.  args: (fc_feats, att_feats, att_masks, obj_dist, rel_ind, pred_dist, gpn_obj_ind, gpn_pool_mtx).
    -> (seq [n, T], seqlp [n, T], stats [n, 4], per live (row, step) the ruled top-2 gaps as a flat array, the trigram penalties
    applied on live rows -- a finished row's 0 0 0 history counts in `stats` but shows nothing)."""
    from oracle import subgc_oracle as O
    P, cfg = orc.P, orc.cfg
    cfg.sample_mode = True
    with torch.no_grad():
        _, score, att, fc, m, keep = O._encode(P, cfg, args, orc.buffers, False, None, None, "stable")
        n = fc.size(0)
        state = O._zeros_state(n, cfg.R, fc)
        f, v, u, mk = O.prepare_feature(P, cfg, fc, att, m, False)
        T = cfg.seq_length if T is None else T
        seq, lps, stats = np.zeros((n, T), np.int64), np.zeros((n, T)), np.zeros((n, 4), np.int64)
        it, unf, gaps, live_hits = torch.zeros(n, dtype=torch.long), np.ones(n, bool), [], 0
        for t in range(T):
            logp, state, _ = O.core_step(P, cfg, it, f, v, u, mk, state, False)
            lp, ev = apply_rules_restatement(logp.numpy(), seq, t, rules, return_events=True)
            stats += ev
            tok = lp.argmax(1)
            live_hits += int(ev[:, 0].sum() if t == 0 else ev[unf, 0].sum())
            gaps += [top2_gap(lp[r]) for r in range(n) if (t == 0 or unf[r])]
            unf = (tok > 0) if t == 0 else unf & (tok > 0)
            tok = tok * unf
            seq[:, t] = tok
            lps[:, t] = lp[np.arange(n), lp.argmax(1)]
            it = torch.from_numpy(tok)
            if not unf.any():
                break
    return seq, lps, stats, np.asarray(gaps), live_hits


def oracle_case(golden, name):
    """(oracle, per-image args) of the forced-decode fixture's tiny model `name` with a sharpened logit layer (x 3: the tiny random
    models are near-uniform otherwise and never repeat a trigram)."""
    import argparse
    import grounding_gt_golden as GG
    from oracle import subgc_oracle as O
    from subgc import synthetic
    fmeta, _ = GG.load_forced()
    opt = dict(fmeta["cases"][name]["opt"])
    opt.setdefault("obj_name_path", None); opt.setdefault("rel_name_path", None)
    opt.update(caption_model="topdown", gpn_nms_thres=1.0, gpn_max_subg=64, test_LSTM=1)
    w = {k: torch.from_numpy(v).clone() for k, v in golden("subgc_beam" if name == "subgc" else "fullgc_train").group("weights").items()}
    sharpen(w)
    orc = O.Oracle(argparse.Namespace(**opt), w)
    batches = [synthetic.make_test_batch(i["M"], D=opt["att_feat_size"], seed=i["seed"], fc_size=opt["att_feat_size"], node_pool=i["pool"])
               for i in fmeta["cases"][name]["images"]]
    return orc, opt, w, batches


def sharpen(w):
    w["logit.weight"] = w["logit.weight"] * 3.0
    w["logit.bias"] = w["logit.bias"] * 3.0
    return w


def all_rules(V1):
    return DecodeRules(block_trigrams=1, suppress_unk=1, decoding_constraint=1, block_bad_endings=1, bad_ids=(1, 2, 3, V1 - 2))
