"""The decode rules in the token loop: a Markov stand-in state through `sampling.token_loop` against a host loop over the restatement;
no rules launch and today's bits when no rule is active; eager loop = graph replay; one batch = the images one by one; the golden tiny
models (sGPN greedy, top-k with injected uniforms, Full-GC, bf16-batched at 40 rows) under all four rules against the restatement
applied to the device's own logits along the device's own tokens; the beam refusal; `caption_images` entries."""
import argparse

import numpy as np
import pytest
import torch

import decode_rules_reference as R
from subgc import eval_glue, forced, functions as F_, ops, synthetic
from subgc.decode_rules import DecodeRules, apply_rules_restatement
from subgc.models import sampling

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAP = 1e-3                                                                      # the project's beam-attention convention for a decided arg-max


def _loop_buffers(n, T):
    z = lambda *s, dt=torch.float32: torch.zeros(*s, device=DEV, dtype=dt)
    return dict(seq=z(n, T, dt=torch.long), seqlp=z(n, T), it=z(n, dt=torch.long), unfinished=z(n, dt=torch.int32), counts=z(T, dt=torch.int32))


def _run_token_loop(tab, T, rules, k=0, ut=None):
    n = tab.size(0)
    b = _loop_buffers(n, T)
    st = R.MarkovState(tab)
    bad, stats = sampling.rules_state(rules, n, DEV) if rules.active else (None, None)
    sampling.token_loop(st, b["seq"], b["seqlp"], b["it"], b["unfinished"], b["counts"], k, 0.6, 1.0, ut, rules, bad, stats)
    torch.cuda.synchronize()
    return b["seq"].cpu().numpy(), b["seqlp"].cpu().numpy(), None if stats is None else stats.cpu().numpy(), st.steps


def test_the_markov_cycle_breaks_at_step_five_and_the_loop_equals_the_host_loop():
    n, V, T = 3, 12, 12
    tab = R.markov_tables(n, V, seed=1)
    step = lambda it: tab[np.arange(n), it]
    dev_tab = torch.from_numpy(tab).to(DEV)
    plain, _, none, steps = _run_token_loop(dev_tab, T, DecodeRules())
    assert plain[0].tolist() == [1, 2, 3] * 4 and none is None and steps == T + 1
    for kw in (dict(block_trigrams=1), dict(block_trigrams=1, suppress_unk=1, decoding_constraint=1, block_bad_endings=1, bad_ids=(2, 4))):
        rules = DecodeRules(**kw)
        want, want_lp, want_stats, gap = R.host_loop(step, n, T, rules)
        assert gap >= GAP
        seq, seqlp, stats, _ = _run_token_loop(dev_tab, T, rules)
        np.testing.assert_array_equal(seq, want)
        np.testing.assert_array_equal(stats, want_stats)
        assert np.abs(seqlp - want_lp).max() <= 1e-5
        assert seq[0, :5].tolist() == [1, 2, 3, 1, 2] and seq[0, 5] != 3 and stats[0, 0] >= 1 and stats[0, 3] >= 1
    # rows that end: the end token leads after word 6, so the batch stops early and nothing is written behind the stop
    tab2 = tab.copy()
    tab2[:, 6, 0] = 9.0
    tab2[:, :, 6] += 1.5
    rules = DecodeRules(block_trigrams=1, decoding_constraint=1)
    want, want_lp, want_stats, gap = R.host_loop(lambda it: tab2[np.arange(n), it], n, T, rules)
    seq, seqlp, stats, _ = _run_token_loop(torch.from_numpy(tab2).to(DEV), T, rules)
    assert gap >= GAP and (want == 0).any()
    np.testing.assert_array_equal(seq, want)
    np.testing.assert_array_equal(stats, want_stats)
    assert np.abs(seqlp - want_lp).max() <= 1e-5


def test_no_rule_active_means_no_rules_launch_and_todays_bits(monkeypatch):
    n, V, T = 5, 37, 10
    tab = torch.from_numpy(R.markov_tables(n, V, seed=2)).to(DEV)
    calls = []
    real = ops.decode_rules
    monkeypatch.setattr(ops, "decode_rules", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    g = torch.Generator().manual_seed(4)
    ut = torch.rand(T, n, generator=g).to(DEV)
    for k in (0, 3):
        # today's loop: step -> pick on the raw logits
        b = _loop_buffers(n, T)
        st = R.MarkovState(tab)
        for t in range(T + 1):
            logp = st.step(b["it"], None, normalize=False)
            if t == T:
                break
            ops.decode_pick(logp, k, 0.6, ut[t] if k else None, t, b["seq"], b["seqlp"], b["it"], b["unfinished"], b["counts"][t:t + 1],
                            b["counts"][t - 1:t] if t > 0 else None, raw=True, top_p=1.0)
        torch.cuda.synchronize()
        for rules in (None, DecodeRules(), DecodeRules(trigram_alpha=5.0, bad_ids=(1, 2))):
            c = _loop_buffers(n, T)
            sampling.token_loop(R.MarkovState(tab), c["seq"], c["seqlp"], c["it"], c["unfinished"], c["counts"], k, 0.6, 1.0, ut if k else None, rules)
            torch.cuda.synchronize()
            assert torch.equal(c["seq"], b["seq"]) and torch.equal(c["seqlp"].view(torch.int32), b["seqlp"].view(torch.int32))
            assert torch.equal(c["counts"], b["counts"])
    assert not calls
    _run_token_loop(tab, T, DecodeRules(decoding_constraint=1))
    assert len(calls) == T                                                     # one rules launch per choice when a rule is on


# ---------------------------------------------------------------------------------------------- the golden tiny models
def _model(golden, name, **over):
    import subgc.models as models
    orc, opt, w, batches = R.oracle_case(golden, name)
    opt = dict(opt, **over)
    m = models.setup(argparse.Namespace(**opt))
    m.load_state_dict(w)
    return m.to(DEV).eval(), opt, [{k: v.to(DEV) for k, v in tb.items()} for tb in batches]


def _forced_logits(m, images, tokens):
    """`forced.forced_decode` with every step's logits kept: the decode state driven along `tokens` (per image [rows_i, Tf]); the
    first rows_i candidate sub-graphs of every image in input order (the models here keep every candidate: gpn_nms_thres = 1).
    -> fp32 [Tf, rows, V + 1] on the host."""
    tok_host, counts = forced._token_rows(tokens, len(images))
    rows, Tf = tok_host.shape
    att, obj, pred, rel = ops.stack_first([[im[k] for im in images] for k in ("att_feats", "obj_dist", "pred_dist", "rel_ind")])
    I, N, _ = att.shape
    X2 = m._encode(att, obj, pred, rel).reshape(I * N, m.GCN_dim).contiguous()
    rows_in = [(i, im["gpn_obj_ind"], im["att_masks"], im["gpn_pool_mtx"]) for i, im in enumerate(images)]
    fc, lens, idx, img = (forced._candidate_rows if m.gpn else forced._full_graph_rows)(m, X2, N, rows_in, counts)
    tok = torch.from_numpy(tok_host).to(DEV)
    P = m._decoder_params()
    pr = F_.Prepared(fc, X2, lens, idx, img, N, P, None, None, 1.0)
    st = F_.DecodeState(pr, P, N, False, xt_table=m.xt_gates_table(), fuse_lstm=True, snapshots=m.decode_snapshots(), W16=m.decode_w16(),
                        b16_batched=m.decode_b16_on())
    z = lambda *s, dt=torch.float32: torch.zeros(*s, device=DEV, dtype=dt)
    seq, seqlp, it, unf, cnt = z(rows, Tf, dt=torch.long), z(rows, Tf), z(rows, dt=torch.long), z(rows, dt=torch.int32), z(Tf, dt=torch.int32)
    out = []
    for t in range(Tf):
        logits = st.step(it, None, normalize=False)
        out.append(logits.float().clone())
        forced.forced_pick(logits, tok, t, seq, seqlp, it, unf, cnt[t:t + 1], cnt[t - 1:t] if t > 0 else None, raw=True)
    torch.cuda.synchronize()
    return torch.stack(out).cpu().numpy()


def _check_against_the_restatement(logits, seq, seqlp, stats, rules, what, lp_tol=1e-4, k=0, temp=0.6, u=None):
    """logits [T, rows, V1]: the device's own along its own tokens `seq` [rows, T].  Every live (row, step): the restatement's choice
    on the ruled row = the device token wherever that choice is decided by GAP; seqlp within lp_tol; the counters of the three rules
    equal the host's over the steps the loop ran.  -> (live steps, undecided ones, trigram penalties applied on live rows)."""
    rows, T = seq.shape
    live = np.concatenate([np.ones((rows, 1), bool), np.cumprod(seq[:, :-1] > 0, 1).astype(bool)], 1)
    ran = np.concatenate([[True], live[:, 1:].any(0)])                          # step t runs while a row was unfinished after step t - 1
    host_stats = np.zeros((rows, 4), np.int64)
    near = total = hits = 0
    for t in range(T):
        if not ran[t]:
            break
        lp, ev = apply_rules_restatement(logits[t].astype(np.float64), seq, t, rules, return_events=True)
        host_stats += ev
        for r in np.flatnonzero(live[:, t]):
            total += 1
            hits += int(ev[r, 0])
            tok = int(seq[r, t])
            if k == 0:
                decided, choice, val = R.top2_gap(lp[r]) >= GAP, int(lp[r].argmax()), lp[r].max()
            else:                                                               # AttModel.py:295-303 on the ruled row, inverse CDF at u
                v = lp[r] / temp
                v = v - (v.max() + np.log(np.exp(v - v.max()).sum()))
                order = np.argsort(-v, kind="stable")
                top = v[order[:k]]
                cdf = np.cumsum(np.exp(top - (top.max() + np.log(np.exp(top - top.max()).sum()))))
                j = min(int((u[r, t] >= cdf).sum()), k - 1)
                decided = bool(np.abs(cdf[:-1] - u[r, t]).min() >= GAP and v[order[k - 1]] - v[order[k]] >= GAP
                               and np.diff(-top).min() >= GAP)
                choice, val = int(order[j]), top[j]
            choice = choice if choice > 0 else 0
            if not decided:
                near += 1
                continue
            assert tok == choice, (what, r, t, tok, choice)
            assert np.isfinite(val) and abs(float(seqlp[r, t]) - float(val)) <= lp_tol, (what, r, t, float(seqlp[r, t]), float(val))
    np.testing.assert_array_equal(stats[:, :3], host_stats[:, :3], err_msg=what)
    print(f"{what}: {total} live steps, {near} undecided at gap {GAP} ({100.0 * near / max(total, 1):.2f} %), {hits} trigram penalties on live rows, "
          f"device counters {stats.sum(0).tolist()}")
    assert near <= 0.05 * total and stats[:, 0].sum() >= hits
    return total, near, hits


def _opt(V1, **kw):
    r = R.all_rules(V1)
    return dict(sample_max=1, beam_size=1, block_trigrams=1, suppress_unk=1, decoding_constraint=1, block_bad_endings=1,
                bad_ending_ids=list(r.bad_ids), **kw), r


@pytest.mark.parametrize("name", ["subgc", "fullgc"])
def test_greedy_decode_of_the_golden_models_under_all_rules(golden, name):
    """CPU oracle alone (test_decode_rules_cpu.py): 0 of 481 (subgc) / 0 of 13 (fullgc) live steps below the gap."""
    m, opt, images = _model(golden, name)
    eo, rules = _opt(opt["vocab_size"] + 1)
    hold = {"skip_att": True}
    m.sample_images(images, opt=eo, batch_out=hold)
    seq, seqlp, stats, bounds = hold["seq"].cpu().numpy(), hold["seqlp"].cpu().numpy(), hold["rule_stats"].cpu().numpy(), hold["bounds"]
    assert stats.shape == (seq.shape[0], 4) and torch.equal(m.rule_stats, hold["rule_stats"])
    logits = _forced_logits(m, images, [seq[a:b] for a, b in zip(bounds, bounds[1:])])
    assert _check_against_the_restatement(logits, seq, seqlp, stats, rules, f"{name} greedy")[2] >= 1
    # the rules did something: the plain decode differs
    plain = {"skip_att": True}
    m.sample_images(images, opt=dict(sample_max=1, beam_size=1), batch_out=plain)
    assert "rule_stats" not in plain and m.rule_stats is None and not torch.equal(plain["seq"], hold["seq"])


def test_topk_decode_with_injected_uniforms_under_all_rules(golden):
    m, opt, images = _model(golden, "subgc", use_topk_sampling=1, the_k=3, topk_temp=0.6)
    eo, rules = _opt(opt["vocab_size"] + 1)
    T, hits = m.seq_length, 0
    for i, im in enumerate(images[:2]):
        n = int(im["gpn_obj_ind"].size(1) * im["gpn_obj_ind"].size(2))
        u = torch.rand(n, T, generator=torch.Generator().manual_seed(50 + i)).to(DEV)
        tb = {k: v for k, v in im.items()}
        ret = m._sample(*synthetic.sample_args(tb), opt=eo, uniforms=u)
        seq, seqlp, stats = ret[0].cpu().numpy(), ret[1].cpu().numpy(), m.rule_stats.cpu().numpy()
        assert seq.shape[0] == n
        logits = _forced_logits(m, [im], [seq])
        hits += _check_against_the_restatement(logits, seq, seqlp, stats, rules, f"subgc top-3 image {i}", k=3, temp=0.6, u=u.cpu().numpy())[2]
    assert hits >= 1


@pytest.mark.parametrize("rows", [1, 10])
def test_eager_loop_equals_graph_replay_bit_for_bit(golden, rows):
    m, opt, images = _model(golden, "subgc", gpn_max_subg=rows)
    eo, rules = _opt(opt["vocab_size"] + 1)
    im = images[2]                                                              # 12 candidate sub-graphs
    args = synthetic.sample_args(im)
    g = m._sample(*args, opt=eo)
    gs = m.rule_stats.clone()
    assert g[0].size(0) == rows and any(isinstance(v, sampling._GraphedLoop) and v.rules is not None for v in m._graph_cache.values())
    g2 = m._sample(*args, opt=eo)                                               # a second replay: the counters start from zero again
    assert torch.equal(m.rule_stats, gs) and torch.equal(g2[0], g[0])
    m.decode_hipgraph = False
    e = m._sample(*args, opt=eo)
    es = m.rule_stats
    torch.cuda.synchronize()
    assert torch.equal(e[0], g[0]) and torch.equal(e[1].view(torch.int32), g[1].view(torch.int32)) and torch.equal(es, gs)
    assert gs[:, :3].sum() > 0
    # the rules key the cache: the plain decode replays another graph and differs
    m.decode_hipgraph = True
    p = m._sample(*args, opt=dict(sample_max=1, beam_size=1))
    assert m.rule_stats is None and not torch.equal(p[0], g[0])


def test_one_batch_of_three_images_equals_the_images_one_by_one(golden):
    m, opt, images = _model(golden, "subgc")
    eo, rules = _opt(opt["vocab_size"] + 1)
    whole = m.sample_images(images, opt=eo)
    for i, im in enumerate(images):
        one = m.sample_images([im], opt=eo)[0]
        assert torch.equal(one[0], whole[i][0]), i
        assert float((one[1] - whole[i][1]).abs().max()) <= 1e-4
        single = m._sample(*synthetic.sample_args(im), opt=eo)
        assert torch.equal(single[0], whole[i][0]), i


def test_bf16_batched_decode_at_forty_rows_under_all_rules(golden):
    """bf16 storage with decode_b16_batched = 1: the same checks, log-probabilities at the bf16 tolerance of SURVEY 8(c) (5e-2)."""
    m, opt, _ = _model(golden, "subgc", compute_dtype="bf16", decode_b16_batched=1)
    images = [{k: v.to(DEV) for k, v in synthetic.make_test_batch(10, D=opt["att_feat_size"], seed=940 + i, fc_size=opt["att_feat_size"],
                                                                   node_pool=None).items()} for i in range(2)]
    eo, rules = _opt(opt["vocab_size"] + 1)
    hold = {"skip_att": True}
    m.sample_images(images, opt=eo, batch_out=hold)
    seq, seqlp, stats, bounds = hold["seq"].cpu().numpy(), hold["seqlp"].cpu().numpy(), hold["rule_stats"].cpu().numpy(), hold["bounds"]
    assert seq.shape[0] == 40
    logits = _forced_logits(m, images, [seq[a:b] for a, b in zip(bounds, bounds[1:])])
    assert _check_against_the_restatement(logits, seq, seqlp, stats, rules, "subgc bf16-batched, 40 rows", lp_tol=5e-2)[2] >= 1


def test_beam_search_refuses_the_three_rules_and_keeps_its_repeat_ban(golden):
    m, opt, images = _model(golden, "subgc")
    args = synthetic.sample_args(images[0])
    for name in ("block_trigrams", "block_bad_endings", "suppress_unk"):
        with pytest.raises(ValueError, match=f"^{name} = 1 with beam_size = 2"):
            m._sample(*args, opt={"beam_size": 2, name: 1, "bad_ending_ids": [1]})
        with pytest.raises(ValueError, match=f"^{name} = 1 with beam_size = 2"):
            m.sample_images(images, opt={"beam_size": 2, name: 1, "bad_ending_ids": [1]})
    a = m._sample(*args, opt={"beam_size": 2, "decoding_constraint": 1})
    assert a[0].size(0) > 0 and m.rule_stats is None


def test_caption_images_hands_the_counters_to_every_entry(golden):
    m, opt, images = _model(golden, "subgc")
    V1 = opt["vocab_size"] + 1
    ix = {str(i): f"w{i}" for i in range(V1)}
    ix.update({"1": "with", "2": "the", "3": "a", str(V1 - 2): "of"})
    infos = [{"id": 100 + i} for i in range(len(images))]
    kw = dict(sample_max=1, beam_size=1, block_trigrams=1, suppress_unk=1, decoding_constraint=1, block_bad_endings=1)
    preds = eval_glue.caption_images(m, images, infos, ix, kw)
    hold = {"skip_att": True}
    m.sample_images(images, opt=dict(kw, bad_ending_ids=[1, 2, 3, V1 - 2]), batch_out=hold)
    seq, stats, bounds = hold["seq"].cpu().numpy(), hold["rule_stats"].cpu().numpy(), hold["bounds"]
    for e, a, b in zip(preds, bounds, bounds[1:]):
        assert e["rule_stats"].shape == (b - a, 4) and e["rule_stats"].dtype == np.int32
        want = {tuple(seq[a + r].tolist()): stats[a + r].tolist() for r in range(b - a)}
        for cap, st in zip(e["caption"], e["rule_stats"]):
            toks = tuple(int(w[1:]) if w.startswith("w") else {"with": 1, "the": 2, "a": 3, "of": V1 - 2}[w] for w in cap.split())
            match = [v for k_, v in want.items() if tuple(x for x in k_ if x > 0)[:len(toks)] == toks and sum(1 for x in k_ if x > 0) == len(toks)]
            assert st.tolist() in match
        assert not any(cap.split()[-1] in ("with", "the", "a", "of") for cap in e["caption"] if cap and len(cap.split()) < m.seq_length)
    plain = eval_glue.caption_images(m, images, infos, ix, dict(sample_max=1, beam_size=1, remove_bad_endings=1))
    assert all("rule_stats" not in e for e in plain)
