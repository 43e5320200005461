"""Beam search under decode rules on the device (`eval_kwargs["beam_rules"]`): `subgc_decode_rules` under the shifted
history layout of `DeviceSearch` (bit for bit against the unshifted call, and against the fp64 restatement within DESIGN 4.W), the
stand-in decoder of beam_rules_fake through `DeviceSearch` against the host `search` driven through the same launches, the golden tiny
models (sGPN beam 2, Full-GC beam 3, diverse 4 x 2) -- host bookkeeping = device bookkeeping, eager = graph replay, the winners' log-probs
against the restatement on forced-decode logits, the counters, the attention of the winners -- `caption_images` in one process and
sharded over two ranks, and the refusals.

Tolerances: 1e-4 on fp32 log-probabilities (the project's), 5e-2 in the bf16-batched regime, 1e-5 on attention rows against
the forced decode (soft-max outputs <= 1 from the same kernels on other row counts: a few ulps of 1, the 1e-6 level; 0.0 seen);
everything else is bit for bit."""
import math

import numpy as np
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

import beam_rules_fake as FK
import decode_rules_reference as R
from subgc import beam, eval_glue, forced, ops, synthetic
from subgc import functions as F_
from subgc.decode_rules import DecodeRules, apply_rules_restatement, sequence_events
from subgc.models import sampling
from test_beam_device_gpu import prepared
from test_decode_rules_loop_gpu import _forced_logits, _model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_SUB, N, LENS = 3, 5, (5, 2, 4)
BAD = (1, 2, 3)
bits = lambda a: np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------ 1. the kernel under shifted histories
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("V", [8, 37, 9488])
def test_rules_kernel_under_a_minus_one_prefix(V, pad):
    Th, ld = 10, V + pad
    rng = np.random.default_rng(V + pad)
    bad = R.bad_ids_for(V)
    d_bad = torch.tensor(bad, dtype=torch.int32, device=DEV)
    fired = banned = 0
    for n in (1, 5):
        x = (rng.standard_normal((n, ld)) * 3).astype(np.float32)
        for alpha in (2.0, math.inf):
            rules = DecodeRules(block_trigrams=1, trigram_alpha=alpha, block_bad_endings=1, bad_ids=bad)
            for t in range(6):
                h = R.histories(n, Th, t, V, first=t)
                h[:, t:] = -1                                                    # (never read)

                def launch(hist, step):
                    buf = torch.from_numpy(x).to(DEV)
                    ops.decode_rules(buf[:, :V], torch.from_numpy(hist).to(DEV), step, rules.flags, rules.trigram_pen, d_bad, None, None)
                    return buf.cpu().numpy()
                base = launch(h, t)
                np.testing.assert_array_equal(bits(base[:, V:]), bits(x[:, V:]))      # the padding columns are not touched
                for g in (0, 1, 2):
                    sh = np.full((n, Th), -1, np.int64)
                    sh[:, g:g + t] = h[:, :t]
                    np.testing.assert_array_equal(bits(launch(sh, t + g)), bits(base), err_msg=f"n {n} alpha {alpha} t {t} prefix {g}")
                plain = torch.from_numpy(x).to(DEV)
                ops.decode_rules(plain[:, :V], torch.from_numpy(h).to(DEV), t, 0, 0.0, None, None, None)
                plain = plain.cpu().numpy()[:, :V]
                for r in range(n):
                    want = apply_rules_restatement(x[r, :V].astype(np.float64), h[r], t, rules)
                    want0 = apply_rules_restatement(x[r, :V].astype(np.float64), h[r], t, DecodeRules())
                    got = base[r, :V]
                    np.testing.assert_array_equal(np.isneginf(got), np.isneginf(want))
                    np.testing.assert_array_equal(bits(got) != bits(plain[r]), want != want0)      # the same columns are altered
                    fin = np.isfinite(want)
                    assert (np.abs(got[fin] - want[fin]) <= R.ruled_bound(x[r, :V], h[r], t, rules)[fin]).all(), (n, alpha, t, r)
                    fired += int((want != want0).sum())
                    banned += int(np.isneginf(want[0]))
    assert fired > 0 and banned > 0


# ------------------------------------------------------------------------------------------------ 2. the stand-in through DeviceSearch
def _fake_opt(beam_size, G, alpha):
    return dict(beam_size=beam_size, group_size=G, diversity_lambda=0.5,
                beam_rules=dict(block_trigrams=1, trigram_alpha=alpha, block_bad_endings=1, bad_ending_ids=list(BAD)))


def _same_beams(da, db, stats=True):
    assert len(da) == len(db)
    for x, y in zip(da, db):
        assert len(x) == len(y)
        for p, q in zip(x, y):
            assert torch.equal(p["seq"], q["seq"]) and torch.equal(p["logps"].view(torch.int32), q["logps"].view(torch.int32))
            assert p["p"] == q["p"] and p["unaug_p"] == q["unaug_p"]
            if stats:
                np.testing.assert_array_equal(p["rule_stats"], q["rule_stats"])


@pytest.mark.parametrize("alpha", [2.0, math.inf])
@pytest.mark.parametrize("T", [6, 10])
@pytest.mark.parametrize("beam_size,G", FK.SHAPES)
def test_device_search_equals_the_host_search_through_the_same_launches(beam_size, G, T, alpha):
    salt, bd, boost = 1, beam_size // G, 2.0
    opt = _fake_opt(beam_size, G, alpha)
    rules = DecodeRules.from_beam_options(opt)
    ds = beam.DeviceSearch(FK.DeviceEngine(N_SUB, beam_size, LENS, N, salt, DEV, boost), T, opt, return_att=True, rules=rules)
    ds.loop(fresh_tables=True)
    seq, seqlp, done, att = ds.collect()
    h_seq, h_lp, h_done = beam.search(FK.DeviceEngine(N_SUB, beam_size, LENS, N, salt, DEV, boost), T, opt, rules=rules)
    assert torch.equal(seq, h_seq) and torch.equal(seqlp.view(torch.int32), h_lp.view(torch.int32))
    _same_beams(done, h_done)
    # the plain search of this decoder is another search: the rules acted
    p_seq, _, p_done = beam.search(FK.DeviceEngine(N_SUB, beam_size, LENS, N, salt, DEV, boost), T, {k: v for k, v in opt.items() if k != "beam_rules"})
    assert "rule_stats" not in p_done[0][0]
    if T == 10:
        assert not torch.equal(p_seq, seq)
    # the maintained history = the search's own tables re-laid: word w of group g in column g + w, -1 elsewhere
    hist, tb = ds.hist[ds.hist_now].cpu().numpy(), ds.tb.seq.cpu().numpy()
    want = np.full((N_SUB, G, bd, T + G - 1), -1, np.int64)
    for g in range(G):
        want[:, g, :, g:g + T] = tb[:, g].transpose(0, 2, 1)
    np.testing.assert_array_equal(hist, want.reshape(N_SUB * beam_size, T + G - 1))
    for s in range(N_SUB):
        for k, b in enumerate(done[s]):
            words = b["seq"].tolist()
            L = FK.length_of(words, T)
            if alpha == math.inf:
                assert not FK.repeats_trigram(words, L), (s, words)
            assert not (0 in words and words.index(0) > 0 and words[words.index(0) - 1] in BAD), (s, words)
            np.testing.assert_array_equal(b["rule_stats"], sequence_events(words, L, rules))
    # the ancestry gather is untouched: the attention code of every kept beam follows its own tokens
    for g in range(G):
        for r in range(bd):
            _, _, d2, a2 = ds.collect((g, r))
            AL = a2["AL"].cpu().numpy()
            for s in range(N_SUB):
                words = d2[s][g * bd + r]["seq"].tolist()
                L = int(a2["len"][s])
                for w in range(L):
                    np.testing.assert_array_equal(AL[w, s], FK.code(s, FK.BOS if w == 0 else words[w - 1], LENS[s], N))
                assert not AL[L:, s].any()
    # a second search on the same buffers (what a graph replay does) starts from a clean history
    ds.eng.st.reset()
    ds.loop()
    again = ds.collect()
    assert torch.equal(again[0], seq) and torch.equal(again[1].view(torch.int32), seqlp.view(torch.int32))
    np.testing.assert_array_equal(ds.hist[ds.hist_now].cpu().numpy(), hist)


@pytest.mark.parametrize("beam_size,G", [(2, 1), (4, 2)])
def test_debug_bounds_mode_accepts_the_minus_one_columns(beam_size, G):
    """G = 1 forks and writes the history through `gather_rows` / `copy2d` on 4-byte float views (the words of an int64 -1 are NaN bit
    patterns there); G = 2 writes the column with `torch.where`.  Both under the entry points' debug checks."""
    opt = _fake_opt(beam_size, G, 2.0)
    rules = DecodeRules.from_beam_options(opt)
    run = lambda: beam.search_device(FK.DeviceEngine(N_SUB, beam_size, LENS, N, 0, DEV), 6, opt, rules=rules)
    want = run()
    with ops.debug_bounds():
        got = run()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))


# ------------------------------------------------------------------------------------------------ 3. the golden tiny models
CASES = {"sgpn_beam2": ("subgc", 2, 1), "fullgc_beam3": ("fullgc", 3, 1), "div_beam4": ("subgc", 4, 2)}


def _rules_opt(V1, beam_size, G, **kw):
    return dict(sample_max=1, beam_size=beam_size, group_size=G, diversity_lambda=0.5,
                beam_rules=dict(block_trigrams=1, trigram_alpha=2.0, block_bad_endings=1, bad_ending_ids=[1, 2, 3, V1 - 2]), **kw)


def _prepared(m, images):
    """The decode batch of `images` as `sample_images` builds it: the kept sub-graphs (sGPN), or one full-graph row per image (Full-GC)."""
    if m.gpn:
        return prepared(m, images)
    att, obj, pred, rel = ops.stack_first([[im[k] for im in images] for k in ("att_feats", "obj_dist", "pred_dist", "rel_ind")])
    I, Nn, _ = att.shape
    X2 = m._encode(att, obj, pred, rel).reshape(I * Nn, m.GCN_dim).contiguous()
    w = sampling.full_graph_rows(m, X2, Nn, [(i, im["gpn_obj_ind"], im["att_masks"], im["gpn_pool_mtx"]) for i, im in enumerate(images)]).whole
    P = m._decoder_params()
    return F_.Prepared(w["fc"], X2, w["lens"], w["idx"], w["img"], Nn, P, None, None, 1.0), P, Nn


def _lengths(seq):
    return np.where((seq == 0).any(1), (seq == 0).argmax(1) + 1, seq.shape[1])


def _check_winners(m, images, seq, seqlp, stats, rules, tol, what):
    """seqlp of every winner against the restatement applied to the forced-decode logits along that winner (plus the beam step's own UNK
    penalty); rule_stats = sequence_events of the winners."""
    rows, T = seq.shape
    sizes = [int(im["gpn_obj_ind"].size(1) * im["gpn_obj_ind"].size(2)) if m.gpn else 1 for im in images]
    assert sum(sizes) == rows
    bounds = np.concatenate([[0], np.cumsum(sizes)])
    logits = _forced_logits(m, images, [seq[a:b] for a, b in zip(bounds, bounds[1:])])
    lens, worst, fired = _lengths(seq), 0.0, 0
    for r in range(rows):
        L = int(lens[r])
        for t in range(L):
            lp, ev = apply_rules_restatement(logits[t, r].astype(np.float64), seq[r], t, rules, return_events=True)
            want = lp[seq[r, t]] - (1000.0 if seq[r, t] == logits.shape[2] - 1 else 0.0)
            assert np.isfinite(want), (what, r, t)
            worst = max(worst, abs(float(seqlp[r, t]) - want))
            fired += int(ev[0, 0]) + int(ev[0, 2])
        assert not seqlp[r, L:].any()
        np.testing.assert_array_equal(stats[r], sequence_events(seq[r], L, rules), err_msg=f"{what} row {r}")
    print(f"{what}: {rows} winners, worst log-prob error {worst:.3e} (bound {tol}), {fired} rule events along the winners")
    assert worst <= tol
    return fired


@pytest.mark.parametrize("case", list(CASES))
def test_golden_models_host_equals_device_eager_equals_replay_and_the_restatement(golden, case):
    name, beam_size, G = CASES[case]
    m, opt, images = _model(golden, name)
    T, V1 = m.seq_length, opt["vocab_size"] + 1
    eo = _rules_opt(V1, beam_size, G)
    rules = DecodeRules.from_beam_options(eo)
    # the eager batched search, bookkeeping on the device and on the host
    pr, P, Nn = _prepared(m, images)
    hold = {"skip_att": True}
    batch = m.sample_images(images, opt=eo, batch_out=hold)
    assert all("rule_stats" in b for per in m.done_beams for beams in per for b in beams)
    seq, seqlp, stats = hold["seq"].cpu().numpy(), hold["seqlp"].numpy(), hold["rule_stats"].numpy()
    assert stats.shape == (seq.shape[0], 4) and stats.dtype == np.int32 and torch.equal(m.rule_stats, hold["rule_stats"])
    with torch.no_grad():
        dev = beam.beam_decode(pr, P, Nn, T, eo, xt_table=m.xt_gates_table(), on_device=True, rules=rules)
        host = beam.beam_decode(pr, P, Nn, T, eo, xt_table=m.xt_gates_table(), on_device=False, rules=rules)
    assert torch.equal(dev[0], host[0]) and torch.equal(dev[1].view(torch.int32), host[1].view(torch.int32))
    _same_beams(dev[2], host[2])
    np.testing.assert_array_equal(dev[0].numpy(), seq)                          # the batch `sample_images` decoded
    fired = _check_winners(m, images, seq, seqlp, stats, rules, 1e-4, case)
    assert fired > 0
    # the rules did something: the plain search differs and carries no counters
    plain = {"skip_att": True}
    m.sample_images(images, opt={k: v for k, v in eo.items() if k != "beam_rules"}, batch_out=plain)
    assert "rule_stats" not in plain and m.rule_stats is None and "rule_stats" not in m.done_beams[0][0]
    if m.gpn:                                                                   # (Full-GC decodes two rows here: the bans hit no word they chose)
        assert not torch.equal(plain["seq"], hold["seq"])
    # one image per call: capture, replay, eager -- bit for bit; the batch gives the same tokens
    for i, im in enumerate(images):
        args = synthetic.sample_args(im)
        g1 = m._sample(*args, opt=eo)
        s1, d1 = m.rule_stats.clone(), m.done_beams
        g2 = m._sample(*args, opt=eo)
        assert any(k[0] == "beam" and ("beam_rules", rules.key) in k[3] for k in m._graph_cache)
        assert torch.equal(g1[0], g2[0]) and torch.equal(g1[1].view(torch.int32), g2[1].view(torch.int32)) and torch.equal(s1, m.rule_stats)
        m.decode_hipgraph = False
        e = m._sample(*args, opt=eo)
        m.decode_hipgraph = True
        assert torch.equal(e[0], g1[0]) and torch.equal(e[1].view(torch.int32), g1[1].view(torch.int32)) and torch.equal(m.rule_stats, s1)
        _same_beams(m.done_beams, d1)
        assert torch.equal(g1[0], batch[i][0]) and float((g1[1] - batch[i][1]).abs().max()) <= 1e-4


@pytest.mark.parametrize("case", list(CASES))
def test_golden_models_attention_of_the_winners_under_rules(golden, case):
    name, beam_size, G = CASES[case]
    m, opt, images = _model(golden, name)
    eo = _rules_opt(opt["vocab_size"] + 1, beam_size, G)
    im = images[0]
    args = synthetic.sample_args(im)
    off = m._sample(*args, opt=eo)
    d_off = m.done_beams
    on = m._sample(*args, opt=dict(eo, return_att=1))
    assert len(on) == 5 and torch.equal(on[0], off[0]) and torch.equal(on[1].view(torch.int32), off[1].view(torch.int32))
    _same_beams(m.done_beams, d_off)                                            # the ancestry step does not change the ruled search
    seq = on[0].cpu().numpy()
    lens = _lengths(seq)
    f = forced.forced_decode(m, [im], [seq], return_att=True)
    fa = f["AL"].cpu().numpy().transpose(1, 0, 2)                               # [rows, Tf, N]
    att = on[4].cpu().numpy()
    steps, n_max = att.shape[1], att.shape[2]
    assert steps == int(lens.max())
    live = np.arange(steps)[None, :] < lens[:, None]
    err = np.abs(fa[:, :steps, :n_max] - att)[live]
    print(case, "beam attention under rules against forced decode", float(err.max()))
    assert float(err.max()) <= 1e-5 and not att[~live].any()


def test_bf16_batched_search_above_32_rows_under_rules(golden):
    m, opt, _ = _model(golden, "subgc", compute_dtype="bf16", decode_b16_batched=1)
    images = [{k: v.to(DEV) for k, v in synthetic.make_test_batch(10, D=opt["att_feat_size"], seed=940 + i, fc_size=opt["att_feat_size"],
                                                                   node_pool=None).items()} for i in range(2)]
    eo = _rules_opt(opt["vocab_size"] + 1, 2, 1)
    rules = DecodeRules.from_beam_options(eo)
    hold = {"skip_att": True}
    m.sample_images(images, opt=eo, batch_out=hold)
    seq = hold["seq"].cpu().numpy()
    assert seq.shape[0] * 2 > 32
    _check_winners(m, images, seq, hold["seqlp"].numpy(), hold["rule_stats"].numpy(), rules, 5e-2, "subgc bf16-batched beam 2")


class _Watch(TorchDispatchMode):
    """tests/test_no_aten_gpu.py's method: every ATen op that launches a device kernel is recorded."""

    def __init__(self):
        super().__init__()
        from test_no_aten_gpu import HARMLESS
        self.seen, self.harmless = {}, HARMLESS

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        r = func(*args, **(kwargs or {}))
        name = str(func)
        if not any(h in name for h in self.harmless):
            ts = [t for t in (list(args) + ([r] if torch.is_tensor(r) else [])) if torch.is_tensor(t)]
            if any(t.is_cuda for t in ts) and not (("copy_" in name or "_to_copy" in name) and any(not t.is_cuda for t in ts)):
                self.seen[name] = self.seen.get(name, 0) + 1
        return r


def test_without_the_key_nothing_changes_and_the_ruled_loop_issues_no_aten_kernel(golden, monkeypatch):
    """beam_rules absent (or empty): no rules launch, the top-k folds the log-softmax in as before, and the outputs are the committed
    beam goldens' (test_parity_gpu.py's comparison).  beam_rules on, one group: the loop's launches are C-ABI launches only."""
    from test_beam_oracle import check_beams
    from test_parity_gpu import build
    calls, modes = [], []
    real_rules, real_topk = ops.decode_rules, ops.row_topk
    monkeypatch.setattr(ops, "decode_rules", lambda *a, **k: (calls.append(1), real_rules(*a, **k))[1])
    monkeypatch.setattr(ops, "row_topk", lambda x, k, v, i, log_softmax=True: (modes.append(bool(log_softmax)), real_topk(x, k, v, i, log_softmax))[1])
    for name in ("subgc_beam3", "subgc_beam4_div"):
        g = golden(name)
        m = build(g, golden("subgc_beam").group("weights"), False)
        b = {k: v.to(DEV) for k, v in g.tensors("inputs").items()}
        ret = m(*synthetic.sample_args(b), opt=dict(g.meta["sample_opt"]), mode="sample")
        check_beams(ret, m.done_beams, g.group("out"), atol=1e-4)
        assert m.rule_stats is None
        empty = m(*synthetic.sample_args(b), opt=dict(g.meta["sample_opt"], beam_rules={}), mode="sample")
        assert torch.equal(empty[0], ret[0]) and torch.equal(empty[1].view(torch.int32), ret[1].view(torch.int32))
        assert len([k for k in m._graph_cache if k[0] == "beam"]) == 1           # an inactive key is no other graph
    assert not calls and modes and all(modes)
    # the ruled search of one group, eagerly on a prepared engine: only C-ABI launches between the first and the last step
    m, opt, images = _model(golden, "subgc")
    eo = _rules_opt(opt["vocab_size"] + 1, 2, 1)
    rules = DecodeRules.from_beam_options(eo)
    pr, P, Nn = prepared(m, images[:1])
    with torch.no_grad():
        eng = beam._BatchEngine(pr, P, Nn, 2, m.xt_gates_table())
        ds = beam.DeviceSearch(eng, m.seq_length, eo, rules=rules)
        ds.loop(fresh_tables=True)
        want = ds.collect()
        eng.st.reset()
        torch.cuda.synchronize()
        del modes[:]
        with _Watch() as w:
            ds.loop()
        torch.cuda.synchronize()
        assert not w.seen, w.seen
        got = ds.collect()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))
    assert len(calls) == 2 * m.seq_length and modes and not any(modes)           # one rules launch per decoder step, top-k on the ruled rows


# ------------------------------------------------------------------------------------------------ 4. the glue
def _glue_case(images):
    infos = [{"id": 100 + i} for i in range(len(images))]
    kw = dict(sample_max=1, beam_size=2, beam_rules=dict(block_trigrams=1, block_bad_endings=1))
    return infos, kw


def _glue_vocab(V1):
    ix = {str(i): f"w{i}" for i in range(V1)}
    ix.update({"1": "with", "2": "the", "3": "a", str(V1 - 2): "of"})
    return ix


def test_caption_images_carries_the_winners_counters_whatever_the_batching(golden):
    m, opt, images = _model(golden, "subgc")
    V1 = opt["vocab_size"] + 1
    ix = _glue_vocab(V1)
    infos, kw = _glue_case(images)                                               # (no ids in kw: they come from the vocabulary)
    whole = eval_glue.caption_images(m, images, infos, ix, kw)
    one = eval_glue.caption_images(m, images, infos, ix, kw, group=1)            # one image per batch: the captured search
    hold = {"skip_att": True}
    m.sample_images(images, opt=dict(kw, beam_rules=dict(kw["beam_rules"], bad_ending_ids=[1, 2, 3, V1 - 2])), batch_out=hold)
    stats, bounds = hold["rule_stats"].numpy(), hold["bounds"]
    assert stats[:, [0, 2]].sum() > 0
    for e, e1, a, b in zip(whole, one, bounds, bounds[1:]):
        assert e["rule_stats"].shape == (b - a, 4) and e["rule_stats"].dtype == np.int32
        assert sorted(map(tuple, e["rule_stats"].tolist())) == sorted(map(tuple, stats[a:b].tolist()))
        assert (e["rule_stats"][:, 1] == 0).all() and (e["rule_stats"][:, 3] == -1).all()
        assert e1["caption"] == e["caption"]
        np.testing.assert_array_equal(e1["rule_stats"], e["rule_stats"])
        assert not any(cap.split()[-1] in ("with", "the", "a", "of") for cap in e["caption"] if cap and len(cap.split()) < m.seq_length)
    plain = eval_glue.caption_images(m, images, infos, ix, dict(sample_max=1, beam_size=2))
    assert all("rule_stats" not in e for e in plain)


def _shard_worker(rank, world, port, q):
    import os
    import test_parallel_decode as PD
    PD._paths()
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    from conftest import Golden
    from subgc import parallel
    torch.cuda.set_device(0)
    parallel.init_distributed("gloo")
    m, opt, images = _model(Golden, "subgc")
    infos, kw = _glue_case(images)
    preds = eval_glue.caption_images(m, images, infos, _glue_vocab(opt["vocab_size"] + 1), kw, group=2, shard=True)
    q.put((rank, [(p["image_id"], p["caption"], np.asarray(p["rule_stats"])) for p in preds]))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_sharded_decode_gathers_the_winners_counters(golden):
    """Two gloo ranks on the one device caption their shares (images 0 and 2, image 1) under beam_rules; after the gather and the
    reorder every rank holds every image's entry, its `rule_stats` equal to the one-process run's."""
    import torch.multiprocessing as mp
    import test_parallel_decode as PD
    world, port = 2, PD._free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_shard_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = PD._collect(q, procs, 500)
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    m, opt, images = _model(golden, "subgc")
    infos, kw = _glue_case(images)
    want = eval_glue.caption_images(m, images, infos, _glue_vocab(opt["vocab_size"] + 1), kw)
    assert len(res) == world and len(images) > world
    assert sum(int(p["rule_stats"][:, [0, 2]].sum()) for p in want) > 0         # the rules fired along some winner
    for _, got in res:
        assert [i for i, _, _ in got] == [p["image_id"] for p in want]
        for (_, cap, stats), p in zip(got, want):
            assert cap == p["caption"]
            assert stats.dtype == np.int32 and stats.shape == p["rule_stats"].shape
            np.testing.assert_array_equal(stats, p["rule_stats"])


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals(golden):
    opt = _fake_opt(4, 2, 2.0)
    rules = DecodeRules.from_beam_options(opt)
    with pytest.raises(ValueError, match="T \\+ group_size - 1 = 65 columns; the limit is 64"):
        beam.DeviceSearch(FK.DeviceEngine(1, 4, (3,), N, 0, DEV), 64, opt, rules=rules)
    beam.DeviceSearch(FK.DeviceEngine(1, 4, (3,), N, 0, DEV), 63, opt, rules=rules)
    m, mopt, images = _model(golden, "subgc")
    args = synthetic.sample_args(images[0])
    for size in (1, None):
        o = {"sample_max": 1, "beam_rules": {"block_trigrams": 1}}
        if size is not None:
            o["beam_size"] = size
        with pytest.raises(ValueError, match="^beam_rules with beam_size = 1: .*top-level keys block_trigrams"):
            m._sample(*args, opt=o)
        with pytest.raises(ValueError, match="^beam_rules with beam_size = 1"):
            m.sample_images(images, opt=o)
    with pytest.raises(ValueError, match="beam_rules\\['suppress_unk'\\]"):
        m._sample(*args, opt={"beam_size": 2, "beam_rules": {"suppress_unk": 1}})
    # the reference's step API: the caller's log-probabilities cannot be ruled
    V1, R_ = mopt["vocab_size"] + 1, m.rnn_size
    state = (torch.zeros(2, 2, R_, device=DEV), torch.zeros(2, 2, R_, device=DEV))
    with pytest.raises(ValueError, match="beam_rules: the step-API engine"):
        m.beam_search(state, torch.zeros(2, V1, device=DEV), None, None, None, None, opt={"beam_size": 2, "beam_rules": {"block_trigrams": 1}})
