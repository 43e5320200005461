"""Forced decode and GT-sentence grounding on the device (include/subgc_forced_hip.h): the pick and finish kernels against their stated
rules and an fp64 log-softmax within the bound DESIGN 4.P derives, the forced decode against the fixture the reference model wrote
(tests/golden/make_golden_forced.py), forcing a greedy decode's own tokens, the score kernel against the fixture the reference's own
`gt_grd_eval` wrote (make_golden_grounding_gt.py) byte for byte, `eval_glue.ground_gt_images` end to end, and no ATen device kernel."""
import argparse
import math
import os

import numpy as np
import pytest
import torch

import grounding_gt_golden as GG
import grounding_golden as G
from subgc import eval_glue, forced, grounding, ops, synthetic
from subgc import grounding_gt as GT
from subgc._lib import SubgcError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24


def lp_bound(V, d, log_s, lp):
    """|lp - exact| <= u (|d| + |lp| + 2 |log S| + ln V + CH + 10), first order, with 0.1 % for the higher orders."""
    ch = (V + 255) // 256
    return 1.001 * U * (abs(d) + abs(lp) + 2 * abs(log_s) + math.log(V) + ch + 10)


def _pick_state(n, T, V, seed, ld_extra=3):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(n, V + ld_extra, generator=g) * 4).to(DEV)[:, :V]
    return x


def _run_pick(x, tok, t, unf0, raw, prev=None, T=None):
    n, V = x.shape
    T = tok.size(1) if T is None else T
    seq = torch.full((n, T), -7, device=DEV, dtype=torch.int64)
    seqlp = torch.full((n, T), -7.0, device=DEV)
    it = torch.full((n,), -7, device=DEV, dtype=torch.int64)
    unf = torch.tensor(unf0, device=DEV, dtype=torch.int32)
    flag = torch.zeros(1, device=DEV, dtype=torch.int32)
    pc = None if prev is None else torch.tensor([prev], device=DEV, dtype=torch.int32)
    forced.forced_pick(x, tok, t, seq, seqlp, it, unf, flag, pc, raw=raw)
    torch.cuda.synchronize()
    return seq.cpu(), seqlp.cpu(), it.cpu(), unf.cpu(), int(flag.item())


@pytest.mark.parametrize("V", [51, 256, 257, 1000, 9488])
def test_forced_pick_one_step(V):
    x = _pick_state(3, 4, V, 100 + V)
    # row 0: a word; row 1: finished before the step; row 2: the end token on a live row
    tok = torch.tensor([[1, V - 1, 5, 5], [2, 3, 4, 4], [3, 0, 9, 9]], device=DEV)
    seq, seqlp, it, unf, flag = _run_pick(x, tok, 1, [1, 0, 1], True)
    assert seq[:, 1].tolist() == [V - 1, 0, 0] == it.tolist() and unf.tolist() == [1, 0, 0] and flag == 1
    assert (seq[:, [0, 2, 3]] == -7).all() and (seqlp[:, [0, 2, 3]] == -7).all()          # one column per step
    ref = torch.log_softmax(x.double().cpu(), 1)
    xd = x.double().cpu()
    worst = 0.0
    for r, c in ((0, V - 1), (2, 0)):
        d = float(xd[r, c] - xd[r].max())
        log_s = float(torch.logsumexp(xd[r] - xd[r].max(), 0))
        err, b = abs(float(seqlp[r, 1]) - float(ref[r, c])), lp_bound(V, d, log_s, float(ref[r, c]))
        worst = max(worst, err / b)
        assert err <= b, (V, r, err, b)
    print(f"V = {V}: worst |lp - fp64 log-softmax| / bound = {worst:.3f}")
    assert float(seqlp[1, 1]) == 0.0                                                       # a finished row files 0, not a log-prob
    # t == 0: every row is live whatever `unfinished` holds; row 2's first token is a word
    seq0, lp0, it0, unf0, flag0 = _run_pick(x, tok, 0, [0, 0, 0], True)
    assert seq0[:, 0].tolist() == [1, 2, 3] and unf0.tolist() == [1, 1, 1] and flag0 == 1 and (lp0[:, 0] < 0).all()
    # log-probabilities in, raw_logits = 0: x[tok] exactly
    lpx = torch.log_softmax(x, 1)
    _, lp1, _, _, _ = _run_pick(lpx, tok, 1, [1, 0, 1], False)
    assert lp1[0, 1] == lpx[0, V - 1].cpu() and lp1[2, 1] == lpx[2, 0].cpu() and float(lp1[1, 1]) == 0.0
    # prev_count == 0: nothing is written; prev_count != 0: the same as without it
    seq2, lp2, it2, unf2, flag2 = _run_pick(x, tok, 1, [1, 0, 1], True, prev=0)
    assert (seq2 == -7).all() and (lp2 == -7).all() and (it2 == -7).all() and unf2.tolist() == [1, 0, 1] and flag2 == 0
    seq3, lp3, it3, unf3, flag3 = _run_pick(x, tok, 1, [1, 0, 1], True, prev=1)
    # equal inputs give equal bits
    assert torch.equal(seq3, seq) and torch.equal(lp3.view(torch.int32), seqlp.view(torch.int32)) and unf3.tolist() == unf.tolist() and flag3 == 1
    # the last step with no row left unfinished leaves the flag alone
    _, _, _, unf4, flag4 = _run_pick(x, tok, 1, [0, 0, 1], True)
    assert unf4.tolist() == [0, 0, 0] and flag4 == 0


def test_forced_pick_clamps_and_debug_bounds_reports():
    V = 257
    x = _pick_state(2, 2, V, 7)
    tok = torch.tensor([[V + 5, 1], [-3, 1]], device=DEV)
    seq, seqlp, it, unf, _ = _run_pick(x, tok, 0, [0, 0], True)
    ref = torch.log_softmax(x.double().cpu(), 1)
    assert seq[:, 0].tolist() == [V - 1, 0] and unf.tolist() == [1, 0]
    assert abs(float(seqlp[0, 0]) - float(ref[0, V - 1])) < 1e-5 and abs(float(seqlp[1, 0]) - float(ref[1, 0])) < 1e-5
    with ops.debug_bounds():
        with pytest.raises(SubgcError, match="forced_pick: forced"):
            _run_pick(x, tok, 0, [0, 0], True)
        _run_pick(x, tok, 1, [1, 1], True)                                                 # column 1 is in range


def test_forced_pick_three_steps_and_finish_are_the_stated_rule():
    V, n, Tf, T = 1000, 3, 3, 5
    x = [_pick_state(n, T, V, 200 + t) for t in range(Tf)]
    tok = torch.tensor([[4, 0, 6], [7, 8, 9], [0, 3, 3]], device=DEV)
    seq = torch.zeros(n, T, device=DEV, dtype=torch.int64)
    seqlp = torch.zeros(n, T, device=DEV)
    it, unf = torch.zeros(n, device=DEV, dtype=torch.int64), torch.zeros(n, device=DEV, dtype=torch.int32)
    counts = torch.zeros(Tf, device=DEV, dtype=torch.int32)
    for t in range(Tf):
        forced.forced_pick(x[t], tok, t, seq, seqlp, it, unf, counts[t:t + 1], counts[t - 1:t] if t else None, raw=True)
    ll, n_tok = forced.forced_finish(seq, seqlp, Tf)
    torch.cuda.synchronize()
    assert seq.cpu().tolist() == [[4, 0, 0, 0, 0], [7, 8, 9, 0, 0], [0, 0, 0, 0, 0]]
    assert counts.cpu().tolist() == [1, 1, 1] and unf.cpu().tolist() == [0, 1, 0] and it.cpu().tolist() == [0, 9, 0]
    lp = seqlp.cpu()
    live = torch.tensor([[1, 1, 0, 0, 0], [1, 1, 1, 0, 0], [1, 0, 0, 0, 0]], dtype=torch.bool)
    assert (lp[~live] == 0).all() and (lp[live] < 0).all()
    ref = [torch.log_softmax(x[t].double().cpu(), 1) for t in range(Tf)]
    assert abs(float(lp[0, 1]) - float(ref[1][0, 0])) < 1e-5 and abs(float(lp[1, 2]) - float(ref[2][1, 9])) < 1e-5
    # finish: the ascending-t fp64 sum, exact
    assert n_tok.cpu().tolist() == [2, 3, 1]
    for r in range(n):
        want = 0.0
        for t in range(int(live[r].sum())):
            want += float(lp[r, t])
        assert float(ll[r]) == want
    # a batch whose rows all ended: the next step writes nothing
    seq2, lp2 = torch.zeros_like(seq), torch.zeros_like(seqlp)
    done = torch.zeros(1, device=DEV, dtype=torch.int32)
    forced.forced_pick(x[1], tok, 1, seq2, lp2, it, unf, counts[1:2], done, raw=True)
    torch.cuda.synchronize()
    assert not seq2.any() and not lp2.any()


# ---------------------------------------------------------------------------------------------- the model
def _model(golden, fmeta, name, **over):
    import subgc.models as models
    opt = dict(fmeta["cases"][name]["opt"])
    opt.setdefault("obj_name_path", None); opt.setdefault("rel_name_path", None)
    opt.update(caption_model="topdown", **over)
    w = golden("subgc_beam" if name == "subgc" else "fullgc_train").group("weights")
    m = models.setup(argparse.Namespace(**opt))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    return m.to(DEV).eval(), opt


def _images(fmeta, name, opt):
    return [{k: v.to(DEV) for k, v in synthetic.make_test_batch(i["M"], D=opt["att_feat_size"], seed=i["seed"], fc_size=opt["att_feat_size"],
                                                                node_pool=i["pool"]).items()} for i in fmeta["cases"][name]["images"]]


def _nodes(AL, idx, words):
    """host: the node every word position attended to most (first arg-max), -1 elsewhere."""
    a = AL.cpu().numpy().transpose(1, 0, 2)                                  # [rows, Tf, N]
    return np.where(words, np.take_along_axis(idx.cpu().numpy(), a.argmax(2), 1), -1)


@pytest.fixture(scope="module")
def fcase():
    return GG.load_forced()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["subgc", "fullgc"])
def test_forced_decode_equals_the_reference_model(golden, fcase, name, dtype):
    fmeta, arr = fcase
    m, opt = _model(golden, fmeta, name, **({"compute_dtype": "bf16"} if dtype == "bf16" else {}))
    tok, b = arr[name + "_tokens"], arr[name + "_bounds"]
    assert tok.shape[1] == fmeta["Tf"] != m.seq_length                       # Tf comes from the token rows, not from the model
    d = forced.forced_decode(m, _images(fmeta, name, opt), [tok[b[i]:b[i + 1]] for i in range(len(b) - 1)], return_att=True)
    torch.cuda.synchronize()
    live = np.concatenate([np.ones((len(tok), 1), bool), np.cumprod(tok[:, :-1] > 0, 1).astype(bool)], 1)
    words = np.cumprod(tok > 0, 1).astype(bool)
    seqlp = d["seqlp"].cpu().numpy()
    np.testing.assert_array_equal(d["seq"].cpu().numpy(), np.where(live, tok, 0))
    assert (seqlp[~live] == 0).all() and d["bounds"] == b.tolist()
    err = float(np.abs(seqlp - arr[name + "_lp"])[live].max())
    print(f"{name} {dtype}: max |seqlp - reference| = {err:.3e} over {int(live.sum())} live steps")
    if dtype == "bf16":
        assert err <= 5e-2                                                   # bf16 against fp32, atol 5e-2
        return
    assert err <= 1e-4
    np.testing.assert_array_equal(d["idx"].cpu().numpy(), arr[name + "_idx"])
    np.testing.assert_array_equal(_nodes(d["AL"], d["idx"], words), arr[name + "_node"])
    assert float(np.abs(d["AL"].cpu().numpy().transpose(1, 0, 2) - arr[name + "_att"])[live].max()) <= 1e-5
    ll, n_tok = d["ll"].cpu().numpy(), d["n_tok"].cpu().numpy()
    np.testing.assert_array_equal(n_tok, live.sum(1))
    assert abs(-ll.sum() / n_tok.sum() - float(arr[name + "_masked_mean"][0])) <= 1e-4
    s = forced.score_captions(m, _images(fmeta, name, opt), [tok[b[i]:b[i + 1]] for i in range(len(b) - 1)])
    np.testing.assert_array_equal(s["ll"], ll)
    assert s["mean_nll"] == float(-ll.sum() / n_tok.sum()) and np.allclose(s["perplexity"], np.exp(-ll / n_tok), rtol=1e-15)


@pytest.mark.parametrize("name", ["subgc", "fullgc"])
def test_forcing_a_greedy_decode_s_own_tokens_returns_them(golden, fcase, name):
    fmeta, _ = fcase
    m, opt = _model(golden, fmeta, name, gpn_nms_thres=1.0, gpn_max_subg=64)   # the NMS keeps every candidate, in input order
    images = _images(fmeta, name, opt)
    hold = {"skip_att": True}
    m.sample_images(images, opt=dict(sample_max=1, beam_size=1, return_att=1), batch_out=hold)
    seq, bounds = hold["seq"].cpu().numpy(), hold["bounds"]
    if name == "subgc":
        assert [b - a for a, b in zip(bounds, bounds[1:])] == [2 * i["M"] for i in fmeta["cases"][name]["images"]]
        keep = hold["keep"].cpu().numpy()
        assert all(keep[a:b].tolist() == list(range(b - a)) for a, b in zip(bounds, bounds[1:]))
    d = forced.forced_decode(m, images, [seq[a:b] for a, b in zip(bounds, bounds[1:])], return_att=True)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(d["seq"].cpu().numpy(), seq)
    words = np.cumprod(seq > 0, 1).astype(bool)
    assert words.sum() > 20
    T = seq.shape[1]
    np.testing.assert_array_equal(_nodes(d["AL"], d["idx"], words), _nodes(hold["AL"][:T], hold["idx"], words))
    glp = hold["seqlp"].cpu().numpy()
    live = np.concatenate([np.ones((len(seq), 1), bool), words[:, :-1]], 1)
    assert float(np.abs(d["seqlp"].cpu().numpy() - glp)[live].max()) <= 1e-4


# ---------------------------------------------------------------------------------------------- the score kernel
@pytest.fixture(scope="module")
def case():
    return GG.load()


@pytest.mark.parametrize("tag", ["rnd", "edge", "model"])
def test_score_kernel_equals_the_restatement_and_the_reference(case, tag):
    meta, arr = case
    refs = GG.references(meta, arr, tag, device=DEV)
    sc = GT.GtGroundingScorer(refs)
    res = GG.results(arr, tag)
    got = sc.score_submission(res)
    GG.same_events(got, GG.restate_submission(refs, res))                    # device bytes = the restatement's
    GG.same_events(got, GG.expected_entries(meta, arr, tag, refs))           # = the reference's
    s = GT.summarize(got, refs)
    ref_accu = float(arr[tag + "_accu"][0])
    print(tag, "grd_accu", s["grd_accu"], "reference", ref_accu)
    GG.accu_close(s["grd_accu"], ref_accu, s["n_classes"])
    # the lists ride along unchanged
    for e in got:
        img = refs.image_ids[e["ref"]]
        if e["rows"] is None:
            assert img not in res
            continue
        for r_, w in zip(e["rows"], res[img]):
            assert r_["idx_in_sent"].tolist() == w["idx_in_sent"]
            np.testing.assert_array_equal(r_["bbox"], np.asarray(w["bbox"], np.float64).reshape(-1, 4).astype(np.float32))
    # two batches, in another order, summarise to the same value
    items = [(e["ref"], None if e["rows"] is None else res[refs.image_ids[e["ref"]]][:len(e["rows"])]) for e in got]
    half = len(items) // 2
    two = sc.score_lists(items[half:]) + sc.score_lists(items[:half])
    GG.accu_close(GT.summarize(two, refs)["grd_accu"], ref_accu, s["n_classes"])
    assert GT.summarize(two, refs)["grd_accu"] == s["grd_accu"]


def test_the_same_box_pairs_hit_and_miss_in_both_score_kernels(case):
    meta, arr = case
    pairs = []
    for tag in ("edge", "rnd"):
        anns, split = GG.annotations(meta, arr, tag)
        res = GG.results(arr, tag)
        for a in anns:
            for s, c in enumerate(a["captions"]):
                lists = res.get(str(a["image_id"]))
                if lists is None or s >= len(lists):
                    continue
                for q, idx in enumerate(c["process_idx"]):
                    if idx in lists[s]["idx_in_sent"]:
                        pairs.append((lists[s]["bbox"][lists[s]["idx_in_sent"].index(idx)], c["process_bnd_box"][q]))
    assert len(pairs) > 100
    anns = [{"image_id": k, "captions": [{"tokens": ["c1"], "process_clss": ["c1"], "process_idx": [0], "process_bnd_box": [g]}]}
            for k, (_, g) in enumerate(pairs)]
    refs = grounding.GroundingReferences(anns, list(range(len(pairs))), meta["det_id_to_det_wd"], G.WD_TO_LEMMA, G.LEMMA_DET, G.VOCAB, meta["lemma"],
                                         device=DEV)
    old = grounding.GroundingScorer(refs).score_entries([(k, {"clss": ["c1"], "idx_in_sent": [0], "bbox": [p]}) for k, (p, _) in enumerate(pairs)])
    new = GT.GtGroundingScorer(refs).score_lists([(k, [{"idx_in_sent": [0], "bbox": [p]}]) for k, (p, _) in enumerate(pairs)])
    a = [int(e["recall"][0, 1]) for e in old]
    b = [int(e["events"][0, 1]) for e in new]
    assert a == b and set(a) == {GT.HIT, GT.MISS}
    assert a == [int(GT.HIT if GT.iou_f32(p, g) > np.float32(0.5) else GT.MISS) for p, g in pairs]


def test_debug_bounds_reports_a_pair_row_past_the_rows(case):
    meta, arr = case
    refs = GG.references(meta, arr, "edge", device=DEV)
    sc = GT.GtGroundingScorer(refs)
    j = refs.index["8002"]
    plan = sc.plan([j], [5])
    table = plan["table"].copy()
    table[plan["P"] + 2] = 5                                                 # pair 2 names row 5 of 5
    arena = torch.zeros(sc.arena_words(plan), device=DEV, dtype=torch.int32)
    with ops.debug_bounds():
        with pytest.raises(SubgcError, match="pair_row"):
            sc.enqueue_score(torch.from_numpy(table).to(DEV), arena, plan)
    sc.enqueue_score(torch.from_numpy(table).to(DEV), arena, plan)           # clamped without it: nothing is read out of range
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- end to end
def _gt_args(case, fcase, refs):
    meta, arr = case
    fmeta, f = fcase
    b, bo = f["subgc_bounds"], f["subgc_box_off"]
    ids = [5000 + i for i in range(len(b) - 1)]
    return ids, {"scorer": GT.GtGroundingScorer(refs), "index": {k: refs.index[str(k)] for k in ids},
                 "rows": {k: f["subgc_tokens"][b[i]:b[i + 1]] for i, k in enumerate(ids)},
                 "boxes": {k: f["subgc_boxes"][bo[i]:bo[i + 1]] for i, k in enumerate(ids)}, "img_wh": None}


def test_ground_gt_images_end_to_end_on_the_model_set(golden, case, fcase):
    meta, arr = case
    fmeta, f = fcase
    m, opt = _model(golden, fmeta, "subgc")
    refs = GG.references(meta, arr, "model", device=DEV)
    ids, gt = _gt_args(case, fcase, refs)
    images, infos = _images(fmeta, "subgc", opt), [{"id": k} for k in ids]
    want = GG.expected_entries(meta, arr, "model", refs)
    ref_accu = float(arr["model_accu"][0])
    for group in (64, 2):
        out = eval_glue.ground_gt_images(m, images, infos, gt, group=group)
        assert [e["image_id"] for e in out] == ids
        GG.same_events([e["gt_grounding"] for e in out], want)
        s = GT.summarize([e["gt_grounding"] for e in out], refs)
        GG.accu_close(s["grd_accu"], ref_accu, s["n_classes"])
        res = GG.results(arr, "model")
        b = f["subgc_bounds"]
        for i, e in enumerate(out):
            for r_, w in zip(e["gt_grounding"]["rows"], res[str(e["image_id"])]):
                assert r_["idx_in_sent"].tolist() == w["idx_in_sent"]
                np.testing.assert_array_equal(r_["bbox"], np.asarray(w["bbox"], np.float64).reshape(-1, 4).astype(np.float32))
            lp = f["subgc_lp"][b[i]:b[i + 1]].astype(np.float64)
            assert np.abs(e["caption_ll"]["ll"] - lp.sum(1)).max() <= 1e-4 * lp.shape[1]
            np.testing.assert_array_equal(e["caption_ll"]["n_tok"], (lp != 0).sum(1))
        # the reference evaluator's file form round-trips through the list launch
        sub = GT.to_submission([e["gt_grounding"] for e in out])
        GG.same_events(gt["scorer"].score_submission(sub["results"]), want)
    with pytest.raises(SubgcError, match="brings 4 rows and has 5 reference captions"):
        eval_glue.ground_gt_images(m, images[:1], infos[:1], dict(gt, rows={ids[0]: gt["rows"][ids[0]][:4]}))


@pytest.mark.skipif(os.getenv("SUBGC_POISON_EMPTY") == "1", reason="the poisoned run fills every torch.empty buffer with an ATen fill_ by design")
def test_forced_decode_and_gt_grounding_issue_no_aten_device_kernel(golden, case, fcase):
    from test_no_aten_gpu import Watch
    meta, arr = case
    fmeta, f = fcase
    refs = GG.references(meta, arr, "model", device=DEV)
    ids, gt = _gt_args(case, fcase, refs)
    for name in ("subgc", "fullgc"):
        m, opt = _model(golden, fmeta, name)
        images = _images(fmeta, name, opt)
        tok, b = f[name + "_tokens"], f[name + "_bounds"]
        tokens = [tok[b[i]:b[i + 1]] for i in range(len(b) - 1)]
        run = (lambda: eval_glue.ground_gt_images(m, images, [{"id": k} for k in ids], gt)) if name == "subgc" else \
              (lambda: forced.forced_decode(m, images, tokens, return_att=True))
        run()
        run()
        torch.cuda.synchronize()
        with Watch() as w:
            run()
        torch.cuda.synchronize()
        assert not w.seen, (name, dict(w.seen))
