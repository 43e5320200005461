"""`eval_collect` with all four scorer passes on at once (consensus, diversity, accuracy, grounding) against its own single-option runs:
the interplay no other test exercises -- the one upload and the one arena shared by every pass, the re-ranker's first choice feeding the
accuracy top-1 and the grounding pick on the device, an image without rows in the middle of the batch, a batch without any row.

Equality is byte for byte over everything a pass defines: the base keys and the plan table as arrays, the scorers' results through their
own `unpack` (an arena's slack -- list slots behind an image's count, sums and orders behind `top_k` -- is `torch.empty` memory and
differs with the arena's place in memory, not with the code).  One comparison is not bitwise: `caption_images(group=1)` against the one
decode batch holds the entries' `subgraph_score` to 2^-18 relative, because the sGPN score is the model's own sum and runs in another
order in a decode batch of another shape (measured: one value 1 ulp apart); every other key of those entries is compared exactly."""
import os

import numpy as np
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

import accuracy_golden as AG
import grounding_golden as GG
from subgc import accuracy, consensus, diversity, eval_glue, grounding, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES, T, T1, N = [2, 0, 3, 1], 6, 7, 5
BOUNDS = [0, 2, 2, 5, 6]
IDS = [70, 71, 72, 73]
PICK = [1, 0, 2, 0]
# host -> device copies of one call with all four passes on, measured on the parent commit with `_Traffic` below for the same arguments:
# the batch's int32 upload, the re-ranker's neighbour table, the diversity plan's table, the grounding boxes
PARENT_H2D = 4


def _same(a, b, where=""):
    """Equal types, shapes and bits, through dicts and lists."""
    if isinstance(a, dict):
        assert isinstance(b, dict) and sorted(a) == sorted(b), where
        for k in a:
            _same(a[k], b[k], f"{where}.{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for j, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{where}[{j}]")
    else:
        x, y = np.asarray(a), np.asarray(b)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), where


@pytest.fixture(scope="module")
def batch():
    """The decode batch and the four options' arguments, built once and never written to."""
    rng = np.random.default_rng(20)
    vocab = GG.VOCAB
    word = lambda x: vocab[str(int(x))]
    corpus_ids = [[[int(x) for x in rng.integers(1, 13, size=int(rng.integers(5, 7)))] for _ in range(2)] for _ in range(8)]
    nn = [[int(x) for x in rng.choice(8, 3, replace=False)] for _ in SIZES]
    rows = BOUNDS[-1]
    seq = np.zeros((rows, T), np.int64)
    for r, n in enumerate([0, 5, 6, 3, 1, 4]):                            # a row with no words (row 0), a row of full length (row 2)
        seq[r, :n] = rng.integers(1, 13, size=n)
    # image 0: its best-scored row has no words, its second row IS a caption of its first neighbour -> the re-ranker's first choice is 1
    # under 'cider' and under 'bleu' (five words: the 4-gram order is defined)
    seq[1, :] = 0
    seq[1, :5] = corpus_ids[nn[0][0]][0][:5]
    corpus_ids[nn[0][0]][0] = corpus_ids[nn[0][0]][0][:5]
    score = np.array([0.9, 0.2, 0.3, 0.8, 0.5, 0.6], np.float32)          # distinct, not sorted (image 2 ranks its rows 1, 2, 0)
    idx = np.stack([np.sort(rng.permutation(N)) for _ in range(rows)])
    d = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(DEV)
    corpus = consensus.ConsensusCorpus([[[word(x) for x in cap] for cap in caps] for caps in corpus_ids], vocab, device=DEV)
    a_refs = accuracy.AccuracyReferences([[[f"w{int(x)}" for x in rng.integers(1, 13, size=int(rng.integers(2, 7)))] for _ in range(2)]
                                          for _ in range(4)], AG.vocab(12), device=DEV)
    meta, arr = GG.load()
    g_refs = GG.references(meta, arr, "rnd", device=DEV)
    d_scorer = diversity.DiversityScorer(None, 2, ix_to_word=vocab)
    return {
        "base": dict(score=d(score, torch.float32), keep=d(np.arange(rows), torch.int64), seq=d(seq, torch.int64), bounds=BOUNDS,
                     AL=d(rng.random((T1, rows, N)), torch.float32), idx=d(idx, torch.int64)),
        "corpus": corpus, "nn": nn,
        "diversity": {"scorer": d_scorer, "plan": d_scorer.plan(diversity.per_image_draws(SIZES, IDS, (2, 100), 2019), SIZES)},
        "accuracy": {"scorer": accuracy.AccuracyScorer(a_refs, oracle_num=2), "index": [2, 0, 3, 1]},
        "grounding": {"scorer": grounding.GroundingScorer(g_refs), "index": [int(x) for x in rng.integers(0, g_refs.n_img, size=4)],
                      "boxes": [grounding.prepare_boxes(rng.random((N, 4)) * 300, (640, 480)) for _ in SIZES]},
    }


def _run(batch, cons=None, pick=None, **on):
    """eval_collect on the batch with the named options (`cons`: a re-ranker)."""
    kw = {k: batch[k] for k, v in on.items() if v}
    if cons is not None:
        kw["consensus"] = {"reranker": cons, "nn": batch["nn"], "top_k": 2}
    return ops.eval_collect(**batch["base"], pick=pick, **kw)


def _parts(batch, h):
    """What each pass defines in `h`, ready for `_same`."""
    out = {}
    if "c_first" in h:
        out["consensus"] = consensus.chunk_entries({"top_k": 2}, h, BOUNDS)
        out["c_first"] = [int(f) for f, n in zip(h["c_first"], SIZES) if n]
    if "d_int" in h:
        out["diversity"] = batch["diversity"]["scorer"].unpack(batch["diversity"]["plan"], h["d_int"], h["d_f64"])
    if "a_words" in h:
        out["accuracy"] = batch["accuracy"]["scorer"].unpack(h["a_words"], BOUNDS)      # an image without rows: its records are zeroed
    if "g_words" in h:
        out["grounding"] = batch["grounding"]["scorer"].unpack(h["g_words"], h["g_plan"])
        out["g_table"] = h["g_plan"]["table"]
    return out


BASE = ("order", "score", "keep", "seq", "att2", "node", "n_words")


@pytest.mark.parametrize("method", ["cider", "bleu"])
def test_all_four_passes_equal_their_single_option_runs(batch, method):
    rr = consensus.make_reranker(batch["corpus"], method, k=3, m=4)
    plain = _run(batch)
    every = _run(batch, rr, diversity=1, accuracy=1, grounding=1)
    assert sorted(plain) == sorted(BASE)
    assert sorted(every) == sorted(BASE + ("c_sim", "c_order", "c_first", "d_int", "d_f64", "a_words", "g_words", "g_plan"))
    assert every["c_sim"].dtype == np.float64 and every["d_f64"].dtype == np.float64 and every["a_words"].dtype == np.int32
    got = _parts(batch, every)
    print(method, "first choices", every["c_first"].tolist(), "order", every["order"].tolist())
    assert every["order"].tolist() == [0, 1, 1, 2, 0, 0]                  # image-local ranks: image 2 was not sorted on entry
    only_c = _run(batch, rr)
    for k in BASE:                                                        # the arg-max follows the pick, which consensus moves
        _same(every[k], (only_c if k in ("att2", "node", "n_words") else plain)[k], k)
    _same(got["consensus"], _parts(batch, only_c)["consensus"], "consensus")
    _same(got["c_first"], _parts(batch, only_c)["c_first"], "c_first")
    _same(got["diversity"], _parts(batch, _run(batch, diversity=1))["diversity"], "diversity")
    _same(got["accuracy"], _parts(batch, _run(batch, rr, accuracy=1))["accuracy"], "accuracy")
    assert [e["top1_row"] for e, n in zip(got["accuracy"], SIZES) if n] == got["c_first"]       # the top-1 comes from c_first
    with_c = _parts(batch, _run(batch, rr, grounding=1))
    _same(got["grounding"], with_c["grounding"], "grounding")
    _same(got["g_table"], with_c["g_table"], "g_table")
    assert got["c_first"][0] == 1 and any(got["c_first"])                 # the pick did come from the re-ranker: not 0 everywhere
    moved = _parts(batch, _run(batch, grounding=1))["grounding"]
    assert any(x["idx_in_sent"].tobytes() != y["idx_in_sent"].tobytes() or x["bbox"].tobytes() != y["bbox"].tobytes()
               for x, y in zip(got["grounding"], moved))                  # ... and the entry follows it
    # an explicit pick wins over the re-ranker's first choice, with and without consensus
    want = _parts(batch, _run(batch, pick=PICK, grounding=1))
    for h in (_run(batch, rr, pick=PICK, diversity=1, accuracy=1, grounding=1), _run(batch, rr, pick=PICK, grounding=1)):
        _same(_parts(batch, h)["grounding"], want["grounding"], "picked")
        _same(h["node"], _run(batch, pick=PICK)["node"], "picked node")


def test_rows_that_are_not_contiguous_give_the_same_outputs(batch):
    """`seq` as a column slice of a wider tensor: the contiguous copy the launches read must live until the arg-max, the last launch that
    reads it, is enqueued -- behind every pass's own allocations."""
    rr = consensus.make_reranker(batch["corpus"], "cider", k=3, m=4)
    seq = batch["base"]["seq"]
    wide = torch.cat([seq, seq.flip(1)], 1)[:, :T]
    assert not wide.is_contiguous() and torch.equal(wide, seq)
    want = _run(batch, rr, diversity=1, accuracy=1, grounding=1)
    got = _run(dict(batch, base=dict(batch["base"], seq=wide)), rr, diversity=1, accuracy=1, grounding=1)
    _same({k: got[k] for k in BASE}, {k: want[k] for k in BASE}, "base")
    _same(_parts(batch, got), _parts(batch, want), "passes")


class _Traffic(TorchDispatchMode):
    """Counts the copies between host and device (the method of tests/test_accuracy_gpu.py, both directions)."""

    def __init__(self):
        super().__init__()
        self.to_host = self.to_device = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        r = func(*args, **(kwargs or {}))
        name = str(func)
        if "copy_" in name or "_to_copy" in name:
            src = args[1] if "copy_" in name and "_to_copy" not in name else args[0]
            dst = args[0] if "copy_" in name and "_to_copy" not in name else r
            if torch.is_tensor(src) and torch.is_tensor(dst):
                self.to_host += int(src.is_cuda and not dst.is_cuda)
                self.to_device += int(dst.is_cuda and not src.is_cuda)
        return r


@pytest.mark.skipif(os.getenv("SUBGC_POISON_EMPTY") == "1", reason="the poisoned run fills every torch.empty buffer with an ATen fill_ by design")
def test_all_four_passes_are_one_copy_back_no_aten_kernel_and_the_parents_uploads(batch):
    from test_no_aten_gpu import Watch
    rr = consensus.make_reranker(batch["corpus"], "cider", k=3, m=4)
    _run(batch, rr, diversity=1, accuracy=1, grounding=1)
    torch.cuda.synchronize()
    with Watch() as w, _Traffic() as t:
        _run(batch, rr, diversity=1, accuracy=1, grounding=1)
    torch.cuda.synchronize()
    print("device -> host", t.to_host, "host -> device", t.to_device)
    assert not w.seen, dict(w.seen)
    assert t.to_host == 1 and t.to_device == PARENT_H2D, (t.to_host, t.to_device)


def test_a_batch_without_rows_launches_nothing_and_keeps_the_keys(batch):
    rr = consensus.make_reranker(batch["corpus"], "cider", k=3, m=4)
    full = _run(batch, rr, diversity=1, accuracy=1, grounding=1)
    z = lambda *shape, dt: torch.zeros(*shape, dtype=dt, device=DEV)
    g, a, d_scorer = batch["grounding"], batch["accuracy"], batch["diversity"]["scorer"]
    plan = d_scorer.plan(diversity.per_image_draws([0, 0], IDS[:2], (2, 100), 2019), [0, 0])
    h = ops.eval_collect(z(0, dt=torch.float32), z(0, dt=torch.int64), z(0, T, dt=torch.int64), [0, 0, 0], AL=torch.rand(T1, 1, N, device=DEV),
                         idx=z(1, N, dt=torch.int64), consensus={"reranker": rr, "nn": batch["nn"][:2], "top_k": 2},
                         diversity={"scorer": d_scorer, "plan": plan}, accuracy={"scorer": a["scorer"], "index": a["index"][:2]},
                         grounding={"scorer": g["scorer"], "index": g["index"][:2], "boxes": g["boxes"][:2]})
    torch.cuda.synchronize()                                              # a launch error would surface here
    assert sorted(h) == sorted(full)
    for k in ("order", "score", "keep", "c_sim", "c_order"):
        assert h[k].shape == (0,) and h[k].dtype == full[k].dtype, k
    assert h["seq"].shape == (0, T) and h["att2"].shape == h["node"].shape == (2, T1) and h["c_first"].shape == (2,)
    assert h["a_words"].shape == (a["scorer"].arena_words(0, 2),) and not h["a_words"].any()
    for e, j in zip(g["scorer"].unpack(h["g_words"], h["g_plan"]), g["index"][:2]):
        _same(e, g["scorer"].empty_entry(j), "empty grounding entry")
    assert [e["drawn"].tolist() for e in d_scorer.unpack(plan, h["d_int"], h["d_f64"])] == [[0, 0], [0, 0]]


def test_caption_images_with_every_option_equals_the_runs_with_one(golden):
    """The small model and images of tests/test_grounding_score_gpu.py; "alone" for accuracy= and grounding= means together with consensus=,
    whose first choice they take (so does the `"grounding"` entry, which is compared with the consensus= run for that reason)."""
    import subgc.models as models
    from subgc import synthetic
    from test_grounding_score_gpu import _grd_case
    out, meta, opt, w, _ = _grd_case(golden, "subgc")
    opt.caption_model = "topdown"
    m = models.setup(opt)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    m = m.to(DEV).eval()
    imgs, vocab = meta["cases"]["subgc"], meta["vocab"]
    dev = [{k: v.to(DEV) for k, v in synthetic.make_test_batch(i["M"], D=opt.att_feat_size, seed=i["seed"], fc_size=opt.att_feat_size,
                                                               node_pool=i["pool"]).items()} for i in imgs]
    infos, ids = [{"id": i["id"]} for i in imgs], [i["id"] for i in imgs]
    kw = dict(sample_max=1, beam_size=1, return_att=1)
    rng = np.random.default_rng(21)
    words = list(vocab.values())
    sents = lambda n: [[[words[int(x)] for x in rng.integers(0, len(words), size=int(rng.integers(2, 8)))] for _ in range(2)] for _ in range(n)]
    rr = consensus.ConsensusReranker(consensus.ConsensusCorpus(sents(8), vocab, device=DEV), k=3, m=4)
    fmeta, arr = GG.load()
    g_refs = GG.references(fmeta, arr, "grd_subgc_0", device=DEV)
    opts = {"consensus": {"reranker": rr, "nn": {k: [int(x) for x in rng.choice(8, 3, replace=False)] for k in ids}, "top_k": 2},
            "diversity": {"scorer": diversity.DiversityScorer(None, 2, ix_to_word=vocab), "top_n": (2, 100), "seed": 2019},
            "accuracy": {"scorer": accuracy.AccuracyScorer(accuracy.AccuracyReferences(sents(len(ids)), vocab, device=DEV), 2),
                         "index": {k: j for j, k in enumerate(ids)}},
            "grounding": {"scorer": grounding.GroundingScorer(g_refs), "index": {k: g_refs.index[str(k)] for k in ids},
                          "boxes": {k: out[f"subgc_{k}_boxes"] for k in ids}, "img_wh": {i["id"]: i["wh"] for i in imgs}}}
    run = lambda group=256, **on: eval_glue.caption_images(m, dev, infos, vocab, kw, group=group, **{k: opts[k] for k in on})
    plain, cons, every = run(), run(consensus=1), run(consensus=1, diversity=1, accuracy=1, grounding=1)
    div, acc, grd = run(diversity=1), run(consensus=1, accuracy=1), run(consensus=1, grounding=1)
    assert max(len(p["caption"]) for p in plain) > 1
    for j, p in enumerate(every):
        assert sorted(p) == sorted(list(plain[j]) + ["consensus_rerank_ind", "consensus_sim", "diversity", "accuracy", "grounding_score"])
        _same({k: p[k] for k in plain[j] if k != "grounding"}, {k: v for k, v in plain[j].items() if k != "grounding"}, "plain")
        _same({k: p[k] for k in ("consensus_rerank_ind", "consensus_sim", "grounding")}, {k: cons[j][k] for k in ("consensus_rerank_ind", "consensus_sim", "grounding")}, "consensus")
        assert p["grounding"]["subg_index"] == int(p["consensus_rerank_ind"][0]) == p["accuracy"]["top1_row"]
        _same(p["diversity"], div[j]["diversity"], "diversity")
        _same(p["accuracy"], acc[j]["accuracy"], "accuracy")
        _same(p["grounding_score"], grd[j]["grounding_score"], "grounding_score")
    # one image per decode batch: the same entries.  The sGPN scores are the model's own: their sums run in another order in a batch of
    # another shape, a few fp32 roundings apart (2^-18 relative leaves room for 64); the ranking they give must not move.
    for p, q in zip(run(group=1, consensus=1, diversity=1, accuracy=1, grounding=1), every):
        np.testing.assert_allclose(p.pop("subgraph_score"), q["subgraph_score"], rtol=2.0 ** -18, atol=0)
        _same(p, {k: v for k, v in q.items() if k != "subgraph_score"}, "group=1")
