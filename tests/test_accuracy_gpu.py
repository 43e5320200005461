"""Accuracy scores on the device (csrc/accuracy.hip through include/subgc_metrics_hip.h): parity with the fixture the reference's own scorers
wrote -- material, picks and oracle material exactly and completely, values within the bounds of DESIGN 4.I -- the shapes at which the
kernels can still go wrong against the plain restatement of tests/accuracy_golden.py, equal bits between runs, and debug bounds mode.

Measured on the fixture on an MI355X (first test, printed; relative): sentence BLEU 3.9e-16, CIDEr 5.3e-16, ROUGE-L 0."""
import os

import numpy as np
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

import accuracy_golden as G
from subgc import accuracy, ops
from subgc.accuracy import SubgcError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def case():
    meta, arr = G.load()
    refs = accuracy.AccuracyReferences(G.fixture_refs(arr), G.vocab(meta["V"]), device=DEV)
    return meta, arr, refs


def within(worst):
    return worst[0] <= G.BLEU_TOL and worst[1] <= G.CIDER_TOL and worst[2] <= G.ROUGE_TOL


def test_fixture_parity_rows_picks_and_corpus(case):
    meta, arr, refs = case
    seq = torch.from_numpy(arr["seq"].astype(np.int64)).to(DEV)
    b = arr["bounds"].tolist()
    top = [0.0, 0.0, 0.0]
    for q, N in enumerate(meta["oracle_nums"]):
        per = accuracy.AccuracyScorer(refs, N).score(seq, b, list(range(len(b) - 1)))
        worst = G.compare(per, G.fixture_per_image(meta, arr, q))           # integers, picks, picked material: ==, every image
        s = accuracy.summarize(per)
        corpus = [G.rel([s[n] for n in accuracy.NAMES[:4]] + [s["oracle"][n] for n in accuracy.NAMES[:4]], arr["top1"][:4].tolist() + arr["oracle"][q, :4].tolist()),
                  G.rel([s["CIDEr"], s["oracle"]["CIDEr"]], [arr["top1"][4], arr["oracle"][q, 4]]),
                  G.rel([s["ROUGE_L"], s["oracle"]["ROUGE_L"]], [arr["top1"][5], arr["oracle"][q, 5]])]
        print(f"oracle_num {N}: max relative difference BLEU {worst[0]:.3g} CIDEr {worst[1]:.3g} ROUGE-L {worst[2]:.3g}; corpus {corpus}")
        assert corpus[0] == 0.0                                              # corpus BLEU comes from the integers
        top = [max(a, c, d) for a, c, d in zip(top, worst, corpus)]
    print("measured maxima over the fixture (BLEU, CIDEr, ROUGE-L):", top)
    assert within(top), top


def random_case(rng, I, n_ref_img, T, ref_lens, R_set, n_rows, max_id=60):
    words = lambda n: [int(x) for x in rng.integers(1, max_id + 1, size=n)]
    ref_ids = []
    for j in range(n_ref_img):
        R = int(R_set[j % len(R_set)])
        ref_ids.append([words(int(ref_lens[(j + r) % len(ref_lens)])) for r in range(R)])
    index = [int(x) for x in rng.integers(0, n_ref_img, size=I)]
    cands, bounds = [], [0]
    for i in range(I):
        for _ in range(int(n_rows[i % len(n_rows)])):
            src = ref_ids[index[i]][int(rng.integers(len(ref_ids[index[i]])))]
            a = int(rng.integers(0, max(1, len(src))))
            c = list(src[a:a + int(rng.integers(0, T + 1))])
            if c:                                                          # one word no reference holds: no two rows share a precision by chance
                c[int(rng.integers(len(c)))] = max_id + 1
            cands.append(c[:T])
        bounds.append(len(cands))
    return ref_ids, index, cands, bounds


def device_refs(ref_ids, V):
    return accuracy.AccuracyReferences([[[f"w{x}" for x in cap] for cap in caps] for caps in ref_ids], G.vocab(V), device=DEV)


def to_seq(cands, T, dtype):
    seq = np.zeros((len(cands), T), np.int64)
    for r, c in enumerate(cands):
        seq[r, :len(c)] = c
    return torch.from_numpy(seq).to(DEV).to(dtype)


def no_near_tie(want, N):
    """The arg-max runs over the device's own values: a case generated here must not hold a near-tie (duplicates are exact ties)."""
    for e in want:
        for k in range(4):
            col = e["values"][:min(e["n"], N), k]
            others = col[col != col.max()]
            if col.max() > 0 and len(others) and (col.max() - others.max()) / col.max() <= 1e-9:
                return False
    return True


def shape_case(T):
    """The first seed whose case holds no near-tie, judged on the restatement alone."""
    for seed in range(100 + T, 160 + T):
        case = build_shape_case(T, seed)
        if all(no_near_tie(G.restate(case[2], case[3], case[1], case[0], N, rows=case[4]), N) for N in (1, 5, 20, 1000)):
            return case
    raise AssertionError("no seed without a near-tie")


def build_shape_case(T, seed):
    rng = np.random.default_rng(seed)
    n_rows = [1, 130, 7, 2, 33, 21, 20, 3, 5, 1, 19, 4] + [2, 3] * 8 + [6, 1]                                    # the last image has one row
    ref_ids, index, cands, bounds = random_case(rng, 30, 8, T, [1, 64, 65, 128, 256, 9, 12], [1, 32, 3, 5], n_rows)
    ref_ids[0][0][0], cands[0][:] = 65535, [65535] + cands[0][1:]         # ids 1 and 65 535
    ref_ids[1][0][0] = 1
    cands[5] = []                                                          # an empty row
    first0 = list(cands[7])                                                # row 7 gets a 0 in front on the device: it ends there
    cands[7] = []
    return ref_ids, index, cands, bounds, G.restate_rows(cands, bounds, index, ref_ids), first0


@pytest.mark.parametrize("T,dtype", [(1, torch.int64), (63, torch.int32), (64, torch.int64)])
def test_shapes_against_the_restatement(T, dtype):
    ref_ids, index, cands, bounds, rows, first0 = shape_case(T)
    refs = device_refs(ref_ids, 65535)
    seq = to_seq(cands, T, dtype)
    seq[7, 1:len(first0)] = torch.tensor(first0[1:], device=DEV, dtype=dtype)      # words after a leading 0 are not read
    for N in (1, 5, 20, 1000):
        want = G.restate(cands, bounds, index, ref_ids, N, rows=rows)
        got = accuracy.AccuracyScorer(refs, N).score(seq, bounds, index)
        assert within(G.compare(got, want))
    # a batch of one image, and explicit top-1 rows
    a, b = bounds[1], bounds[2]
    first = [5]
    got = accuracy.AccuracyScorer(refs, 20).score(seq[a:b].contiguous(), [0, b - a], [index[1]], first=first)
    assert within(G.compare(got, G.restate(cands[a:b], [0, b - a], [index[1]], ref_ids, 20, first=first)))


def test_remove_bad_endings_trims_like_decode_sequence():
    from subgc.eval_glue import BAD_ENDINGS
    vocab = {str(i + 1): w for i, w in enumerate(("cat", "dog", "sits", "runs") + BAD_ENDINGS[:4])}      # ids 5 .. 8 are bad endings
    R = [[["cat", "sits", "on", "dog"], ["dog", "runs"]], [["with", "in"], ["cat"]]]
    refs = accuracy.AccuracyReferences(R, vocab, device=DEV)
    ref_ids = [[refs.encode(c) for c in caps] for caps in R]
    cands = [[1, 3, 7, 5], [2, 4], [5, 6, 7], [1, 5]]                      # row 2 is nothing but bad endings: kept whole
    seq = to_seq(cands, 6, torch.int64)
    got = accuracy.AccuracyScorer(refs, 5).score(seq, [0, 2, 4], [0, 1], remove_bad_endings=1)
    bad = {5, 6, 7, 8}
    want = G.restate([G.trim(c, bad) for c in cands], [0, 2, 4], [0, 1], ref_ids, 5)
    assert G.trim(cands[0], bad) == [1, 3] and G.trim(cands[2], bad) == [5, 6, 7]
    assert within(G.compare(got, want))
    plain = accuracy.AccuracyScorer(refs, 5).score(seq, [0, 2, 4], [0, 1])
    assert plain[0]["material"][0, 0] == 4 and got[0]["material"][0, 0] == 2


def test_two_runs_give_equal_bits(case):
    meta, arr, refs = case
    seq = torch.from_numpy(arr["seq"].astype(np.int32)).to(DEV)
    b = arr["bounds"].tolist()
    sc = accuracy.AccuracyScorer(refs, 20)
    one, two = sc.score(seq, b, list(range(len(b) - 1))), sc.score(seq, b, list(range(len(b) - 1)))
    for x, y in zip(one, two):
        assert all(np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes() for k in x)


def test_debug_bounds_reports_a_bad_seg_and_a_bad_image_index(case):
    meta, arr, refs = case
    seq = torch.from_numpy(arr["seq"][:40].astype(np.int64)).to(DEV)
    sc = accuracy.AccuracyScorer(refs, 5)
    arena = torch.empty(sc.arena_words(40, 3), device=DEV, dtype=torch.int32)
    with ops.debug_bounds(True):
        tab = ops.upload([0, 30, 10, 40, 0, 1, 2], torch.int32, DEV)
        with pytest.raises(SubgcError, match=r"seg \(row boundaries of the images\) is not monotone inside \[0, 40\].*first at image 1: 30 \.\. 10"):
            sc.enqueue(seq, tab, 3, tab[4:], None, 0, arena)
        tab = ops.upload([0, 10, 30, 40, 0, 40, 2], torch.int32, DEV)
        with pytest.raises(SubgcError, match="img_ref"):
            sc.enqueue(seq, tab, 3, tab[4:], None, 0, arena)
        tab = ops.upload([0, 10, 30, 40, 0, 1, 2], torch.int32, DEV)
        sc.enqueue(seq, tab, 3, tab[4:], None, 0, arena)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ inside the decode batch's own pass
def _glue_refs(vocab, n_img=5, seed=5):
    """Reference captions of `n_img` images over the model's words plus two words the model does not know."""
    rng = np.random.default_rng(seed)
    words = [vocab[str(i)] for i in range(1, 60)] + ["zz1", "zz2"]
    return [[[words[min(int(x), len(words)) - 1] for x in rng.zipf(1.3, size=int(rng.integers(1, 14)))] for _ in range(int(rng.integers(1, 6)))]
            for _ in range(n_img)]


def _same_entry(a, b):
    assert sorted(a) == sorted(b)
    for key in a:
        assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), key


def _stand_alone(scorer, preds, index, first=None):
    seq, bounds = accuracy.encode_predictions(preds, scorer.refs)
    return scorer.score(torch.from_numpy(seq).to(DEV), bounds, [index[p["image_id"]] for p in preds], first=first)


@pytest.mark.parametrize("rbe", [0, 1])
def test_caption_images_with_accuracy_end_to_end(golden, rbe):
    import inspect
    from subgc import consensus, diversity, eval_glue
    from test_consensus_gpu import _glue_model
    m, images, infos = _glue_model(golden)
    kw = dict(sample_max=1, beam_size=1, return_att=1, remove_bad_endings=0)
    vocab = {str(i): f"w{i}" for i in range(1, 60)}
    plain = eval_glue.caption_images(m, images, infos, vocab, kw)
    last = [s.split()[-1] for p in plain for s in p["caption"] if s]
    common = [w for w, _ in sorted({w: last.count(w) for w in set(last)}.items(), key=lambda t: (-t[1], t[0]))][:3]
    for w, name in zip(common, ("the", "of", "a")):                       # the most frequent last words become dangling function words
        vocab[w[1:]] = name
    kw["remove_bad_endings"] = rbe
    refs = accuracy.AccuracyReferences(_glue_refs(vocab), vocab, device=DEV)
    scorer = accuracy.AccuracyScorer(refs, 5)
    index = {1000: 4, 1001: 0, 1002: 2}
    acc = {"scorer": scorer, "index": index}
    assert inspect.signature(eval_glue.caption_images).parameters["accuracy"].default is None       # off by default
    before = eval_glue.caption_images(m, images, infos, vocab, kw)
    after = eval_glue.caption_images(m, images, infos, vocab, kw, accuracy=acc)
    if rbe:
        assert any(len(a.split()) < len(b.split()) for p0, p in zip(before, plain) for a, b in zip(p0["caption"], p["caption"]))
    for p0, p1 in zip(before, after):
        assert set(p1) - set(p0) == {"accuracy"}
        for key, v in p0.items():                                         # nothing that was there changes, key for key
            if key == "grounding":
                assert sorted(p1[key]) == sorted(v) and all(np.array_equal(p1[key][k], v[k]) for k in v)
            elif isinstance(v, np.ndarray):
                np.testing.assert_array_equal(p1[key], v)
            else:
                assert p1[key] == v
        assert p1["accuracy"]["n"] == len(p1["caption"]) and p1["accuracy"]["top1_row"] == 0
    # the strings are already trimmed: the stand-alone scorer on them, without trimming, is the same computation
    for p1, e in zip(after, _stand_alone(scorer, after, index)):
        _same_entry(p1["accuracy"], e)
    assert max(p["accuracy"]["values"][:, 0].max() for p in after) > 0      # something matched: the check is not about zeros
    for group in (1, 2):                                                  # the batch an image falls into cannot change its result
        for p1, p2 in zip(after, eval_glue.caption_images(m, images, infos, vocab, kw, group=group, accuracy=acc)):
            _same_entry(p1["accuracy"], p2["accuracy"])
    # with consensus= the top-1 row is the re-ranker's first choice, taken on the device; with diversity= all three ride together
    rng = np.random.default_rng(11)
    words = [vocab[str(i)] for i in range(1, 60)]
    sents = [[[words[min(int(x), len(words)) - 1] for x in rng.zipf(1.4, size=int(rng.integers(1, 12)))] for _ in range(3)] for _ in range(40)]
    rr = consensus.ConsensusReranker(consensus.ConsensusCorpus(sents, vocab, device=DEV), k=8, m=10)
    cons = {"reranker": rr, "nn": {info["id"]: [int(x) for x in rng.choice(40, 8, replace=False)] for info in infos}, "top_k": 4}
    div = {"scorer": diversity.DiversityScorer(None, 5, ix_to_word=vocab), "top_n": (3, 100), "seed": 2019}
    only = eval_glue.caption_images(m, images, infos, vocab, kw, consensus=cons, diversity=div)
    both = eval_glue.caption_images(m, images, infos, vocab, kw, consensus=cons, diversity=div, accuracy=acc)
    firsts = [int(p["consensus_rerank_ind"][0]) for p in both]
    print("re-ranker's first choices:", firsts)
    for p0, p1, e in zip(only, both, _stand_alone(scorer, both, index, first=firsts)):
        assert set(p1) - set(p0) == {"accuracy"} and p1["accuracy"]["top1_row"] == p1["consensus_rerank_ind"][0]
        np.testing.assert_array_equal(p1["consensus_rerank_ind"], p0["consensus_rerank_ind"])
        assert p1["consensus_sim"].tobytes() == p0["consensus_sim"].tobytes()
        _same_entry(p1["diversity"], p0["diversity"])
        _same_entry(p1["accuracy"], e)
    s = accuracy.summarize([p["accuracy"] for p in both])
    assert s["images"] == 3 and 0 <= s["Bleu_1"] <= s["oracle"]["Bleu_1"] <= 1
    with pytest.raises(ValueError, match="sct"):
        eval_glue.caption_images(m, images, infos, vocab, dict(kw, sct=1), accuracy=acc)
    with pytest.raises(ValueError, match=r"no reference image for image ids \[1002\]"):
        eval_glue.caption_images(m, images, infos, vocab, kw, accuracy={"scorer": scorer, "index": {1000: 0, 1001: 1}})


class _Traffic(TorchDispatchMode):
    """Counts device -> host copies (the method of tests/test_no_aten_gpu.py, turned to the copies it lets through)."""

    def __init__(self):
        super().__init__()
        self.to_host = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        r = func(*args, **(kwargs or {}))
        name = str(func)
        if "copy_" in name or "_to_copy" in name:
            src = args[1] if "copy_" in name and "_to_copy" not in name else args[0]
            dst = args[0] if "copy_" in name and "_to_copy" not in name else r
            if torch.is_tensor(src) and torch.is_tensor(dst) and src.is_cuda and not dst.is_cuda:
                self.to_host += 1
        return r


@pytest.mark.skipif(os.getenv("SUBGC_POISON_EMPTY") == "1", reason="the poisoned run fills every torch.empty buffer with an ATen fill_ by design")
def test_eval_collect_with_accuracy_is_one_copy_no_aten_kernel_and_changes_nothing_else(case):
    from subgc import consensus
    from test_no_aten_gpu import Watch
    meta, arr, refs = case
    seq = torch.from_numpy(arr["seq"].astype(np.int64)).to(DEV)
    rows, T = seq.shape
    b = arr["bounds"].tolist()
    I = len(b) - 1
    score = torch.linspace(1, 0, rows, device=DEV)                        # descending: the ranking keeps the fixture's caption order
    keep = torch.arange(rows, device=DEV)
    AL = torch.rand(T + 1, rows, 9, device=DEV)
    idx = torch.arange(9, device=DEV).repeat(rows, 1)
    vocab = G.vocab(meta["V"])
    rr = consensus.ConsensusReranker(consensus.ConsensusCorpus(G.fixture_refs(arr), vocab, device=DEV), k=6, m=8)
    cons = {"reranker": rr, "nn": [[(i + d) % I for d in range(1, 7)] for i in range(I)], "top_k": 4}
    scorer = accuracy.AccuracyScorer(refs, 20)
    acc = {"scorer": scorer, "index": list(range(I))}

    def run(**kw):
        return ops.eval_collect(score, keep, seq, b, AL=AL, idx=idx, **kw)

    run(consensus=cons, accuracy=acc)
    torch.cuda.synchronize()
    with Watch() as w, _Traffic() as t:
        h = run(consensus=cons, accuracy=acc)
    torch.cuda.synchronize()
    assert not w.seen, dict(w.seen)
    assert t.to_host == 1, t.to_host                                      # still ONE device -> host copy per batch
    # accuracy=None: the same keys and bits as a call that never heard of it, and the other outputs do not move when it is on
    off, without = run(consensus=cons, accuracy=None), run(consensus=cons)
    assert sorted(off) == sorted(without) == sorted(k for k in h if k != "a_words")
    for key in off:
        assert off[key].tobytes() == without[key].tobytes() == h[key].tobytes(), key
    plain, plain_acc = run(), run(accuracy=acc)
    assert sorted(plain_acc) == sorted(list(plain) + ["a_words"]) and all(plain[k].tobytes() == plain_acc[k].tobytes() for k in plain)
    # the entries are the stand-alone scorer's, top-1 from the re-ranker's device-side first choice / row 0
    for got, want in ((h, scorer.score(seq, b, list(range(I)), first=[int(x) for x in h["c_first"]])), (plain_acc, scorer.score(seq, b, list(range(I))))):
        for x, y in zip(scorer.unpack(got["a_words"], b), want):
            _same_entry(x, y)
    assert any(int(x) != 0 for x in h["c_first"])                         # the re-ranker did move some top-1
    assert within(G.compare(scorer.unpack(plain_acc["a_words"], b), G.fixture_per_image(meta, arr, meta["oracle_nums"].index(20))))


def test_score_predictions_is_the_drop_in_and_prints_the_reference_lines(case, capsys):
    meta, arr, refs = case
    cands, b = G.rows_to_ids(arr["seq"]), arr["bounds"]
    preds = [{"image_id": 1000 + i, "caption": [" ".join(f"w{x}" for x in c) for c in cands[b[i]:b[i + 1]]]} for i in range(len(b) - 1)]
    by_id = {1000 + i: caps for i, caps in enumerate(G.fixture_refs(arr))}
    q = meta["oracle_nums"].index(20)
    s, per = accuracy.score_predictions(preds[::-1], by_id, G.vocab(meta["V"]), oracle_num=20, device=DEV)      # any order of the list
    worst = G.compare(per[::-1], G.fixture_per_image(meta, arr, q))
    assert within(worst)
    assert [s[n] for n in accuracy.NAMES[:4]] == arr["top1"][:4].tolist() and [s["oracle"][n] for n in accuracy.NAMES[:4]] == arr["oracle"][q, :4].tolist()
    assert G.rel([s["CIDEr"], s["oracle"]["CIDEr"]], [arr["top1"][4], arr["oracle"][q, 4]]) <= G.CIDER_TOL
    assert G.rel([s["ROUGE_L"], s["oracle"]["ROUGE_L"]], [arr["top1"][5], arr["oracle"][q, 5]]) <= G.ROUGE_TOL
    out = capsys.readouterr().out.splitlines()
    assert out[:6] == ["%s: %0.3f" % (n, s[n]) for n in accuracy.NAMES] and "The following is top-20: " in out
    assert out[-6:] == ["oracle {}: {}".format(n, s["oracle"][n]) for n in accuracy.NAMES[:4]] + [
        "oracle cider: {}".format(s["oracle"]["CIDEr"]), "oracle rouge: {}".format(s["oracle"]["ROUGE_L"])]
    accuracy.score_predictions(preds[:2], {k: by_id[k] for k in (1000, 1001)}, G.vocab(meta["V"]), oracle_num=1, device=DEV)
    assert len(capsys.readouterr().out.splitlines()) == 6                 # oracle_num 1: the six top-1 lines alone
    with pytest.raises(SubgcError, match=r"no reference captions for image ids \[1001\]"):
        accuracy.score_predictions(preds[:2], {1000: by_id[1000]}, G.vocab(meta["V"]), device=DEV)


def _shard_worker(rank, world, port, q):
    import test_parallel_decode as P
    P._paths()
    import os
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    from subgc import eval_glue, parallel
    torch.cuda.set_device(0)
    parallel.init_distributed("gloo")
    m, D = P._gpu_model()
    images = [{k: v.to(DEV) for k, v in b.items()} for b in P._images(D)]
    refs = accuracy.AccuracyReferences(_glue_refs(P.VOCAB, len(images)), P.VOCAB, device=DEV)
    acc = {"scorer": accuracy.AccuracyScorer(refs, 5), "index": {50 + i: i for i in range(len(images))}}
    preds = eval_glue.caption_images(m, images, [{"id": 50 + i} for i in range(len(images))], P.VOCAB, P.KW, group=2, shard=True, accuracy=acc)
    q.put((rank, [(p["image_id"], {k: np.asarray(v) for k, v in p["accuracy"].items()}) for p in preds]))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_sharded_decode_gathers_the_accuracy_entries():
    """Two ranks on one device caption their shares; every rank ends with every image's entry, equal to the one-process run's."""
    import torch.multiprocessing as mp
    import test_parallel_decode as P
    from subgc import eval_glue
    world, port = 2, P._free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_shard_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = P._collect(q, procs, 500)
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    m, D = P._gpu_model()
    images = [{k: v.to(DEV) for k, v in b.items()} for b in P._images(D)]
    refs = accuracy.AccuracyReferences(_glue_refs(P.VOCAB, len(images)), P.VOCAB, device=DEV)
    acc = {"scorer": accuracy.AccuracyScorer(refs, 5), "index": {50 + i: i for i in range(len(images))}}
    want = eval_glue.caption_images(m, images, [{"id": 50 + i} for i in range(len(images))], P.VOCAB, P.KW, accuracy=acc)
    assert len(res) == world and len(images) > world
    for _, got in res:
        assert [i for i, _ in got] == [p["image_id"] for p in want]
        for (_, e), p in zip(got, want):
            _same_entry(e, p["accuracy"])
    s = accuracy.summarize([p["accuracy"] for p in want])
    assert s == accuracy.summarize([e for _, e in res[0][1]])             # corpus numbers accumulate across ranks
