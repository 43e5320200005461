"""The nearest-image search on the device (subgc.neighbours, csrc/neighbours.hip, include/subgc_neighbours_hip.h) against the fixture
the reference's own `find_NNimg` wrote (tests/golden/make_golden_neighbours.py).

Distances are compared BIT FOR BIT with the fixture's scipy `cdist` matrix (NaN as NaN: scipy's inf - inf carries the x86 sign bit, the
device's does not).  Lists are compared bit for bit with the contract's restatement (`find_nn_restatement`) and with the reference's
under the tie rule of tests/neighbours_golden.py.  No tolerance appears anywhere in this file."""
import numpy as np
import pytest
import torch

import neighbours_golden as G
from subgc import consensus, eval_glue, neighbours as NB, ops
from subgc._lib import SubgcError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
META, ARR = G.load()
CASES = sorted(META["cases"])
FINITE = [n for n in CASES if not META["cases"][n]["nonfinite"]]


def _up(a):
    return torch.from_numpy(np.array(a)).to(DEV)                             # a copy: the shared features are read-only


def _same_distances(got, ref):
    nan = np.isnan(ref)
    bad = np.argwhere((got.view(np.uint64) != ref.view(np.uint64)) & ~nan)
    assert (np.isnan(got) == nan).all()
    assert not len(bad), (bad[:4].tolist(), [(float(got[a, b]).hex(), float(ref[a, b]).hex()) for a, b in bad[:4]])


_DIST = {}


def device_dist(name):
    """The device distance matrix of a case, computed once and left unchanged."""
    if name not in _DIST:
        te, tr = G.features(META, ARR, name)
        d = torch.empty(len(te), len(tr), device=DEV, dtype=torch.float64)
        ops.nn_dist(_up(te), _up(tr), d)
        _DIST[name] = d
    return _DIST[name]


@pytest.mark.parametrize("name", CASES)
def test_distances_are_scipys_bits(name):
    _same_distances(device_dist(name).cpu().numpy(), ARR[name + "_cdist"])


@pytest.mark.parametrize("pads", [(3, 5, 7), (2, 4, 6)])
@pytest.mark.parametrize("name", CASES)
def test_distances_with_strided_operands_and_poisoned_padding(name, pads):
    """Row pitches beyond D / N, NaN in every pad element of the inputs and a sentinel around the output: a pad element that entered a
    sum would make it NaN, a store beyond N would overwrite the sentinel.  Odd and even pitches: the 8-byte and the 16-byte read path,
    the latter also with an odd D (its last column is a lone 8-byte read)."""
    te, tr = G.features(META, ARR, name)
    (Q, D), N = te.shape, len(tr)
    q = torch.full((Q, D + pads[0]), float("nan"), device=DEV, dtype=torch.float64)
    x = torch.full((N, D + pads[1]), float("nan"), device=DEV, dtype=torch.float64)
    out = torch.full((Q + 1, N + pads[2]), -7.0, device=DEV, dtype=torch.float64)
    q[:, :D] = _up(te)
    x[:, :D] = _up(tr)
    ops.nn_dist(q[:, :D], x[:, :D], out[:Q, :N])
    h = out.cpu().numpy()
    _same_distances(np.ascontiguousarray(h[:Q, :N]), ARR[name + "_cdist"])
    assert (h[Q] == -7.0).all() and (h[:, N:] == -7.0).all()


@pytest.mark.parametrize("name", CASES)
def test_lists_and_values_are_the_contracts_bits_for_every_k(name):
    c = META["cases"][name]
    ref_d = ARR[name + "_cdist"]
    order = np.argsort(G.keys(ref_d), axis=1, kind="stable")
    Q, N = ref_d.shape
    for src, d_dev in (("fixture", _up(ref_d)), ("device", device_dist(name))):
        h_d = d_dev.cpu().numpy()
        for k in c["ks"]:
            idx = torch.full((Q, k), -1, device=DEV, dtype=torch.int32)
            val = torch.full((Q, k), -1.0, device=DEV, dtype=torch.float64)
            ops.nn_select(d_dev, N, k, idx, val)
            np.testing.assert_array_equal(idx.cpu().numpy(), order[:, :k], err_msg=f"{src} k={k}")
            assert val.cpu().numpy().tobytes() == np.take_along_axis(h_d, order[:, :k], 1).tobytes(), (src, k)      # the entries' own bits
            only = torch.full((Q, k), -1, device=DEV, dtype=torch.int32)
            ops.nn_select(d_dev, N, k, only, None)                                                   # val may be NULL
            assert torch.equal(only, idx)
            G.compare_lists(idx.cpu().numpy(), ARR[name + "_lists"], ref_d, k)                      # and the reference's, under the tie rule


def test_select_reads_a_strided_matrix_and_nothing_beyond_n():
    ref_d = ARR["dup_cdist"]
    Q, N = ref_d.shape
    buf = torch.full((Q, N + 9), -1.0, device=DEV, dtype=torch.float64)        # smaller than every distance: read, it would lead every list
    buf[:, :N] = _up(ref_d)
    idx = torch.empty(Q, 100, device=DEV, dtype=torch.int32)
    ops.nn_select(buf[:, :N], N, 100, idx)
    np.testing.assert_array_equal(idx.cpu().numpy(), np.argsort(G.keys(ref_d), axis=1, kind="stable")[:, :100])


def test_refusals_reach_the_caller_with_their_numbers():
    d = torch.zeros(2, 5, device=DEV, dtype=torch.float64)
    with pytest.raises(SubgcError, match=r"k = 6; 1 <= k <= min\(N, 1024\) = 5"):
        ops.nn_select(d, 5, 6, torch.empty(2, 6, device=DEV, dtype=torch.int32))
    with pytest.raises(SubgcError, match="float64"):
        ops.nn_dist(torch.zeros(2, 3, device=DEV), torch.zeros(4, 3, device=DEV, dtype=torch.float64), torch.zeros(2, 4, device=DEV, dtype=torch.float64))
    te, tr = G.features(META, ARR, "nonfinite")
    with pytest.raises(SubgcError, match="training feature row 5 holds a non-finite value"):       # the row with an inf; 1e200 is finite
        NB.ImageIndex(tr, device=DEV)
    ix = NB.ImageIndex(G.features(META, ARR, "plain")[1], device=DEV)
    with pytest.raises(SubgcError, match="holds no row of 97 distances"):
        ix.search(G.features(META, ARR, "plain")[0], k=3, workspace_bytes=100)


# ------------------------------------------------------------------------------------------------ the host module
_INDEX = {}


def index_of(name):
    if name not in _INDEX:
        _INDEX[name] = NB.ImageIndex(G.features(META, ARR, name)[1].astype(np.float32) if "recipe" in META["cases"][name] else
                                     G.features(META, ARR, name)[1], device=DEV)
    return _INDEX[name]


def test_search_is_chunk_invariant_and_reads_no_stale_workspace():
    te, tr = G.features(META, ARR, "dup")
    (Q, _), N = te.shape, len(tr)
    ix = NB.ImageIndex(tr, device=DEV)
    q = _up(te)
    whole_i, whole_d = ix.search(q, k=100)
    assert whole_i.dtype == torch.int32 and whole_d.dtype == torch.float64 and whole_i.shape == whole_d.shape == (Q, 100)
    assert ix._ws.numel() == Q * N
    for rows in (1, 64):                                                   # 65 chunks of one row; a chunk of 64 and one of 1
        ix._ws = torch.full((rows * N + 17,), float("nan"), device=DEV, dtype=torch.float64)      # a poisoned workspace, larger than needed
        i2, d2 = ix.search(q, k=100, workspace_bytes=rows * N * 8 + 7)
        assert ix._ws.numel() == rows * N + 17                             # it was used as it was, not replaced
        assert torch.equal(i2, whole_i) and d2.cpu().numpy().tobytes() == whole_d.cpu().numpy().tobytes()
        assert torch.isnan(ix._ws[rows * N:]).all()                        # and nothing beyond the chunk was written
    lists, dist = NB.find_nn_restatement(te, tr, 100)
    np.testing.assert_array_equal(whole_i.cpu().numpy(), lists)
    assert whole_d.cpu().numpy().tobytes() == np.take_along_axis(dist, lists, 1).tobytes()
    host_i, _ = ix.search(te.astype(np.float32), k=100)                    # a host array of another dtype: converted as the reference converts
    assert torch.equal(host_i, whole_i)


@pytest.mark.parametrize("name", FINITE)
def test_find_nn_is_the_references_list_under_the_tie_rule(name):
    c = META["cases"][name]
    te, _ = G.features(META, ARR, name)
    k = c["num_NNimg"]
    lists = index_of(name).find_nn(te, k=k)
    assert isinstance(lists, list) and isinstance(lists[0], list) and type(lists[0][0]) is int and len(lists) == len(te) and len(lists[0]) == k
    left_out = G.compare_lists(np.asarray(lists), ARR[name + "_lists"], ARR[name + "_cdist"], k)
    assert left_out == c["tie_positions"]
    if c["all_duplicates"]:
        assert lists == [list(range(k))] * len(te)
    elif not c["duplicates"]:
        assert left_out == 0 and lists == ARR[name + "_lists"].tolist()      # no ties: THE reference's lists, position for position


def test_from_annotations_arranges_rows_in_list_order():
    te, tr = G.features(META, ARR, "plain")
    ids = [f"img{j}" for j in range(len(tr))]
    perm = np.random.RandomState(3).permutation(len(tr))
    dct = {ids[j]: tr[j].astype(np.float32).astype(np.float64) for j in range(len(tr))}
    ix = NB.ImageIndex.from_annotations(dct, [{"id": ids[j]} for j in perm], device=DEV)
    lists, _ = NB.find_nn_restatement(te, np.stack([dct[ids[j]] for j in perm]), 10)
    assert ix.find_nn(te, k=10) == lists.tolist()


# ------------------------------------------------------------------------------------------------ in front of the re-rankers
def _golden_rerankers():
    import consensus_bleu_golden as GB
    import consensus_golden as GC
    meta, arr = GC.load()
    sents, _ = GC.corpus_sentences(arr)
    corpus = consensus.ConsensusCorpus(sents, {str(i): GC.word(i) for i in range(1, meta["V"] + 1)}, device=DEV)
    yield "cider", consensus.ConsensusReranker(corpus, k=meta["k"], m=meta["m"]), arr
    meta, arr = GB.load()
    sents, _ = GB.corpus_sentences(arr)
    corpus = consensus.ConsensusCorpus(sents, GB.vocab(meta["V"]), device=DEV)
    for name, p in meta["sets"].items():
        yield "bleu " + name, consensus.BleuConsensusReranker(corpus, k=meta["k"], m=p["m"], ngram=p["n"], fpr=p["fpr"]), arr


def test_a_device_neighbour_tensor_gives_the_host_lists_bits_and_max_caps_is_only_a_capacity():
    for name, rr, arr in _golden_rerankers():
        seq, bounds = _up(arr["cand"]), [int(x) for x in arr["bounds"]]
        nn = [[int(x) for x in r] for r in arr["nn"]]
        o_host, s_host = rr.rerank(seq, bounds, nn)
        true_caps = rr.neighbours(nn)[1]
        d_nn = _up(arr["nn"].astype(np.int32))                                # [I, k + 4]: a pitch beyond k, read in place
        o_dev, s_dev, p_dev = rr.rerank(seq, bounds, d_nn, return_pairs=True)
        bound = rr.caps_bound()
        per_img = np.diff(rr.corpus.cap_off)
        assert bound == int(np.sort(per_img)[-rr.k:].sum()) and true_caps <= bound <= consensus.MAX_CAPS, name
        assert p_dev[0].shape[1] == bound
        for a, b, x, y in zip(o_host, o_dev, s_host, s_dev):
            np.testing.assert_array_equal(a, b, err_msg=name)
            assert x.tobytes() == y.tobytes(), name
        rr._caps_bound = consensus.MAX_CAPS                                   # the largest capacity there is: still the same bits
        o_max, s_max = rr.rerank(seq, bounds, d_nn)
        for a, b, x, y in zip(o_host, o_max, s_host, s_max):
            np.testing.assert_array_equal(a, b, err_msg=name)
            assert x.tobytes() == y.tobytes(), name
        rr._caps_bound = consensus.MAX_CAPS + 1
        with pytest.raises(SubgcError, match=f"hold {consensus.MAX_CAPS + 1} captions; the limit is {consensus.MAX_CAPS}"):
            rr.rerank(seq, bounds, d_nn)
        rr._caps_bound = None
        with pytest.raises(SubgcError, match=r"int32 \["):
            rr.rerank(seq, bounds, d_nn.long())
        with pytest.raises(SubgcError, match=r"int32 \["):
            rr.rerank(seq, bounds, d_nn[:, :rr.k - 1].contiguous())


def _same_value(a, b, key):
    if isinstance(a, dict):
        assert sorted(a) == sorted(b), key
        for k in a:
            _same_value(a[k], b[k], f"{key}.{k}")
    elif isinstance(a, (list, tuple)) and a and isinstance(a[0], (dict, list, tuple, np.ndarray)):
        assert len(a) == len(b), key
        for j, (x, y) in enumerate(zip(a, b)):
            _same_value(x, y, f"{key}[{j}]")
    elif isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        assert np.asarray(a).dtype == np.asarray(b).dtype and np.asarray(a).tobytes() == np.asarray(b).tobytes(), key
    else:
        assert a == b, key


@pytest.mark.parametrize("method,return_att,with_acc", [("cider", 1, True), ("cider", 0, False), ("bleu", 1, False), ("bleu", 0, True)])
def test_caption_images_with_an_index_reproduces_the_host_list_path(golden, method, return_att, with_acc):
    from subgc import accuracy
    from test_accuracy_gpu import _glue_refs
    from test_consensus_gpu import _glue_model
    m, images, infos = _glue_model(golden)
    kw = dict(sample_max=1, beam_size=1, return_att=return_att, remove_bad_endings=1)
    vocab = {str(i): f"w{i}" for i in range(1, 60)}
    rng = np.random.default_rng(11)
    words = [vocab[str(i)] for i in range(1, 60)] + ["zz1", "zz2"]
    sents = [[[words[min(int(x), len(words)) - 1] for x in rng.zipf(1.4, size=int(rng.integers(0, 16)))] for _ in range(int(rng.integers(2, 6)))]
             for _ in range(80)]
    rr = consensus.make_reranker(consensus.ConsensusCorpus(sents, vocab, device=DEV), method, k=10, m=20)
    rs = np.random.RandomState(5)
    train = np.maximum(rs.standard_normal((80, 33)), 0).astype(np.float32)
    train[41] = train[7]                                                      # a duplicated training image
    feats = {info["id"]: np.maximum(rs.standard_normal(33), 0).astype(np.float32) for info in infos}
    feats[infos[1]["id"]] = train[7].copy()                                   # ... that one image is nearest to, at distance 0, twice
    index = NB.ImageIndex(train, device=DEV)
    found = index.find_nn(np.stack([feats[i["id"]] for i in infos]), k=12)
    assert found[1][:2] == [7, 41]
    nn = {info["id"]: l for info, l in zip(infos, found)}
    extra = {}
    if with_acc:
        extra["accuracy"] = {"scorer": accuracy.AccuracyScorer(accuracy.AccuracyReferences(_glue_refs(vocab), vocab, device=DEV), 5),
                             "index": {1000: 4, 1001: 0, 1002: 2}}
    by_list = eval_glue.caption_images(m, images, infos, vocab, kw, consensus={"reranker": rr, "nn": nn, "top_k": 4}, **extra)
    for arg in ({"k_search": 12}, {}, {"workspace_bytes": 80 * 8}):           # lists longer than k, exactly k, one query row per chunk
        by_index = eval_glue.caption_images(m, images, infos, vocab, kw, consensus=dict({"reranker": rr, "index": index, "features": feats, "top_k": 4}, **arg),
                                            **extra)
        for p0, p1 in zip(by_list, by_index):
            assert set(p1) - set(p0) == {"consensus_nn"} and set(p0) <= set(p1)
            for key in p0:
                _same_value(p0[key], p1[key], key)
            assert p1["consensus_nn"].dtype == np.int64 and p1["consensus_nn"].tolist() == nn[p1["image_id"]][:10]
    assert any(len(p["consensus_rerank_ind"]) > 1 for p in by_list)          # something was re-ranked
    split = eval_glue.caption_images(m, images, infos, vocab, kw, group=1, consensus={"reranker": rr, "index": index, "features": feats, "top_k": 4}, **extra)
    # one image per decode batch: the model's own scores depend on the batch in their last bits (with or without this feature), so the
    # host-list path at the same grouping is the yardstick; an image's neighbour list does not depend on the batch at all
    list_split = eval_glue.caption_images(m, images, infos, vocab, kw, group=1, consensus={"reranker": rr, "nn": nn, "top_k": 4}, **extra)
    for p0, p1, p2 in zip(list_split, by_index, split):
        for key in p0:
            _same_value(p0[key], p2[key], key)
        assert p2["consensus_nn"].tolist() == p1["consensus_nn"].tolist()
    with pytest.raises(ValueError, match="exactly one of consensus\\['nn'\\]"):
        eval_glue.caption_images(m, images, infos, vocab, kw, consensus={"reranker": rr, "nn": nn, "index": index, "features": feats})
    with pytest.raises(ValueError, match="exactly one of consensus\\['nn'\\]"):
        eval_glue.caption_images(m, images, infos, vocab, kw, consensus={"reranker": rr})
    with pytest.raises(ValueError, match="consensus\\['features'\\] has no feature vector for image ids \\[1002\\]"):
        eval_glue.caption_images(m, images, infos, vocab, kw, consensus={"reranker": rr, "index": index, "features": {1000: feats[1000], 1001: feats[1001]}})
    with pytest.raises(ValueError, match="consensus\\['nn'\\] has no neighbour list for image ids \\[1002\\]"):       # today's text, unchanged
        eval_glue.caption_images(m, images, infos, vocab, kw, consensus={"reranker": rr, "nn": {1000: nn[1000], 1001: nn[1001]}})
    with pytest.raises(SubgcError, match="k_search = 5 is smaller than the re-ranker's k = 10"):
        eval_glue.caption_images(m, images, infos, vocab, kw, consensus={"reranker": rr, "index": index, "features": feats, "k_search": 5})
